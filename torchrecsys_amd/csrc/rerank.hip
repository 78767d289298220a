// rerank.hip — diversified re-ranking: greedy Maximal-Marginal-Relevance (MMR) selection over each user's candidate
// pool and the intra-list diversity of given lists (model.py recommend_diverse / evaluate_diversity; the rule is the
// contract in include/trs.h "diversified re-ranking", the design in DESIGN.md 4.14).
//
// Both kernels run one workgroup per list of at most TRS_RETRIEVE_KMAX = 128 entries, L lanes per entry: entry
// j = tid / L, part h = tid % L, 128 * L threads.  L = 2 up to Dp = 128 and L = 4 at Dp = 256, so a lane never holds
// more than 64 floats of a row (with two lanes at Dp = 256 the 128-register row spilled to scratch).  The entry's row
// of the trs_neighbour_fold buffer is gathered once, 16 bytes per load, and stays in registers: the lane keeps the
// float4 chunks L * c + h, c < Dp / (4 L).  One row at a time is handed to every entry through LDS (mr_publish_row);
// with the chunks interleaved between an entry's lanes the 16 lanes of a ds_read_b128 group read L consecutive
// 16-byte slots, each a broadcast: no bank conflict.  mr_sim is the inner product of the lane's chunks with the
// published row (four independent fma chains), completed by shuffles among the entry's lanes.
//
// mmr_rerank_kernel<Dp, L>  relevance of every entry (min-max scaled, made non-increasing along the pool), then k - 1
//                        steps: publish the last pick's row | barrier | every entry folds its similarity to that row
//                        into its running penalty, forms m = a * rel - b * pen and a 64-bit key (m's order, then the
//                        lower pool position), wave maximum by shuffles, one partial per wave in LDS | barrier | every
//                        thread reads the partials: the next pick.  k * N * Dp fmas per user instead of the N^2 * Dp
//                        of a full similarity matrix.  No scratch, no float atomics; the one atomic is the error flag's.
// list_ild_kernel<Dp, L> every valid entry's row is published in turn (two LDS buffers: one barrier per row); the
//                        entries behind it add 1 - sim to a float64 register; one thread adds the 128 sums in order.
#include <type_traits>

#include "trs_common.h"

namespace {

constexpr int MR_NMAX = TRS_RETRIEVE_KMAX;  // entries per list
static_assert((MR_NMAX & (MR_NMAX - 1)) == 0, "a position is masked with MR_NMAX - 1");

static inline int mr_dp(int D) {  // the folded buffer's row width (trs_item_fold_bytes)
  int p = 16;
  while (p < D) p <<= 1;
  return p;
}

// ------------------------------------------------------------------------------------------------ shared pieces
// The lane's chunks of row `id` of X (n_pad, Dp).  An entry that is not `ok` reads row 0 (always there) instead of
// branching around the loads, which keeps all of them in flight together; its values are never used: such an entry is
// never published and what it computes is dropped.
template <int Dp, int L>
__device__ __forceinline__ void mr_gather_row(const float* X, int64_t id, bool ok, int h, float4 (&row)[Dp / (4 * L)]) {
  const float4* src = reinterpret_cast<const float4*>(X + (ok ? id : 0) * Dp) + h;
#pragma unroll
  for (int c = 0; c < Dp / (4 * L); ++c) row[c] = src[L * c];
}

// The L lanes of one entry put its row into buf (Dp floats, 16-byte aligned).
template <int Dp, int L>
__device__ __forceinline__ void mr_publish_row(float* buf, const float4 (&row)[Dp / (4 * L)], int h) {
  float4* dst = reinterpret_cast<float4*>(buf) + h;
#pragma unroll
  for (int c = 0; c < Dp / (4 * L); ++c) dst[L * c] = row[c];
}

// <the entry's row, the row in buf> in fp32; every lane of the entry gets the same value.
template <int Dp, int L>
__device__ __forceinline__ float mr_sim(const float* buf, const float4 (&row)[Dp / (4 * L)], int h) {
  const float4* b = reinterpret_cast<const float4*>(buf) + h;
  float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
#pragma unroll
  for (int c = 0; c < Dp / (4 * L); ++c) {
    const float4 x = b[L * c];
    acc.x = __builtin_fmaf(row[c].x, x.x, acc.x);
    acc.y = __builtin_fmaf(row[c].y, x.y, acc.y);
    acc.z = __builtin_fmaf(row[c].z, x.z, acc.z);
    acc.w = __builtin_fmaf(row[c].w, x.w, acc.w);
  }
  return trs_group_sum<L>((acc.x + acc.y) + (acc.z + acc.w));
}

// Selection key of an unselected entry: m's order (a NaN below every number, -0.0 = +0.0), then the lower position.
// Never 0: the low word is at least 1.
__device__ __forceinline__ uint64_t mr_key(float m, int pos) {
  uint32_t o = 0;
  if (m == m) {
    if (m == 0.f) m = 0.f;
    const uint32_t b = __float_as_uint(m);
    o = (b & 0x80000000u) ? ~b : (b | 0x80000000u);
  }
  return ((uint64_t)o << 32) | (uint64_t)(uint32_t)(MR_NMAX - pos);
}

__device__ __forceinline__ uint64_t mr_wave_max(uint64_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t other = __shfl_xor((unsigned long long)v, o, 64);
    v = other > v ? other : v;
  }
  return v;
}

// ------------------------------------------------------------------------------------------------ MMR
struct MmrArgs {
  const float* X;  // (n_pad, Dp)
  int64_t n_items;
  const int64_t* pool_ids;   // (n_q, N)
  const float* pool_scores;  // (n_q, N)
  int N, k;
  float a, b;  // 1 - lambda, lambda
  int64_t* ids_out;   // (n_q, k)
  float* scores_out;  // (n_q, k)
  int32_t* pos_out;   // (n_q, k) or NULL
  int32_t* err;       // or NULL
};

template <int Dp, int L>
__global__ __launch_bounds__(MR_NMAX * L) void mmr_rerank_kernel(const MmrArgs g) {
  constexpr int THREADS = MR_NMAX * L, WAVES = THREADS / 64;
  __shared__ __attribute__((aligned(16))) float rowbuf[Dp];
  __shared__ float v[MR_NMAX];    // the pool's scores
  __shared__ float rel[MR_NMAX];  // scaled relevance before the running minimum
  __shared__ int okf[MR_NMAX];    // 1: a valid entry
  __shared__ int picks[MR_NMAX];
  __shared__ uint64_t part[WAVES];

  const int tid = threadIdx.x, j = tid / L, h = tid % L;
  const int N = g.N;
  const int64_t base = (int64_t)blockIdx.x * N;

  int64_t id = -1;
  float vj = 0.f;
  if (j < N) {
    id = g.pool_ids[base + j];
    vj = g.pool_scores[base + j];
  }
  const bool valid = (uint64_t)id < (uint64_t)g.n_items;  // never an address otherwise
  if (!valid && id != -1 && h == 0 && g.err) atomicOr(g.err, 1);
  if (h == 0) {
    v[j] = vj;
    okf[j] = valid ? 1 : 0;
  }
  float4 row[Dp / (4 * L)];
  mr_gather_row<Dp, L>(g.X, id, valid, h, row);
  __syncthreads();

  // v_min, v_max, the first valid position and the number of valid entries: every thread scans the pool in LDS
  float vmin = 0.f, vmax = 0.f;
  int first = -1, n_valid = 0;
  for (int i = 0; i < N; ++i) {
    if (!okf[i]) continue;
    const float x = v[i];
    if (first < 0) {
      first = i;
      vmin = x;
      vmax = x;
    } else {
      vmin = x < vmin ? x : vmin;
      vmax = x > vmax ? x : vmax;
    }
    ++n_valid;
  }
  if (h == 0) rel[j] = (valid && vmax != vmin) ? (vj - vmin) / (vmax - vmin) : 0.f;
  __syncthreads();
  float r = 0.f;  // rel_j <- min(rel_j, rel_{j-1}) over the valid entries up to j
  bool seen_one = false;
  for (int i = 0; i <= j && i < N; ++i) {
    if (!okf[i]) continue;
    const float x = rel[i];
    r = (!seen_one || x < r) ? x : r;
    seen_one = true;
  }

  const int n_pick = g.k < n_valid ? g.k : n_valid;
  const float ar = g.a * r;
  bool taken = !valid;
  float pen = -INFINITY;
  int s = first;  // pick 0: the first valid position
  for (int t = 0; t < n_pick; ++t) {
    if (tid == 0) picks[t] = s;
    if (t + 1 == n_pick) break;
    if (j == s) {
      taken = true;
      mr_publish_row<Dp, L>(rowbuf, row, h);
    }
    __syncthreads();
    const float sim = mr_sim<Dp, L>(rowbuf, row, h);
    pen = sim > pen ? sim : pen;
    const float m = ar - g.b * pen;
    const uint64_t key = mr_wave_max(taken ? 0 : mr_key(m, j));
    if ((tid & 63) == 0) part[tid >> 6] = key;
    __syncthreads();
    uint64_t best = part[0];
#pragma unroll
    for (int i = 1; i < WAVES; ++i) best = part[i] > best ? part[i] : best;
    // best != 0: t + 1 < n_pick <= n_valid leaves an unselected valid entry; the mask keeps s a position regardless
    s = (MR_NMAX - (int)(uint32_t)(best & 0xFFFFFFFFu)) & (MR_NMAX - 1);
  }
  __syncthreads();

  const int64_t out = (int64_t)blockIdx.x * g.k;
  for (int t = tid; t < g.k; t += THREADS) {
    const int p = t < n_pick ? picks[t] : -1;
    g.ids_out[out + t] = p >= 0 ? g.pool_ids[base + p] : -1;
    g.scores_out[out + t] = p >= 0 ? v[p] : -INFINITY;
    if (g.pos_out) g.pos_out[out + t] = p;
  }
}

// ------------------------------------------------------------------------------------------------ intra-list diversity
struct IldArgs {
  const float* X;
  int64_t n_items;
  const int64_t* ids;  // (n_q, k)
  int k;
  double* out;  // (n_q)
};

template <int Dp, int L>
__global__ __launch_bounds__(MR_NMAX * L) void list_ild_kernel(const IldArgs g) {
  __shared__ __attribute__((aligned(16))) float rowbuf[2][Dp];
  __shared__ int okf[MR_NMAX];
  __shared__ double sums[MR_NMAX];

  const int tid = threadIdx.x, j = tid / L, h = tid % L;
  const int k = g.k;
  const int64_t id = j < k ? g.ids[(int64_t)blockIdx.x * k + j] : -1;
  const bool valid = (uint64_t)id < (uint64_t)g.n_items;
  if (h == 0) okf[j] = valid ? 1 : 0;
  float4 row[Dp / (4 * L)];
  mr_gather_row<Dp, L>(g.X, id, valid, h, row);
  __syncthreads();

  double acc = 0.0;  // sum over the valid entries s < j of 1 - sim(j, s), in ascending s
  int nb = 0;        // rows published so far: the two buffers alternate, so one barrier per row orders them
  for (int s = 0; s + 1 < k; ++s) {
    if (!okf[s]) continue;
    float* buf = rowbuf[nb & 1];
    ++nb;
    if (j == s) mr_publish_row<Dp, L>(buf, row, h);
    __syncthreads();
    const float sim = mr_sim<Dp, L>(buf, row, h);
    if (valid && j > s) acc += 1.0 - (double)sim;
  }
  if (h == 0) sums[j] = acc;
  __syncthreads();
  if (tid == 0) {
    int64_t nv = 0;
    double total = 0.0;
    for (int i = 0; i < k; ++i) {
      nv += okf[i];
      total += sums[i];
    }
    g.out[blockIdx.x] = nv >= 2 ? total / (double)(nv * (nv - 1) / 2) : 0.0;
  }
}

// ------------------------------------------------------------------------------------------------ launchers
// f(Dp, L as integral_constants) for the padded row length of mr_dp()
template <class F>
static void mr_for_dp(int Dp, F f) {
  using two = std::integral_constant<int, 2>;
  switch (Dp) {
    case 16: f(std::integral_constant<int, 16>{}, two{}); break;
    case 32: f(std::integral_constant<int, 32>{}, two{}); break;
    case 64: f(std::integral_constant<int, 64>{}, two{}); break;
    case 128: f(std::integral_constant<int, 128>{}, two{}); break;
    default: f(std::integral_constant<int, 256>{}, std::integral_constant<int, 4>{}); break;
  }
}

// What both entry points check alike: the list count and length, and the folded buffer.
static int mr_check(const char* who, const void* fold_dev, int64_t fold_bytes, int64_t n_items, int D, int64_t n_q,
                    int k) {
  TRS_REQUIRE(n_q >= 0 && n_q < ((int64_t)1 << 31), "%s: n_q=%lld outside 0..2^31-1", who, (long long)n_q);
  TRS_REQUIRE(k >= 1 && k <= TRS_RETRIEVE_KMAX, "%s: k=%d outside 1..%d", who, k, TRS_RETRIEVE_KMAX);
  TRS_REQUIRE(D >= 1 && D <= TRS_RETRIEVE_DMAX, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(n_items >= 1, "%s: n_items=%lld < 1", who, (long long)n_items);
  const int64_t need = trs_item_fold_bytes(n_items, D);
  TRS_REQUIRE(fold_bytes == need, "%s: fold_bytes=%lld is not trs_item_fold_bytes(n_items, D)=%lld", who,
              (long long)fold_bytes, (long long)need);
  TRS_REQUIRE(fold_dev || n_q == 0, "%s: fold buffer is NULL", who);
  return TRS_OK;
}

}  // namespace

extern "C" int trs_mmr_rerank(const void* nfold_dev, int64_t fold_bytes, int64_t n_items, int32_t D,
                              const int64_t* pool_ids_dev, const float* pool_scores_dev, int64_t n_q, int32_t N,
                              int32_t k, float lambda, int64_t* ids_out_dev, float* scores_out_dev,
                              int32_t* pos_out_dev, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_mmr_rerank";
  TRS_REQUIRE(N >= 1 && N <= TRS_RETRIEVE_KMAX, "%s: N=%d outside 1..%d", who, N, TRS_RETRIEVE_KMAX);
  TRS_TRY(mr_check(who, nfold_dev, fold_bytes, n_items, D, n_q, k));
  TRS_REQUIRE(k <= N, "%s: k=%d > N=%d", who, k, N);
  TRS_REQUIRE(lambda >= 0.f && lambda <= 1.f, "%s: lambda must be a number in [0, 1]", who);  // (a NaN fails both)
  if (n_q == 0) return TRS_OK;
  TRS_REQUIRE(pool_ids_dev && pool_scores_dev && ids_out_dev && scores_out_dev,
              "%s: pool_ids/pool_scores/ids_out/scores_out is NULL", who);
  MmrArgs g = {};
  g.X = (const float*)nfold_dev;
  g.n_items = n_items;
  g.pool_ids = pool_ids_dev;
  g.pool_scores = pool_scores_dev;
  g.N = N;
  g.k = k;
  g.a = 1.0f - lambda;
  g.b = lambda;
  g.ids_out = ids_out_dev;
  g.scores_out = scores_out_dev;
  g.pos_out = pos_out_dev;
  g.err = err_flag_dev;
  mr_for_dp(mr_dp(D), [&](auto dp, auto l) {
    constexpr int Dp = decltype(dp)::value, L = decltype(l)::value;
    hipLaunchKernelGGL((mmr_rerank_kernel<Dp, L>), dim3((unsigned)n_q), dim3(MR_NMAX * L), 0, (hipStream_t)stream, g);
  });
  TRS_CHECK_LAUNCH("mmr_rerank_kernel");
  return TRS_OK;
}

extern "C" int trs_list_ild(const void* nfold_dev, int64_t fold_bytes, int64_t n_items, int32_t D,
                            const int64_t* ids_dev, int64_t n_q, int32_t k, double* ild_out_dev, void* stream) {
  const char* who = "trs_list_ild";
  TRS_TRY(mr_check(who, nfold_dev, fold_bytes, n_items, D, n_q, k));
  if (n_q == 0) return TRS_OK;
  TRS_REQUIRE(ids_dev && ild_out_dev, "%s: ids/ild_out is NULL", who);
  IldArgs g = {};
  g.X = (const float*)nfold_dev;
  g.n_items = n_items;
  g.ids = ids_dev;
  g.k = k;
  g.out = ild_out_dev;
  mr_for_dp(mr_dp(D), [&](auto dp, auto l) {
    constexpr int Dp = decltype(dp)::value, L = decltype(l)::value;
    hipLaunchKernelGGL((list_ild_kernel<Dp, L>), dim3((unsigned)n_q), dim3(MR_NMAX * L), 0, (hipStream_t)stream, g);
  });
  TRS_CHECK_LAUNCH("list_ild_kernel");
  return TRS_OK;
}
