// retrieve.hip — batched top-k retrieval over the whole catalogue with seen-item masking and ranking metrics
// (model.py recommend / evaluate_ranking; math in include/trs.h "retrieval", design in DESIGN.md "Retrieval").
//
// item_fold_kernel      S (n_items_pad, Dp) = item + sum of metadata rows, c (n_items_pad) = per-item constant.
// the tile loop         one workgroup = 32 query rows x one split of the item tiles; its pieces are written once ("the
//                       tile loop" below) and two kernels run it, each with its own epilogue.  The queries' user rows
//                       sit in registers as the A operand of v_mfma_f32_32x32x2_f32; each of the 4 waves multiplies
//                       them with 32 items of a 128-item tile (B read straight from S, 16 bytes per lane).  Per score:
//                       + user and item constants, the seen bit of the tile's LDS bitmask (filled by walking the users'
//                       sorted seen CSR segments alongside the tiles), the key.
// retrieve_topk_kernel  the tile loop with the top-k epilogue: a compare with the user's running k-th best key and an
//                       append of the survivors to the user's LDS candidate buffer (RT_CAP keys).  A buffer that could
//                       overflow in the next tile is compacted first: bitonic sort in LDS, keep k, raise the threshold.
//                       Each workgroup writes its users' sorted top-k keys of its split to the workspace.
// retrieve_merge_kernel joins the splits (bitonic in LDS), writes ids / scores and, given a relevance CSR, metrics.
// mask_seen_kernel      generic path (MLP, k > KMAX): seen entries of score rows -> -inf.
// neighbour_fold_kernel rows of a table (an item fold's S block, the user table) -> a buffer in the item fold's layout:
//                       the rows, optionally scaled to unit length, zero-padded, then a block of zero constants.
//                       trs_neighbours_topk runs retrieve_topk_kernel<NQ, true> over it: the query rows are rows of
//                       the buffer itself and each query's own row is the one excluded id (similar_items / _users).
// rank_metrics_kernel   generic path: metrics of given top-k ids.
// rank_values_kernel    exact ranks (rank_items / evaluate_ranks): key(u, t) of every (query, target) pair by the tile
//                       loop's MFMA step over gathered rows (bit-identical values).
// rank_count_kernel     the tile loop over rows of one (query, target) pair each with `count += key > target key` as
//                       its epilogue; the item splits add their counts to the ranks by 64-bit integer atomics.
//
// The MFMA is an exact fp32 FMA chain (gemm.hip:1-3); the dimension order of the dot product differs from the scoring
// kernels', so on arbitrary weights the scores agree with predict() to rounding, and exactly where all products and
// partial sums are representable (tests/test_ranking.py).
#include "score_kernels.h"

namespace {

constexpr int RT_UT = 32;                  // query users per workgroup: one 32-row MFMA block
constexpr int RT_WAVES = 4;
constexpr int RT_TN = RT_WAVES * 32;       // items per tile
constexpr int RT_CAP = 256;                // candidate keys per user: KMAX + one tile of survivors
constexpr int RT_SPLIT_TARGET = 512;       // workgroups wanted (2 per CU) when the user tiles alone are fewer
constexpr int RT_MERGE_MAX = 4096;         // splits * k keys merged in LDS per user
static_assert(TRS_RETRIEVE_KMAX + RT_TN <= RT_CAP, "a tile's survivors must fit behind k kept keys");

using f32x16 = __attribute__((ext_vector_type(16))) float;

static inline int rt_dp(int D) {
  if (D < 1 || D > TRS_RETRIEVE_DMAX) return 0;
  int p = 16;
  while (p < D) p <<= 1;
  return p;
}
static inline int64_t rt_items_pad(int64_t n) { return (n + RT_TN - 1) / RT_TN * RT_TN; }
static inline int64_t rt_user_tiles(int64_t n_q) { return (n_q + RT_UT - 1) / RT_UT; }
static inline int64_t rt_splits(int64_t n_q, int64_t n_items, int k) {
  int64_t s = (RT_SPLIT_TARGET + rt_user_tiles(n_q) - 1) / rt_user_tiles(n_q);
  const int64_t tiles = rt_items_pad(n_items) / RT_TN;
  if (s > tiles) s = tiles;
  if (s > RT_MERGE_MAX / k) s = RT_MERGE_MAX / k;
  return s < 1 ? 1 : s;
}

// ------------------------------------------------------------------------------------------------ fold
// One wave per item row: lanes over the Dp columns.
__global__ __launch_bounds__(TRS_BLOCK) void item_fold_kernel(int net, const trs_tables T, const int32_t* item_meta,
                                                             int Dp, int64_t n_pad, float* __restrict__ S,
                                                             float* __restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6; i < n_pad; i += nwave) {
    const bool real = i < T.n_items;
    float part = 0.f;  // FM: sum_d (S_d^2 - item_d^2 - sum_m meta_md^2)
    float lin = 0.f;
    for (int d = lane; d < Dp; d += 64) {
      float s = 0.f, sq = 0.f;
      if (real && d < T.D) {
        const float v = T.item[i * T.D + d];
        s = v;
        sq = v * v;
        for (int m = 0; m < T.M; ++m) {
          const int64_t mid = item_meta[i * T.M + m];
          if ((uint64_t)mid >= (uint64_t)T.n_meta[m]) continue;  // (ids were range-checked at ingest)
          const float x = T.meta[m][mid * T.D + d];
          s += x;
          sq += x * x;
        }
      }
      S[i * Dp + d] = s;
      part += s * s - sq;
    }
    if (net == TRS_NET_FM) part = trs_wave_sum(part);
    if (lane == 0) {
      if (real) {
        lin = T.item_lin[i];
        if (net == TRS_NET_FM) {
          for (int m = 0; m < T.M; ++m) {
            const int64_t mid = item_meta[i * T.M + m];
            if ((uint64_t)mid < (uint64_t)T.n_meta[m]) lin += T.meta_lin[m][mid];
          }
          lin += 0.5f * part;
        }
      }
      c[i] = lin;
    }
  }
}

// One wave per row, one pass: lane l holds columns 4l .. 4l+3 (Dp <= 256: one float4 per lane) between the load, the
// norm and the store.  Inverse norm, restated in tests/neighbours_ref.py: per lane the squares summed in ascending d
// (from 0.f, products and sums rounded separately), trs_wave_sum over the 64 lanes, 1.0f / sqrtf; 0 for a zero row.
__global__ __launch_bounds__(TRS_BLOCK) void neighbour_fold_kernel(const float* __restrict__ rows, int64_t n_rows, int D,
                                                                  int64_t ld, int cosine, int Dp, int64_t n_pad,
                                                                  float* __restrict__ X, float* __restrict__ c) {
  const int lane = threadIdx.x & 63;
  const int d0 = 4 * lane;
  const bool vec = (ld & 3) == 0 && (reinterpret_cast<uintptr_t>(rows) & 15) == 0;  // rows start on 16 bytes
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  for (int64_t i = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6; i < n_pad; i += nwave) {
    float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
    if (i < n_rows && d0 < D) {
      const float* r = rows + i * ld + d0;
      if (vec && d0 + 4 <= D) {
        v = *reinterpret_cast<const float4*>(r);
      } else {
        v.x = r[0];
        if (d0 + 1 < D) v.y = r[1];
        if (d0 + 2 < D) v.z = r[2];
        if (d0 + 3 < D) v.w = r[3];
      }
    }
    if (cosine) {
      float sq = 0.f;
      sq += v.x * v.x;
      sq += v.y * v.y;
      sq += v.z * v.z;
      sq += v.w * v.w;
      sq = trs_wave_sum(sq);
      const float inv = sq > 0.f ? 1.0f / sqrtf(sq) : 0.f;
      v.x *= inv;
      v.y *= inv;
      v.z *= inv;
      v.w *= inv;
    }
    if (d0 < Dp) *reinterpret_cast<float4*>(X + i * Dp + d0) = v;
    if (lane == 0) c[i] = 0.f;
  }
}

// ------------------------------------------------------------------------------------------------ the tile loop
// What retrieve_topk_kernel and rank_count_kernel share, each piece written once.  Lane coordinates throughout:
// w = wave of the workgroup, col = lane & 31, h = lane >> 5.

// The catalogue and the query side: what the tile loop reads.
struct TileArgs {
  const float* S;
  const float* c;
  const float* user;
  const float* user_lin;
  int64_t n_users, n_items, n_tiles, tiles_per_split;
  int D;
  int k;  // top-k only; here and not in RetrieveArgs: behind `seen` it costs retrieve_topk_kernel<4 / 8, false> a VGPR
  const int64_t* users;
  int64_t n_q;
  trs_csr seen;  // off == NULL: no masking
};

// the item tiles [t0, t1) of split blockIdx.y
__device__ __forceinline__ void rt_split_bounds(const TileArgs& a, int64_t& t0, int64_t& t1) {
  t0 = (int64_t)blockIdx.y * a.tiles_per_split;
  t1 = t0 + a.tiles_per_split < a.n_tiles ? t0 + a.tiles_per_split : a.n_tiles;
}

// dense user of query q; -1 behind the last query
__device__ __forceinline__ int64_t rt_query_user(const TileArgs& a, int64_t q) { return q < a.n_q ? a.users[q] : -1; }

// Start of the seen walk of dense user u (-1: none) in a split whose first tile is t0: positions [p, e) of seen.items,
// p at the first seen item >= the split's first item.  SELF: the "seen" row of u is the single id u itself (neighbour
// search: users and items are the same rows); the positions are the ids and a.seen is not read.
template <bool SELF>
__device__ __forceinline__ void rt_seen_init(const TileArgs& a, int64_t u, int64_t t0, int64_t& p, int64_t& e) {
  int64_t lo = 0, hi = 0;
  if (SELF) {
    if ((uint64_t)u < (uint64_t)a.n_users) {  // rt_seen_tile skips it in a split that starts behind it
      lo = u;
      hi = u + 1;
    }
  } else if (a.seen.off && (uint64_t)u < (uint64_t)a.seen.n_rows) {
    hi = a.seen.off[u + 1];
    int64_t l = a.seen.off[u], r = hi;
    const int64_t first = t0 * RT_TN;
    while (l < r) {
      const int64_t m = (l + r) >> 1;
      if (a.seen.items[m] < first) l = m + 1; else r = m;
    }
    lo = l;
  }
  p = lo;
  e = hi;
}

// One query row's seen bits of the tile of items [base, base + RT_TN) -> wb[RT_WAVES] (a word per wave's 32 items); the
// walk position p moves to the first seen item behind the tile.
template <bool SELF>
__device__ __forceinline__ void rt_seen_tile(const TileArgs& a, int64_t base, uint32_t* wb, int64_t& pos, int64_t e) {
#pragma unroll
  for (int j = 0; j < RT_WAVES; ++j) wb[j] = 0;
  int64_t p = pos;
  while (p < e) {
    const int64_t it = SELF ? p : (int64_t)a.seen.items[p];
    if (it >= base + RT_TN) break;
    if (it >= base) wb[(it - base) >> 5] |= 1u << ((it - base) & 31);
    ++p;
  }
  pos = p;
}

// A operand of float4 step qq: the lane holds U[col][8*qq + 4*h + cc], cc = 0..3, of `row` (the MFMA's k index is
// lane >> 5 of each step); 0 from column D on and for a row that is not `ok`.
__device__ __forceinline__ void rt_load_a(const float* row, bool ok, int D, int qq, int h, float (&av)[4]) {
#pragma unroll
  for (int cc = 0; cc < 4; ++cc) {
    const int d = 8 * qq + 4 * h + cc;
    av[cc] = (ok && d < D) ? row[d] : 0.f;
  }
}

// One float4 step of the product: 8 columns of 32 rows of A against the lane's B row at sb (+ 4 * h already applied).
__device__ __forceinline__ f32x16 rt_mfma_step(f32x16 acc, const float (&av)[4], const float* sb) {
  const float4 b = *reinterpret_cast<const float4*>(sb);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[0], b.x, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[1], b.y, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[2], b.z, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x2f32(av[3], b.w, acc, 0, 0, 0);
  return acc;
}

// A operand of dense user u (-1, or outside the table: a zero row): NQ float4 steps in registers
template <int NQ>
__device__ __forceinline__ void rt_load_a_row(const TileArgs& a, int64_t u, int h, float (&av)[NQ][4]) {
  const bool ok = (uint64_t)u < (uint64_t)a.n_users;
  const float* row = a.user + (ok ? u : 0) * (int64_t)a.D;
#pragma unroll
  for (int qq = 0; qq < NQ; ++qq) rt_load_a(row, ok, a.D, qq, h, av[qq]);
}

// query row of the lane's accumulator register r (gemm.hip epilogue map)
__device__ __forceinline__ int rt_acc_row(int r, int h) { return (r & 3) + 8 * (r >> 2) + 4 * h; }

// The tile product for this wave's item `item`: 32 query rows x 32 items from a zeroed accumulator.
template <int NQ>
__device__ __forceinline__ f32x16 rt_tile_product(const TileArgs& a, const float (&av)[NQ][4], int64_t item, int h) {
  const float* sb = a.S + item * (8 * NQ) + 4 * h;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
#pragma unroll
  for (int qq = 0; qq < NQ; ++qq) acc = rt_mfma_step(acc, av[qq], sb + 8 * qq);
  return acc;
}

// Head of the epilogue for the accumulator value of register r, query row ur: s = (acc + user const) + ci and the
// item's key; 0 for a padding item (in_range false), a seen one (the row's bit of the tile's mask) or a row without
// bit r of `live`.  rank_count_kernel calls it; retrieve_topk_kernel spells the same three lines out (see there).
__device__ __forceinline__ uint64_t rt_tile_key(float acc, float ucon, float ci, bool in_range, uint32_t live, int r,
                                                const uint32_t* seenb, int ur, int w, int col, int64_t item) {
  const bool seen = (seenb[ur * RT_WAVES + w] >> col) & 1u;
  const float s = (acc + ucon) + ci;
  return (in_range && !seen && ((live >> r) & 1u)) ? trs_topk_key(s, (uint32_t)item) : 0;
}

// one compare-exchange of a descending bitonic network over b[]: pair j of the pass (size, stride)
__device__ __forceinline__ void rt_bitonic_step(uint64_t* b, int j, int size, int stride) {
  const int lo = 2 * j - (j & (stride - 1));
  const int hi = lo + stride;
  const bool desc = (lo & size) == 0;
  const uint64_t x = b[lo], y = b[hi];
  if ((x < y) == desc) {
    b[lo] = y;
    b[hi] = x;
  }
}

// ------------------------------------------------------------------------------------------------ fused top-k
struct RetrieveArgs : TileArgs {
  uint64_t* part;  // (splits, n_q, k) keys, descending
};

// Sort (descending) the candidate buffers of the users whose count exceeds `lim`, keep their first k keys and raise
// their thresholds to the k-th key once k candidates were seen.  Called by the whole workgroup between barriers.
__device__ void rt_compact(uint64_t* cand, uint64_t* th, int* cnt, int* flagged, int* nflag, int k, int lim) {
  const int tid = threadIdx.x;
  if (tid == 0) {
    int n = 0;
    for (int u = 0; u < RT_UT; ++u)
      if (cnt[u] > lim) flagged[n++] = u;
    *nflag = n;
  }
  __syncthreads();
  const int nf = *nflag;
  if (nf == 0) return;
  for (int size = 2; size <= RT_CAP; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      for (int i = tid; i < nf * (RT_CAP / 2); i += TRS_BLOCK)
        rt_bitonic_step(cand + flagged[i / (RT_CAP / 2)] * RT_CAP, i % (RT_CAP / 2), size, stride);
      __syncthreads();
    }
  }
  for (int i = tid; i < nf * RT_CAP; i += TRS_BLOCK) {
    const int f = i / RT_CAP, j = i % RT_CAP;
    if (j >= k) cand[flagged[f] * RT_CAP + j] = 0;
  }
  if (tid < nf) {
    const int u = flagged[tid];
    if (cnt[u] >= k) th[u] = cand[u * RT_CAP + k - 1];
    if (cnt[u] > k) cnt[u] = k;
  }
  __syncthreads();
}

// The tile loop with the top-k epilogue.  SELF: rt_seen_init; the <NQ, false> instances are the kernels of recommend()
// / evaluate_ranking().
template <int NQ, bool SELF>  // Dp = 8 * NQ
__global__ __launch_bounds__(TRS_BLOCK, 2) void retrieve_topk_kernel(const RetrieveArgs a) {
  __shared__ uint64_t cand[RT_UT * RT_CAP];
  __shared__ uint64_t th[RT_UT];
  __shared__ int cnt[RT_UT];
  __shared__ uint32_t seenb[RT_UT * RT_WAVES];
  __shared__ int64_t seen_p[RT_UT], seen_e[RT_UT];
  __shared__ int flagged[RT_UT];
  __shared__ int nflag;

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 31, h = lane >> 5;
  const int64_t q0 = (int64_t)blockIdx.x * RT_UT;
  int64_t t0, t1;
  rt_split_bounds(a, t0, t1);

  for (int i = tid; i < RT_UT * RT_CAP; i += TRS_BLOCK) cand[i] = 0;
  for (int i = tid; i < RT_UT * RT_WAVES; i += TRS_BLOCK) seenb[i] = 0;
  if (tid < RT_UT) {
    th[tid] = 0;
    cnt[tid] = 0;
    rt_seen_init<SELF>(a, rt_query_user(a, q0 + tid), t0, seen_p[tid], seen_e[tid]);
  }

  float av[NQ][4];
  rt_load_a_row<NQ>(a, rt_query_user(a, q0 + col), h, av);
  // user constants of this lane's 16 accumulator rows; `live`: the rows that hold a user of the table
  float ucon[16];
  uint32_t live = 0;
#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int64_t u = rt_query_user(a, q0 + rt_acc_row(r, h));
    const bool ok = (uint64_t)u < (uint64_t)a.n_users;
    ucon[r] = ok ? a.user_lin[u] : 0.f;
    live |= (ok ? 1u : 0u) << r;
  }

  for (int64_t t = t0; t < t1; ++t) {
    __syncthreads();  // the previous tile's appends are done
    rt_compact(cand, th, cnt, flagged, &nflag, a.k, RT_CAP - RT_TN);
    if (tid < RT_UT && (SELF || a.seen.off))
      rt_seen_tile<SELF>(a, t * RT_TN, seenb + tid * RT_WAVES, seen_p[tid], seen_e[tid]);
    __syncthreads();
    const int64_t item = t * RT_TN + w * 32 + col;
    const f32x16 acc = rt_tile_product<NQ>(a, av, item, h);
    const float ci = a.c[item];
    const bool in_range = item < a.n_items;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ur = rt_acc_row(r, h);
      // rt_tile_key, inline: through the function retrieve_topk_kernel<8, *> ran 0.2 - 1.0 % slower
      const bool seen = (seenb[ur * RT_WAVES + w] >> col) & 1u;
      const float s = (acc[r] + ucon[r]) + ci;
      const uint64_t key = (in_range && !seen && ((live >> r) & 1u)) ? trs_topk_key(s, (uint32_t)item) : 0;
      if (key > th[ur]) {
        const int p = atomicAdd(&cnt[ur], 1);
        cand[ur * RT_CAP + p] = key;
      }
    }
  }
  __syncthreads();
  rt_compact(cand, th, cnt, flagged, &nflag, a.k, 0);
  uint64_t* out = a.part + (int64_t)blockIdx.y * a.n_q * a.k;
  for (int i = tid; i < RT_UT * a.k; i += TRS_BLOCK) {
    const int u = i / a.k, j = i % a.k;
    const int64_t q = q0 + u;
    if (q < a.n_q) out[q * a.k + j] = cand[u * RT_CAP + j];
  }
}

// ------------------------------------------------------------------------------------------------ metrics
// (hits, dcg, idcg, n_rel) of the list ids[0..k) (dense ids, -1 = none) against rel row u, in ascending r.
__device__ void rt_metrics(const int64_t* ids, int k, int64_t u, const trs_csr rel, double* out) {
  int64_t lo = 0, hi = 0;
  if ((uint64_t)u < (uint64_t)rel.n_rows) {
    lo = rel.off[u];
    hi = rel.off[u + 1];
  }
  double hits = 0.0, dcg = 0.0, idcg = 0.0;
  for (int r = 0; r < k; ++r) {
    const int64_t id = ids[r];
    bool hit = false;
    if (id >= 0) {
      int64_t l = lo, rr = hi;
      while (l < rr) {
        const int64_t m = (l + rr) >> 1;
        const int64_t v = rel.items[m];
        if (v == id) {
          hit = true;
          break;
        }
        if (v < id) l = m + 1; else rr = m;
      }
    }
    const double g = 1.0 / log2((double)(r + 2));
    if (hit) {
      hits += 1.0;
      dcg += g;
    }
    if (r < hi - lo) idcg += g;
  }
  out[0] = hits;
  out[1] = dcg;
  out[2] = idcg;
  out[3] = (double)(hi - lo);
}

struct MergeArgs {
  const uint64_t* part;
  int64_t n_q, splits;
  int k, fm;
  const int64_t* users;
  trs_csr rel;  // off == NULL: no metrics
  int64_t* ids;
  float* scores;
  double* metrics;
};

// One workgroup per query user (grid-stride): the splits' k keys each -> the best k.
__global__ __launch_bounds__(TRS_BLOCK) void retrieve_merge_kernel(const MergeArgs m) {
  __shared__ uint64_t s[RT_MERGE_MAX];
  __shared__ int64_t ids[TRS_RETRIEVE_KMAX];
  const int tid = threadIdx.x;
  const int n = (int)(m.splits * m.k);
  int P = 1;
  while (P < n) P <<= 1;
  for (int64_t q = blockIdx.x; q < m.n_q; q += gridDim.x) {
    __syncthreads();
    for (int i = tid; i < P; i += TRS_BLOCK) {
      uint64_t key = 0;
      if (i < n) key = m.part[((int64_t)(i / m.k) * m.n_q + q) * m.k + i % m.k];
      s[i] = key;
    }
    __syncthreads();
    if (m.splits > 1) {
      for (int size = 2; size <= P; size <<= 1) {
        for (int stride = size >> 1; stride > 0; stride >>= 1) {
          for (int i = tid; i < P / 2; i += TRS_BLOCK) rt_bitonic_step(s, i, size, stride);
          __syncthreads();
        }
      }
    }
    for (int j = tid; j < m.k; j += TRS_BLOCK) {
      const uint64_t key = s[j];
      int64_t id = -1;
      float sc = -INFINITY;
      if (key != 0) {
        id = (int64_t)(0xFFFFFFFFu - (uint32_t)(key & 0xFFFFFFFFu));
        sc = trs_topk_key_score(key);
        if (m.fm) sc = trs::sigmoidf_(sc);
      }
      ids[j] = id;
      m.ids[q * m.k + j] = id;
      m.scores[q * m.k + j] = sc;
    }
    __syncthreads();
    if (m.rel.off && tid == 0) rt_metrics(ids, m.k, m.users[q], m.rel, m.metrics + q * 4);
  }
}

__global__ __launch_bounds__(TRS_BLOCK) void rank_metrics_kernel(const int64_t* ids, int64_t n_q, int k,
                                                                const int64_t* users, const trs_csr rel,
                                                                double* out) {
  const int64_t stride = (int64_t)gridDim.x * TRS_BLOCK;
  for (int64_t q = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x; q < n_q; q += stride)
    rt_metrics(ids + q * k, k, users[q], rel, out + q * 4);
}

// One workgroup per score row (grid-stride): the user's seen items -> -inf.
__global__ __launch_bounds__(TRS_BLOCK) void mask_seen_kernel(float* scores, int64_t n_rows, int64_t n_items,
                                                             const int64_t* users, const trs_csr seen) {
  for (int64_t r = blockIdx.x; r < n_rows; r += gridDim.x) {
    const int64_t u = users[r];
    if ((uint64_t)u >= (uint64_t)seen.n_rows) continue;
    const int64_t lo = seen.off[u], hi = seen.off[u + 1];
    for (int64_t p = lo + threadIdx.x; p < hi; p += TRS_BLOCK) {
      const int64_t it = seen.items[p];
      if ((uint64_t)it < (uint64_t)n_items) scores[r * n_items + it] = -INFINITY;
    }
  }
}

// ------------------------------------------------------------------------------------------------ exact ranks
// rank(u, t) = #{ i in C_u, i != t : key(u, i) > key(u, t) } (include/trs.h "exact ranks").  A query row of the counting
// kernel is one (query, target) pair: row j = entry j of the targets CSR.  (Several targets of a user per row were
// tried and do not fit the registers: profiles/EXPERIMENTS.md.)
constexpr uint64_t RK_NONE = ~(uint64_t)0;  // key of a padding slot or an invalid pair: no key is above it

struct RankArgs : TileArgs {  // (k of the shared block is not used here and stays 0)
  int Dp, fm;
  int64_t n_t;
  trs_csr targets;  // row q: the targets of query q
  uint64_t* tkey;   // (n_t) key(u, t) of every pair
  int64_t* ranks;   // (n_t)
  float* values;    // (n_t) or NULL
};

// first q in [0, n) with a[q + 1] > x: the row of a CSR-like offset array that holds position x
__device__ __forceinline__ int64_t rk_row_of(const int64_t* a, int64_t n, int64_t x) {
  int64_t l = 0, r = n;
  while (l < r) {
    const int64_t m = (l + r) >> 1;
    if (a[m + 1] <= x) l = m + 1; else r = m;
  }
  return l;
}

// key(u, t) of 32 pairs per wave by the tile loop's own MFMA step: row `col` of the A block is the pair's user, column
// `col` of the B block the pair's target, and the diagonal of the 32 x 32 product holds <U_u, S_t> in the very order
// the tile loop accumulates it — the value is bit-identical to the one the counting kernel compares with.
// Also sets ranks[j] to 0 (-1 for a user outside the table or a target outside the catalogue).
__global__ __launch_bounds__(TRS_BLOCK) void rank_values_kernel(const RankArgs a) {
  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 31, h = lane >> 5;
  const int64_t j = ((int64_t)blockIdx.x * RT_WAVES + w) * 32 + col;
  bool ok = false;
  int64_t u = 0, t = 0;
  if (j < a.n_t) {
    const int64_t q = rk_row_of(a.targets.off, a.n_q, j);
    if (q < a.n_q) {
      const int64_t uu = a.users[q], tt = a.targets.items[j];
      ok = (uint64_t)uu < (uint64_t)a.n_users && (uint64_t)tt < (uint64_t)a.n_items;
      if (ok) {
        u = uu;
        t = tt;
      }
    }
  }
  const float* urow = a.user + u * (int64_t)a.D;
  const float* sb = a.S + t * (int64_t)a.Dp + 4 * h;
  f32x16 acc;
#pragma unroll
  for (int r = 0; r < 16; ++r) acc[r] = 0.f;
  for (int qq = 0; qq < a.Dp / 8; ++qq) {  // uniform trip count: every lane takes part in every MFMA
    float av[4];
    rt_load_a(urow, ok, a.D, qq, h, av);
    acc = rt_mfma_step(acc, av, sb + 8 * qq);
  }
  // accumulator row rt_acc_row(r, h) == col sits in the half h = (col >> 2) & 1 at r = (col & 3) + 4 * (col >> 3)
  if (j < a.n_t && h == ((col >> 2) & 1)) {
    const int rr = (col & 3) + 4 * (col >> 3);
    float dot = 0.f;
#pragma unroll
    for (int r = 0; r < 16; ++r)
      if (r == rr) dot = acc[r];
    const float v = (dot + a.user_lin[u]) + a.c[t];
    a.tkey[j] = ok ? trs_topk_key(v, (uint32_t)t) : RK_NONE;
    a.ranks[j] = ok ? 0 : -1;
    if (a.values) a.values[j] = ok ? (a.fm ? trs::sigmoidf_(v) : v) : -INFINITY;
  }
}

// The tile loop with the counting epilogue over 32 (query, target) rows: the keys above each row's target key (read
// from LDS: the lanes of a half wave share a row, so the read is a broadcast) are counted in int32 registers.  No
// candidate buffer and no LDS atomic in the tile loop.  After the last tile the counters are summed over the 32 columns
// and the 4 waves, and each split adds its part to ranks[] with one 64-bit integer atomic per row.
template <int NQ>  // Dp = 8 * NQ
__global__ __launch_bounds__(TRS_BLOCK, 2) void rank_count_kernel(const RankArgs a) {
  __shared__ uint64_t tk[RT_UT];
  __shared__ int64_t row_u[RT_UT];  // the row's dense user; -1: no such row, or a user outside the table
  __shared__ float row_c[RT_UT];    // its user constant
  __shared__ uint32_t seenb[RT_UT * RT_WAVES];
  __shared__ int64_t seen_p[RT_UT], seen_e[RT_UT];
  __shared__ int part[RT_WAVES][RT_UT];

  const int tid = threadIdx.x, lane = tid & 63, w = tid >> 6, col = lane & 31, h = lane >> 5;
  const int64_t r0 = (int64_t)blockIdx.x * RT_UT;
  int64_t t0, t1;
  rt_split_bounds(a, t0, t1);

  for (int i = tid; i < RT_UT * RT_WAVES; i += TRS_BLOCK) seenb[i] = 0;
  if (tid < RT_UT) {
    const int64_t j = r0 + tid;
    int64_t u = -1;
    if (j < a.n_t) {
      const int64_t q = rk_row_of(a.targets.off, a.n_q, j);
      if (q < a.n_q && a.targets.off[q + 1] > j) {  // (offsets that do not ascend: nothing is read or written)
        const int64_t uu = a.users[q];
        if ((uint64_t)uu < (uint64_t)a.n_users) u = uu;
      }
    }
    tk[tid] = u >= 0 ? a.tkey[j] : RK_NONE;
    row_u[tid] = u;
    row_c[tid] = u >= 0 ? a.user_lin[u] : 0.f;
    rt_seen_init<false>(a, u, t0, seen_p[tid], seen_e[tid]);
  }
  __syncthreads();

  float av[NQ][4];
  rt_load_a_row<NQ>(a, row_u[col], h, av);
  // The user constants stay in LDS beside the target keys (16 more registers do not fit next to av[32][4] and the
  // counters at D = 256).  A row without a live user holds an RK_NONE key: nothing is counted, so it needs no live bit.
  int cnt[16];
#pragma unroll
  for (int r = 0; r < 16; ++r) cnt[r] = 0;

  for (int64_t t = t0; t < t1; ++t) {
    if (a.seen.off) {
      __syncthreads();  // the previous tile's reads of seenb are done
      if (tid < RT_UT) rt_seen_tile<false>(a, t * RT_TN, seenb + tid * RT_WAVES, seen_p[tid], seen_e[tid]);
      __syncthreads();
    }
    const int64_t item = t * RT_TN + w * 32 + col;
    const f32x16 acc = rt_tile_product<NQ>(a, av, item, h);
    const float ci = a.c[item];
    const bool in_range = item < a.n_items;
#pragma unroll
    for (int r = 0; r < 16; ++r) {
      const int ur = rt_acc_row(r, h);
      // every row is live (a row without a user holds an RK_NONE key); the call, not the three lines: with them inline
      // rank_count_kernel<16> ran 0.4 % slower
      cnt[r] += rt_tile_key(acc[r], row_c[ur], ci, in_range, ~0u, r, seenb, ur, w, col, item) > tk[ur] ? 1 : 0;
    }
  }

#pragma unroll
  for (int r = 0; r < 16; ++r) {
    const int c = trs_group_sum_i<32>(cnt[r]);  // over the 32 columns of this half wave
    if (col == 0) part[w][rt_acc_row(r, h)] = c;
  }
  __syncthreads();
  if (tid < RT_UT) {
    int64_t total = 0;
#pragma unroll
    for (int j = 0; j < RT_WAVES; ++j) total += part[j][tid];
    if (total > 0 && tk[tid] != RK_NONE)
      atomicAdd(reinterpret_cast<unsigned long long*>(a.ranks + r0 + tid), (unsigned long long)total);
  }
}

// ------------------------------------------------------------------------------------------------ launchers
static int check_csr(const trs_csr* c, const char* who, const char* what) {
  TRS_REQUIRE(c->off && c->items && c->n_rows >= 0, "%s: %s CSR has NULL arrays", who, what);
  return TRS_OK;
}

// f(integral_constant<int, NQ>) for the padded row length Dp = 8 * NQ of rt_dp()
template <class F>
static void rt_for_nq(int Dp, F f) {
  switch (Dp) {
    case 16: f(std::integral_constant<int, 2>{}); break;
    case 32: f(std::integral_constant<int, 4>{}); break;
    case 64: f(std::integral_constant<int, 8>{}); break;
    case 128: f(std::integral_constant<int, 16>{}); break;
    default: f(std::integral_constant<int, 32>{}); break;
  }
}

// The tile loop's arguments for a folded buffer of (n_items, D) and a user table of row length D.
static void rt_fill(TileArgs& a, const void* fold_dev, int64_t n_items, int D, const float* user, const float* user_lin,
                    int64_t n_users, const int64_t* users, int64_t n_q, const trs_csr* seen) {
  const int64_t n_pad = rt_items_pad(n_items);
  a.S = (const float*)fold_dev;
  a.c = a.S + n_pad * rt_dp(D);
  a.user = user;
  a.user_lin = user_lin;
  a.n_users = n_users;
  a.n_items = n_items;
  a.n_tiles = n_pad / RT_TN;
  a.D = D;
  a.users = users;
  a.n_q = n_q;
  if (seen) a.seen = *seen;
}

// Spreads the item tiles over `splits` workgroups per query tile; returns the splits that own at least one tile.
static int64_t rt_set_splits(TileArgs& a, int64_t splits) {
  a.tiles_per_split = (a.n_tiles + splits - 1) / splits;
  return (a.n_tiles + a.tiles_per_split - 1) / a.tiles_per_split;
}

// The fused kernel over the query tiles x item splits of `a`, then the merge.
template <bool SELF>
static int run_retrieve(const char* who, RetrieveArgs& a, int Dp, int64_t splits, MergeArgs& m, hipStream_t s) {
  const int64_t used = rt_set_splits(a, splits);
  TRS_REQUIRE(rt_user_tiles(a.n_q) < ((int64_t)1 << 31), "%s: too many query users in one call", who);
  const dim3 grid((unsigned)rt_user_tiles(a.n_q), (unsigned)used);
  rt_for_nq(Dp, [&](auto nq) {
    hipLaunchKernelGGL((retrieve_topk_kernel<decltype(nq)::value, SELF>), grid, dim3(TRS_BLOCK), 0, s, a);
  });
  TRS_CHECK_LAUNCH("retrieve_topk_kernel");
  m.part = a.part;
  m.n_q = a.n_q;
  m.splits = used;
  m.k = a.k;
  const int64_t mg = a.n_q < 65536 ? a.n_q : 65536;
  hipLaunchKernelGGL(retrieve_merge_kernel, dim3((unsigned)mg), dim3(TRS_BLOCK), 0, s, m);
  TRS_CHECK_LAUNCH("retrieve_merge_kernel");
  return TRS_OK;
}

// What trs_retrieve_topk and trs_item_ranks check alike: a Linear / FM scorer with a user table.
static int rt_check_scorer(const char* who, int net, const trs_tables* T) {
  TRS_REQUIRE(T != nullptr, "%s: tables is NULL", who);
  TRS_REQUIRE(net == TRS_NET_LINEAR || net == TRS_NET_FM, "%s: net must be TRS_NET_LINEAR or TRS_NET_FM", who);
  TRS_REQUIRE(T->user && T->user_lin && T->n_users > 0 && T->n_items > 0, "%s: user table is NULL/empty", who);
  return TRS_OK;
}

// What every entry point over a folded buffer checks: the query count and the buffer.
static int rt_check_fold(const char* who, int64_t n_items, int D, int64_t n_q, const void* fold_dev,
                         int64_t fold_bytes) {
  TRS_REQUIRE(n_q >= 0, "%s: negative n_q", who);
  const int64_t fneed = trs_item_fold_bytes(n_items, D);
  TRS_REQUIRE(fneed > 0, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(fold_dev && fold_bytes >= fneed, "%s: fold buffer too small (%lld < %lld)", who, (long long)fold_bytes,
              (long long)fneed);
  return TRS_OK;
}

// What trs_retrieve_topk and trs_neighbours_topk check alike: k, the query count, the folded buffer, the workspace.
static int rt_check_topk(const char* who, int64_t n_items, int D, int k, int64_t n_q, const void* fold_dev,
                         int64_t fold_bytes, const void* workspace_dev, int64_t workspace_bytes) {
  TRS_REQUIRE(k >= 1 && k <= TRS_RETRIEVE_KMAX, "%s: k=%d outside 1..%d (larger k: score rows + trs_topk)", who, k,
              TRS_RETRIEVE_KMAX);
  TRS_REQUIRE(k <= n_items, "%s: k=%d > n_items=%lld", who, k, (long long)n_items);
  TRS_TRY(rt_check_fold(who, n_items, D, n_q, fold_dev, fold_bytes));
  TRS_REQUIRE(workspace_bytes >= trs_retrieve_workspace_bytes(n_q, k) && (workspace_dev || n_q == 0),
              "%s: workspace too small (%lld < %lld)", who, (long long)workspace_bytes,
              (long long)trs_retrieve_workspace_bytes(n_q, k));
  return TRS_OK;
}

}  // namespace

extern "C" int64_t trs_item_fold_bytes(int64_t n_items, int32_t D) {
  const int Dp = rt_dp(D);
  if (n_items <= 0 || Dp == 0) return 0;
  return rt_items_pad(n_items) * (int64_t)(Dp + 1) * 4;
}

extern "C" int trs_item_fold(int net, const trs_tables* T, const int32_t* item_meta_dev, void* fold_dev,
                             int64_t fold_bytes, void* stream) {
  TRS_TRY(trs_check_tables("trs_item_fold", net, T, TRS_SKIP_USER | TRS_SKIP_META_ROWS));  // folds item-side rows only
  TRS_REQUIRE(T->M == 0 || item_meta_dev, "trs_item_fold: item_meta is NULL but M=%d", T->M);
  TRS_TRY(rt_check_fold("trs_item_fold", T->n_items, T->D, 0, fold_dev, fold_bytes));
  const int Dp = rt_dp(T->D);
  const int64_t n_pad = rt_items_pad(T->n_items);
  float* S = (float*)fold_dev;
  hipLaunchKernelGGL(item_fold_kernel, dim3(trs_grid(n_pad, TRS_BLOCK / 64)), dim3(TRS_BLOCK), 0, (hipStream_t)stream,
                     net, *T, item_meta_dev, Dp, n_pad, S, S + n_pad * Dp);
  TRS_CHECK_LAUNCH("item_fold_kernel");
  return TRS_OK;
}

extern "C" int64_t trs_retrieve_workspace_bytes(int64_t n_q, int32_t k) {
  if (n_q <= 0 || k <= 0) return 0;
  // splits <= ceil(TARGET / tiles) -> splits * n_q <= (TARGET + tiles) * RT_UT: a bound monotone in n_q and k
  return (RT_SPLIT_TARGET + rt_user_tiles(n_q)) * (int64_t)RT_UT * k * 8;
}

extern "C" int trs_retrieve_topk(int net, const trs_tables* T, const void* fold_dev, int64_t fold_bytes,
                                 const int64_t* users_dev, int64_t n_q, int32_t k, const trs_csr* seen,
                                 const trs_csr* rel, int64_t* ids_out_dev, float* scores_out_dev,
                                 double* metrics_out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const char* who = "trs_retrieve_topk";
  TRS_TRY(rt_check_scorer(who, net, T));
  TRS_TRY(rt_check_topk(who, T->n_items, T->D, k, n_q, fold_dev, fold_bytes, workspace_dev, workspace_bytes));
  if (seen) TRS_TRY(check_csr(seen, who, "seen"));
  if (rel) TRS_TRY(check_csr(rel, who, "relevance"));
  TRS_REQUIRE(!rel || metrics_out_dev, "%s: a relevance CSR needs metrics_out", who);
  if (n_q == 0) return TRS_OK;
  TRS_REQUIRE(users_dev && ids_out_dev && scores_out_dev, "%s: users/ids_out/scores_out is NULL", who);
  RetrieveArgs a = {};
  rt_fill(a, fold_dev, T->n_items, T->D, T->user, T->user_lin, T->n_users, users_dev, n_q, seen);
  a.k = k;
  a.part = (uint64_t*)workspace_dev;
  MergeArgs m = {};
  m.fm = net == TRS_NET_FM;
  m.users = users_dev;
  if (rel) m.rel = *rel;
  m.ids = ids_out_dev;
  m.scores = scores_out_dev;
  m.metrics = metrics_out_dev;
  return run_retrieve<false>(who, a, rt_dp(T->D), rt_splits(n_q, T->n_items, k), m, (hipStream_t)stream);
}

extern "C" int trs_neighbour_fold(const float* rows_dev, int64_t n_rows, int32_t D, int64_t ld, int32_t cosine,
                                  void* fold_dev, int64_t fold_bytes, void* stream) {
  const char* who = "trs_neighbour_fold";
  TRS_REQUIRE(rows_dev != nullptr, "%s: rows is NULL", who);
  TRS_REQUIRE(n_rows > 0, "%s: n_rows=%lld < 1", who, (long long)n_rows);
  TRS_REQUIRE(rt_dp(D) > 0, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(ld >= D, "%s: ld=%lld < D=%d", who, (long long)ld, D);
  TRS_REQUIRE(cosine == 0 || cosine == 1, "%s: cosine must be 0 or 1", who);
  TRS_TRY(rt_check_fold(who, n_rows, D, 0, fold_dev, fold_bytes));
  const int Dp = rt_dp(D);
  const int64_t n_pad = rt_items_pad(n_rows);
  float* X = (float*)fold_dev;
  hipLaunchKernelGGL(neighbour_fold_kernel, dim3(trs_grid(n_pad, TRS_BLOCK / 64)), dim3(TRS_BLOCK), 0,
                     (hipStream_t)stream, rows_dev, n_rows, (int)D, ld, (int)cosine, Dp, n_pad, X, X + n_pad * Dp);
  TRS_CHECK_LAUNCH("neighbour_fold_kernel");
  return TRS_OK;
}

extern "C" int trs_neighbours_topk(const void* fold_dev, int64_t fold_bytes, int64_t n_rows, int32_t D,
                                   const int64_t* queries_dev, int64_t n_q, int32_t k, int64_t* ids_out_dev,
                                   float* scores_out_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const char* who = "trs_neighbours_topk";
  TRS_REQUIRE(n_rows > 0, "%s: n_rows=%lld < 1", who, (long long)n_rows);
  TRS_TRY(rt_check_topk(who, n_rows, D, k, n_q, fold_dev, fold_bytes, workspace_dev, workspace_bytes));
  if (n_q == 0) return TRS_OK;
  TRS_REQUIRE(queries_dev && ids_out_dev && scores_out_dev, "%s: queries/ids_out/scores_out is NULL", who);
  const int Dp = rt_dp(D);
  RetrieveArgs a = {};
  rt_fill(a, fold_dev, n_rows, D, nullptr, nullptr, n_rows, queries_dev, n_q, nullptr);
  a.user = a.S;      // the catalogue and the query rows are the same padded matrix: the row length is Dp,
  a.D = Dp;
  a.user_lin = a.c;  // and the zero block is every item constant and every query constant (n_rows <= n_pad entries)
  a.k = k;
  a.part = (uint64_t*)workspace_dev;
  MergeArgs m = {};  // fm = 0: raw inner products out
  m.users = queries_dev;
  m.ids = ids_out_dev;
  m.scores = scores_out_dev;
  return run_retrieve<true>(who, a, Dp, rt_splits(n_q, n_rows, k), m, (hipStream_t)stream);
}

extern "C" int trs_mask_seen(float* scores_dev, int64_t n_rows, int64_t n_items, const int64_t* users_dev,
                             const trs_csr* seen, void* stream) {
  TRS_REQUIRE(n_rows >= 0 && n_items > 0, "trs_mask_seen: bad sizes");
  TRS_REQUIRE(seen != nullptr, "trs_mask_seen: seen CSR is NULL");
  TRS_TRY(check_csr(seen, "trs_mask_seen", "seen"));
  if (n_rows == 0) return TRS_OK;
  TRS_REQUIRE(scores_dev && users_dev, "trs_mask_seen: scores/users is NULL");
  hipLaunchKernelGGL(mask_seen_kernel, dim3((unsigned)(n_rows < 65536 ? n_rows : 65536)), dim3(TRS_BLOCK), 0,
                     (hipStream_t)stream, scores_dev, n_rows, n_items, users_dev, *seen);
  TRS_CHECK_LAUNCH("mask_seen_kernel");
  return TRS_OK;
}

extern "C" int trs_rank_metrics(const int64_t* ids_dev, int64_t n_q, int32_t k, const int64_t* users_dev,
                                const trs_csr* rel, double* metrics_out_dev, void* stream) {
  TRS_REQUIRE(k >= 1, "trs_rank_metrics: k=%d < 1", k);
  TRS_REQUIRE(n_q >= 0, "trs_rank_metrics: negative n_q");
  TRS_REQUIRE(rel != nullptr, "trs_rank_metrics: relevance CSR is NULL");
  TRS_TRY(check_csr(rel, "trs_rank_metrics", "relevance"));
  if (n_q == 0) return TRS_OK;
  TRS_REQUIRE(ids_dev && users_dev && metrics_out_dev, "trs_rank_metrics: ids/users/metrics_out is NULL");
  hipLaunchKernelGGL(rank_metrics_kernel, dim3(trs_grid(n_q, TRS_BLOCK)), dim3(TRS_BLOCK), 0, (hipStream_t)stream,
                     ids_dev, n_q, (int)k, users_dev, *rel, metrics_out_dev);
  TRS_CHECK_LAUNCH("rank_metrics_kernel");
  return TRS_OK;
}

// ------------------------------------------------------------------------------------------------ exact ranks (host)
extern "C" int64_t trs_item_ranks_workspace_bytes(int64_t n_q, int64_t n_targets) {
  if (n_q <= 0 || n_targets < 0) return 0;
  return (n_q + 1 + n_targets) * 8;  // n_q + 1 words that are not used (the size is ABI), then a key per target
}

extern "C" int trs_item_ranks(int net, const trs_tables* T, const void* fold_dev, int64_t fold_bytes,
                              const int64_t* users_dev, int64_t n_q, const trs_csr* targets, const trs_csr* seen,
                              int64_t* ranks_out_dev, float* values_out_dev, void* workspace_dev,
                              int64_t workspace_bytes, void* stream) {
  const char* who = "trs_item_ranks";
  hipStream_t s = (hipStream_t)stream;
  TRS_TRY(rt_check_scorer(who, net, T));
  TRS_TRY(rt_check_fold(who, T->n_items, T->D, n_q, fold_dev, fold_bytes));
  TRS_REQUIRE(targets != nullptr, "%s: targets CSR is NULL", who);
  TRS_TRY(check_csr(targets, who, "targets"));
  TRS_REQUIRE(targets->n_rows == n_q, "%s: targets has %lld rows for n_q=%lld queries", who,
              (long long)targets->n_rows, (long long)n_q);
  if (seen) TRS_TRY(check_csr(seen, who, "seen"));
  const int stages = trs_tuning().ranks_stages;
  TRS_REQUIRE(stages >= 1 && stages <= 3, "%s: RANKS_STAGES=%d outside 1..3", who, stages);
  if (n_q == 0) return TRS_OK;
  TRS_REQUIRE(users_dev && ranks_out_dev, "%s: users/ranks_out is NULL", who);
  TRS_REQUIRE(workspace_dev && workspace_bytes >= trs_item_ranks_workspace_bytes(n_q, 0),
              "%s: workspace too small (%lld < %lld before the targets)", who, (long long)workspace_bytes,
              (long long)trs_item_ranks_workspace_bytes(n_q, 0));
  // the number of pairs lives on the device: one 8-byte read-back, the only synchronisation of the call
  int64_t n_t = 0;
  if (hipMemcpyAsync(&n_t, targets->off + n_q, sizeof(n_t), hipMemcpyDeviceToHost, s) != hipSuccess ||
      hipStreamSynchronize(s) != hipSuccess) {
    trs_set_error("%s: reading targets->off[n_q] failed: %s", who, hipGetErrorString(hipGetLastError()));
    return TRS_E_LAUNCH;
  }
  TRS_REQUIRE(n_t >= 0, "%s: targets->off[n_q]=%lld < 0", who, (long long)n_t);
  if (n_t == 0) return TRS_OK;
  TRS_REQUIRE(workspace_bytes >= trs_item_ranks_workspace_bytes(n_q, n_t), "%s: workspace too small (%lld < %lld)", who,
              (long long)workspace_bytes, (long long)trs_item_ranks_workspace_bytes(n_q, n_t));
  RankArgs a = {};
  rt_fill(a, fold_dev, T->n_items, T->D, T->user, T->user_lin, T->n_users, users_dev, n_q, seen);
  a.Dp = rt_dp(T->D);
  a.fm = net == TRS_NET_FM;
  a.n_t = n_t;
  a.targets = *targets;
  a.tkey = (uint64_t*)workspace_dev + (n_q + 1);
  a.ranks = ranks_out_dev;
  a.values = values_out_dev;
  const int64_t vgrid = (n_t + RT_TN - 1) / RT_TN, row_tiles = rt_user_tiles(n_t);
  TRS_REQUIRE(vgrid < ((int64_t)1 << 31), "%s: too many targets in one call", who);
  if (stages & 1) {
    hipLaunchKernelGGL(rank_values_kernel, dim3((unsigned)vgrid), dim3(TRS_BLOCK), 0, s, a);
    TRS_CHECK_LAUNCH("rank_values_kernel");
  }
  if (!(stages & 2)) return TRS_OK;
  int64_t splits = (RT_SPLIT_TARGET + row_tiles - 1) / row_tiles;
  if (splits > a.n_tiles) splits = a.n_tiles;
  const dim3 grid((unsigned)row_tiles, (unsigned)rt_set_splits(a, splits));
  rt_for_nq(a.Dp, [&](auto nq) {
    hipLaunchKernelGGL((rank_count_kernel<decltype(nq)::value>), grid, dim3(TRS_BLOCK), 0, s, a);
  });
  TRS_CHECK_LAUNCH("rank_count_kernel");
  return TRS_OK;
}
