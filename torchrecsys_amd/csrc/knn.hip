// knn.hip — sparse item-kNN: the neighbourhood model of model.py fit_itemknn.  The rule is the contract in
// include/trs.h "item kNN", the design in DESIGN.md 4.20.
//
// knn_build_kernel   a workgroup owns an item i (handed out by a device-side counter: the work per item is heavy-tailed).
//                    The catalogue's columns are cut into tiles of TRS_KNN_TILE ids whose 32-bit co-occurrence counters
//                    live in LDS.  Per tile: every user of i adds 1 to the counter of each of its items inside the tile
//                    (LDS integer atomics: exact in any order); an add that returns 0 appends the column to a touched
//                    list of TRS_KNN_TOUCHED entries.  The candidates are then visited, and their counters reset, from
//                    that list, or by a sweep of the tile when the list overflowed; each becomes a 64-bit key
//                    (trs_topk_key of the fp32 similarity and the id) and, when above the running K-th key, goes into a
//                    buffer in LDS that a bitonic sort cuts back to its K largest whenever it fills.  The keys are
//                    distinct, so the K largest are one set whatever the arrival order; the final sort puts them in key
//                    order and they are written once.
//                    Where the tile segment of a user's sorted list starts: with one tile it is the whole list; an item
//                    with at most one user per thread keeps a cursor per user that only moves forward, eight entries
//                    requested at a time (no search); otherwise two binary searches per (user, tile).
// knn_rows_kernel    out[r] = the score row of a history: a workgroup per (row, tile of KNN_ROW_TILE columns), the tile
//                    in LDS; the history's items in CSR order, the K slots of one item by K lanes (distinct columns: a
//                    plain read-add-write), a barrier between items; the tile is written out coalesced, zeros included.
#include "trs_common.h"

#include <math.h>

namespace {

constexpr int KB_THREADS = 512;  // knn_build_kernel: 8 waves; 2 workgroups per CU by LDS
constexpr int KB_WAVES = KB_THREADS / TRS_WAVE;
constexpr int KB_BUF = 1024;     // candidate keys between two cuts: K <= 128 kept + up to KB_THREADS per round
constexpr int KB_SHORT = 4;      // a tile segment up to this long is walked by its own lane, a longer one by the wave
constexpr int KB_BATCH = 8;      // list entries a cursor requests together
static_assert(KB_BUF >= 2 * KB_THREADS && TRS_KNN_KMAX <= KB_BUF - KB_THREADS, "a round's appends must fit");
static_assert((KB_BUF & (KB_BUF - 1)) == 0, "bitonic sort");
constexpr size_t KB_LDS = (size_t)KB_BUF * 8 + (size_t)TRS_KNN_TILE * 4 + (size_t)TRS_KNN_TOUCHED * 4;

constexpr int KNN_ROW_TILE = 8192;  // columns per workgroup of knn_rows_kernel (32 KiB of LDS)

// the fp32 similarity from the integers: fp64, every operation rounded once, then one rounding to fp32
__device__ __forceinline__ float knn_sim(int kind, double h, uint32_t c, int64_t ni, int64_t nj) {
  const double cd = (double)c;
  double s;
  if (kind == TRS_KNN_COSINE)
    s = cd / (__dsqrt_rn((double)ni * (double)nj) + h);
  else if (kind == TRS_KNN_JACCARD)
    s = cd / ((double)(ni + nj - (int64_t)c) + h);
  else if (kind == TRS_KNN_CONDITIONAL)
    s = cd / ((double)ni + h);
  else
    s = cd;
  return __double2float_rn(s);
}

// first position in [lo, hi) whose id is >= v (the list is sorted)
__device__ __forceinline__ int64_t knn_lower_bound(const int32_t* __restrict__ items, int64_t lo, int64_t hi, int64_t v) {
  while (lo < hi) {
    const int64_t mid = (lo + hi) >> 1;
    if ((int64_t)items[mid] < v) lo = mid + 1; else hi = mid;
  }
  return lo;
}

// buf[0 .. S) into descending order; S a power of two <= KB_BUF; every thread of the workgroup calls it
__device__ __forceinline__ void knn_sort_desc(uint64_t* buf, int S) {
  const int t = threadIdx.x;
  for (int k = 2; k <= S; k <<= 1)
    for (int j = k >> 1; j > 0; j >>= 1) {
      if (t < (S >> 1)) {
        const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1));
        const int hi = lo | j;
        const uint64_t a = buf[lo], b = buf[hi];
        if ((lo & k) == 0 ? a < b : a > b) {
          buf[lo] = b;
          buf[hi] = a;
        }
      }
      __syncthreads();
    }
}

// the buffer cut back to its K largest keys, in descending order; *thr = the K-th (0 while there are fewer).  Every
// thread calls it, behind a barrier that made *count final.
__device__ __forceinline__ void knn_cut(uint64_t* buf, unsigned* count, uint64_t* thr, int K) {
  const int have = (int)*count;
  int S = TRS_WAVE;
  while (S < have) S <<= 1;
  for (int x = threadIdx.x; x < S; x += KB_THREADS)
    if (x >= have) buf[x] = 0;
  __syncthreads();
  knn_sort_desc(buf, S);
  if (threadIdx.x == 0) {
    const int keep = have < K ? have : K;
    *count = (unsigned)keep;
    *thr = keep == K ? buf[K - 1] : 0;
  }
  __syncthreads();
}

struct KnnBuild {
  const int64_t* hoff;     // user -> items
  const int32_t* hitems;
  const int64_t* ioff;     // item -> users
  const int32_t* iusers;
  int64_t n_users, n;
  int kind, K;
  double h;
  int32_t* ids_out;
  float* w_out;
  unsigned* next;          // the item counter
  int32_t* err;
};

__global__ __launch_bounds__(KB_THREADS) void knn_build_kernel(const KnnBuild a) {
  extern __shared__ __attribute__((aligned(16))) unsigned char knn_lds[];
  uint64_t* buf = reinterpret_cast<uint64_t*>(knn_lds);
  unsigned* cnt = reinterpret_cast<unsigned*>(knn_lds + (size_t)KB_BUF * 8);
  unsigned* touched = cnt + TRS_KNN_TILE;
  __shared__ unsigned s_item, s_count, s_touched;
  __shared__ uint64_t s_thr;

  const int tid = threadIdx.x, lane = tid & (TRS_WAVE - 1), wave = tid / TRS_WAVE;
  const int64_t n = a.n;
  const int ntiles = (int)((n + TRS_KNN_TILE - 1) / TRS_KNN_TILE);
  bool bad = false;

  for (int x = tid; x < TRS_KNN_TILE; x += KB_THREADS) cnt[x] = 0;
  if (tid == 0) s_touched = 0;

  for (;;) {
    __syncthreads();  // the previous item's reads of s_item / s_count are done
    if (tid == 0) {
      s_item = atomicAdd(a.next, 1u);
      s_count = 0;
      s_thr = 0;
    }
    __syncthreads();
    const int64_t i = s_item;
    if (i >= n) break;  // (uniform)
    const int64_t io = a.ioff[i];
    int64_t ni = a.ioff[i + 1] - io;
    if (ni < 0) ni = 0;
    const bool cursor = ntiles > 1 && ni <= KB_THREADS;  // (uniform) a thread owns a user and walks its list once

    // cursor mode: this thread's user and where its list stands
    int64_t pos = 0, end = 0;
    if (cursor && tid < ni) {
      const int64_t u = a.iusers[io + tid];
      if ((uint64_t)u < (uint64_t)a.n_users) {
        pos = a.hoff[u];
        end = a.hoff[u + 1];
        while (pos < end && a.hitems[pos] < 0) {  // never an address
          bad = true;
          ++pos;
        }
      } else {
        bad = true;
      }
    }

    for (int t = 0; t < ntiles && ni > 0; ++t) {
      const int64_t b0 = (int64_t)t * TRS_KNN_TILE;
      const int64_t tl = n - b0 < TRS_KNN_TILE ? n - b0 : TRS_KNN_TILE;
      // one more user of i holds id j: the counter, and the touched list on the first
      auto bump = [&](int64_t j) {
        const uint64_t x = (uint64_t)(j - b0);
        if (x < (uint64_t)tl) {
          if (atomicAdd(&cnt[x], 1u) == 0) {
            const unsigned p = atomicAdd(&s_touched, 1u);
            if (p < TRS_KNN_TOUCHED) touched[p] = (unsigned)x;
          }
        } else {
          bad = true;  // outside the catalogue, or a list that is not sorted: skipped
        }
      };

      if (cursor) {
        const int64_t b1 = b0 + tl;
        while (pos < end) {  // KB_BATCH entries requested together: a thread's walk is a chain of load latencies
          int32_t v[KB_BATCH];
#pragma unroll
          for (int q = 0; q < KB_BATCH; ++q) v[q] = pos + q < end ? a.hitems[pos + q] : INT32_MAX;  // (b1 <= INT32_MAX)
          int m = 0;
#pragma unroll
          for (int q = 0; q < KB_BATCH; ++q)
            if (m == q && (int64_t)v[q] < b1) {  // the entries in front of the tile's end
              bump(v[q]);
              ++m;
            }
          pos += m;
          if (m < KB_BATCH) break;
        }
        if (t == ntiles - 1 && pos < end) bad = true;  // ids >= n
      } else {
        for (int64_t c0 = (int64_t)wave * TRS_WAVE; c0 < ni; c0 += KB_WAVES * TRS_WAVE) {
          int64_t lo = 0, len = 0;
          if (c0 + lane < ni) {
            const int64_t u = a.iusers[io + c0 + lane];
            if ((uint64_t)u < (uint64_t)a.n_users) {
              const int64_t o = a.hoff[u], e = a.hoff[u + 1];
              if (e > o) {
                int64_t hi = e;
                lo = o;
                if (ntiles > 1) {
                  lo = knn_lower_bound(a.hitems, o, e, b0);
                  hi = knn_lower_bound(a.hitems, lo, e, b0 + tl);
                  if ((t == 0 && lo > o) || (t == ntiles - 1 && hi < e)) bad = true;  // ids < 0 or >= n
                }
                len = hi - lo;
              }
            } else {
              bad = true;
            }
          }
          if (len > 0 && len <= KB_SHORT)
            for (int64_t q = 0; q < len; ++q) bump(a.hitems[lo + q]);
          uint64_t m = __ballot(len > KB_SHORT);
          while (m) {  // (wave-uniform)
            const int src = __ffsll((unsigned long long)m) - 1;
            m &= m - 1;
            const int64_t slo = __shfl(lo, src, TRS_WAVE), sl = __shfl(len, src, TRS_WAVE);
            for (int64_t q = lane; q < sl; q += TRS_WAVE) bump(a.hitems[slo + q]);
          }
        }
      }
      __syncthreads();
      const unsigned nt = s_touched;
      __syncthreads();        // ... read by all before the next tile's adds
      if (nt == 0) continue;  // (uniform) nobody's list enters this tile
      if (tid == 0) s_touched = 0;  // for the next tile: every round below ends with a barrier

      const bool listed = nt <= TRS_KNN_TOUCHED;
      const int total = listed ? (int)nt : (int)tl;
      for (int r0 = 0; r0 < total; r0 += KB_THREADS) {
        const int e = r0 + tid;
        if (e < total) {
          const unsigned x = listed ? touched[e] : (unsigned)e;
          const unsigned c = cnt[x];
          if (c) {
            cnt[x] = 0;
            const int64_t j = b0 + x;
            if (j != i) {
              const int64_t nj = a.ioff[j + 1] - a.ioff[j];
              const uint64_t key = trs_topk_key(knn_sim(a.kind, a.h, c, ni, nj), (uint32_t)j);
              if (key > s_thr) buf[atomicAdd(&s_count, 1u)] = key;
            }
          }
        }
        __syncthreads();
        const bool full = s_count > KB_BUF - KB_THREADS;  // (uniform)
        __syncthreads();                                  // ... read by all before the next round appends
        if (full) knn_cut(buf, &s_count, &s_thr, a.K);
      }
    }

    __syncthreads();
    knn_cut(buf, &s_count, &s_thr, a.K);
    const int have = (int)s_count;
    for (int k = tid; k < a.K; k += KB_THREADS) {
      const uint64_t key = k < have ? buf[k] : 0;
      a.ids_out[i * a.K + k] = key ? (int32_t)(0xFFFFFFFFu - (uint32_t)key) : -1;
      a.w_out[i * a.K + k] = key ? trs_topk_key_score(key) : 0.f;
    }
  }
  if (bad && a.err) atomicOr(a.err, 1);
}

// ---------------------------------------------------------------------------------------------------- score rows
__global__ __launch_bounds__(TRS_BLOCK) void knn_rows_kernel(const int32_t* __restrict__ ids, const float* __restrict__ w,
                                                             int64_t n, int K, const int64_t* __restrict__ off,
                                                             const int32_t* __restrict__ items, int64_t csr_rows,
                                                             const int64_t* __restrict__ rows, float* __restrict__ out,
                                                             int32_t* __restrict__ err) {
  __shared__ float tile[KNN_ROW_TILE];
  const int tid = threadIdx.x;
  const int64_t r = blockIdx.x;
  const int64_t b0 = (int64_t)blockIdx.y * KNN_ROW_TILE;
  const int tl = (int)(n - b0 < KNN_ROW_TILE ? n - b0 : KNN_ROW_TILE);
  const bool report = blockIdx.y == 0 && err != nullptr;
  const int64_t hrow = rows[r];
  int64_t o = 0, len = 0;
  if ((uint64_t)hrow < (uint64_t)csr_rows) {
    o = off[hrow];
    len = off[hrow + 1] - o;
    if (len < 0) len = 0;
  } else if (report && tid == 0) {
    atomicOr(err, 1);  // a row outside the CSR: an empty history
  }
  for (int x = tid; x < tl; x += TRS_BLOCK) tile[x] = 0.f;
  __syncthreads();
  for (int64_t p = 0; p < len; ++p) {
    const int64_t i = items[o + p];  // (uniform)
    if ((uint64_t)i < (uint64_t)n) {
      if (tid < K) {
        const int64_t j = ids[i * K + tid];
        const uint64_t x = (uint64_t)(j - b0);
        if (x < (uint64_t)tl)
          tile[x] += w[i * K + tid];  // a row lists a column once: the K lanes write K distinct entries
        else if (report && (j < -1 || j >= n))
          atomicOr(err, 1);  // never an address
      }
    } else if (report && tid == 0) {
      atomicOr(err, 1);  // never an address
    }
    __syncthreads();
  }
  float* dst = out + r * n + b0;
  for (int x = tid; x < tl; x += TRS_BLOCK) dst[x] = tile[x];
}

static inline bool knn_kind_ok(int kind) {
  return kind == TRS_KNN_COSINE || kind == TRS_KNN_JACCARD || kind == TRS_KNN_CONDITIONAL || kind == TRS_KNN_COUNT;
}
static inline bool knn_csr_ok(const trs_csr* c) { return c != nullptr && c->off != nullptr && c->items != nullptr; }

}  // namespace

extern "C" int64_t trs_knn_build_workspace_bytes(int64_t n, int32_t K) {
  if (n < 1 || n > INT32_MAX || K < 1 || K > TRS_KNN_KMAX) return 0;
  return 256;  // the item counter, on a line of its own
}

extern "C" int trs_knn_build(const trs_csr* hist, const trs_csr* inv, int64_t n_users, int64_t n, int32_t kind,
                             double shrinkage, int32_t K, int32_t* nbr_ids_out_dev, float* nbr_w_out_dev,
                             void* workspace_dev, int64_t workspace_bytes, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_knn_build";
  TRS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n=%lld outside 1..2^31-1", who, (long long)n);
  TRS_REQUIRE(n_users >= 0 && n_users <= INT32_MAX, "%s: n_users=%lld outside 0..2^31-1", who, (long long)n_users);
  TRS_REQUIRE(K >= 1 && K <= TRS_KNN_KMAX, "%s: K=%d outside 1..%d", who, K, TRS_KNN_KMAX);
  TRS_REQUIRE(knn_kind_ok(kind), "%s: unknown kind %d", who, kind);
  TRS_REQUIRE(shrinkage >= 0.0 && shrinkage <= 1.79769313486231570815e+308, "%s: shrinkage must be finite and >= 0",
              who);
  TRS_REQUIRE(nbr_ids_out_dev != nullptr && nbr_w_out_dev != nullptr, "%s: nbr_ids_out / nbr_w_out is NULL", who);
  TRS_REQUIRE(knn_csr_ok(hist) && knn_csr_ok(inv), "%s: a CSR is NULL or has NULL arrays", who);
  TRS_REQUIRE(hist->n_rows == n_users, "%s: history CSR has %lld rows for n_users=%lld", who, (long long)hist->n_rows,
              (long long)n_users);
  TRS_REQUIRE(inv->n_rows == n, "%s: inverse CSR has %lld rows for n=%lld", who, (long long)inv->n_rows, (long long)n);
  TRS_REQUIRE(workspace_dev != nullptr, "%s: workspace is NULL", who);
  TRS_REQUIRE(workspace_bytes >= trs_knn_build_workspace_bytes(n, K), "%s: workspace of %lld bytes, %lld needed", who,
              (long long)workspace_bytes, (long long)trs_knn_build_workspace_bytes(n, K));
  hipStream_t s = (hipStream_t)stream;
  (void)hipFuncSetAttribute((const void*)knn_build_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, (int)KB_LDS);
  if (hipMemsetAsync(workspace_dev, 0, 256, s) != hipSuccess) {
    trs_set_error("%s: hipMemsetAsync failed", who);
    return TRS_E_LAUNCH;
  }
  const KnnBuild a = {hist->off, hist->items, inv->off, inv->items, n_users, n, kind, K, shrinkage,
                      nbr_ids_out_dev, nbr_w_out_dev, (unsigned*)workspace_dev, err_flag_dev};
  const int64_t grid = n < 512 ? n : 512;  // 256 CUs x 2 resident workgroups; the counter hands out the items
  hipLaunchKernelGGL(knn_build_kernel, dim3((unsigned)grid), dim3(KB_THREADS), KB_LDS, s, a);
  TRS_CHECK_LAUNCH("knn_build_kernel");
  return TRS_OK;
}

extern "C" int trs_knn_scores(const int32_t* nbr_ids_dev, const float* nbr_w_dev, int64_t n, int32_t K,
                              const trs_csr* hist, const int64_t* rows_dev, int64_t n_rows, float* out_dev,
                              int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_knn_scores";
  TRS_REQUIRE(n >= 1 && n <= INT32_MAX, "%s: n=%lld outside 1..2^31-1", who, (long long)n);
  TRS_REQUIRE(K >= 1 && K <= TRS_KNN_KMAX, "%s: K=%d outside 1..%d", who, K, TRS_KNN_KMAX);
  TRS_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "%s: n_rows=%lld outside 0..2^31-1", who, (long long)n_rows);
  if (n_rows == 0) return TRS_OK;
  TRS_REQUIRE(nbr_ids_dev != nullptr && nbr_w_dev != nullptr && rows_dev != nullptr && out_dev != nullptr,
              "%s: nbr_ids / nbr_w / rows / out is NULL", who);
  TRS_REQUIRE(knn_csr_ok(hist), "%s: history CSR is NULL or has NULL arrays", who);
  TRS_REQUIRE(hist->n_rows >= 1, "%s: history CSR has %lld rows", who, (long long)hist->n_rows);
  const int64_t tiles = (n + KNN_ROW_TILE - 1) / KNN_ROW_TILE;
  TRS_REQUIRE(tiles <= 65535, "%s: n=%lld needs more than 65535 column tiles", who, (long long)n);
  hipLaunchKernelGGL(knn_rows_kernel, dim3((unsigned)n_rows, (unsigned)tiles), dim3(TRS_BLOCK), 0, (hipStream_t)stream,
                     nbr_ids_dev, nbr_w_dev, n, (int)K, hist->off, hist->items, hist->n_rows, rows_dev, out_dev,
                     err_flag_dev);
  TRS_CHECK_LAUNCH("knn_rows_kernel");
  return TRS_OK;
}
