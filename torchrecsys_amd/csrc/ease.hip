// ease.hip — EASE (Steck, WWW 2019): the closed-form item-item model of model.py fit_ease.  The rule is the contract in
// include/trs.h "EASE", the design in DESIGN.md 4.17.
//
// ease_gram_init_kernel     A = 0 with 1 on the diagonal of the padding (rows / columns n .. nbar-1).
// ease_gram_pairs_kernel    one wave per user: an fp64 atomic add of 1.0 per ordered pair of the user's items.  Every
//                           partial sum is an integer below 2^53, so the result is exact whatever the order.
// ease_gram_diag_kernel     A[i][i] += lambda: one rounding, after the counts are complete.
// ease_chol_block_kernel    one wave factors an NB x NB diagonal block in LDS (left-looking, column by column, the pivot
//                           handed out by a shuffle) and inverts the factor (one lane per column, forward substitution).
// ease_gemm_kernel<TA, TB>  C <- beta C + alpha op(A) op(B) in fp64 on v_mfma_f64_16x16x4_f64: a workgroup of four waves
//                           owns a 64 x 64 tile of C, a wave 32 x 32 of it (2 x 2 MFMA tiles); K in steps of 16 through
//                           LDS, the next step's operands requested into registers before the current step's MFMAs.
// ease_mirror_kernel        the upper triangle from the lower one.
// ease_weights_kernel       B[i][j] = (float)(-P[i][j] / P[j][j]), B[i][i] = 0.
// ease_rows_kernel<VEC>     out[r] = the sum of the rows of B a history lists, in CSR order, one fp32 add per item.
#include "trs_common.h"

#include <math.h>

namespace {

constexpr int NB = TRS_EASE_NB;  // block size of the solver == tile edge of the GEMM kernel
static_assert(NB == 64, "the kernels below are written for 64 x 64 blocks");

static inline int64_t ease_nbar(int64_t n) { return (n + NB - 1) / NB * NB; }

// ---------------------------------------------------------------------------------------------------- Gram
__global__ __launch_bounds__(TRS_BLOCK) void ease_gram_init_kernel(double* __restrict__ A, int64_t n, int64_t nbar) {
  const int64_t total = nbar * nbar;
  for (int64_t e = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x; e < total; e += (int64_t)gridDim.x * TRS_BLOCK) {
    const int64_t r = e / nbar, c = e - r * nbar;
    A[e] = (r == c && r >= n) ? 1.0 : 0.0;
  }
}

__global__ __launch_bounds__(TRS_BLOCK) void ease_gram_pairs_kernel(const int64_t* __restrict__ off,
                                                                    const int32_t* __restrict__ items, int64_t n_users,
                                                                    int64_t n, int64_t nbar, double* __restrict__ A,
                                                                    int32_t* __restrict__ err) {
  const int lane = threadIdx.x & (TRS_WAVE - 1);
  const int64_t waves = (int64_t)gridDim.x * (TRS_BLOCK / TRS_WAVE);
  for (int64_t u = (int64_t)blockIdx.x * (TRS_BLOCK / TRS_WAVE) + threadIdx.x / TRS_WAVE; u < n_users; u += waves) {
    const int64_t o = off[u];
    int64_t len = off[u + 1] - o;
    if (len <= 0) continue;  // (wave-uniform)
    if (len > n) {           // more entries than items: not a list of distinct items
      if (lane == 0 && err) atomicOr(err, 1);
      continue;
    }
    const int64_t pairs = len * len;
    for (int64_t e = lane; e < pairs; e += TRS_WAVE) {
      const int64_t a = e / len, b = e - a * len;
      const int64_t i = items[o + a], j = items[o + b];
      if ((uint64_t)i < (uint64_t)n && (uint64_t)j < (uint64_t)n)
        atomicAdd(&A[i * nbar + j], 1.0);
      else if (err)
        atomicOr(err, 1);  // never an address
    }
  }
}

__global__ __launch_bounds__(TRS_BLOCK) void ease_gram_diag_kernel(double* __restrict__ A, int64_t n, int64_t nbar,
                                                                   double lambda) {
  const int64_t i = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x;
  if (i < n) A[i * nbar + i] += lambda;
}

// ---------------------------------------------------------------------------------------------------- diagonal block
constexpr int CH_LD = NB + 1;

// A_kk = L L^T of the lower triangle of the NB x NB block at A (row stride ld); L (upper triangle 0) is written back
// over it and W = L^-1 (upper triangle 0) to the block at Wout.  One wave: lane i owns row i of L and column i of W.
__global__ __launch_bounds__(NB) void ease_chol_block_kernel(double* __restrict__ A, double* __restrict__ Wout,
                                                             int64_t ld, int32_t* __restrict__ err) {
  __shared__ double S[NB * CH_LD];
  __shared__ double W[NB * CH_LD];
  const int i = threadIdx.x;
  for (int r = 0; r < NB; ++r) S[r * CH_LD + i] = i <= r ? A[(int64_t)r * ld + i] : 0.0;
  __syncthreads();

  bool bad = false;
  for (int j = 0; j < NB; ++j) {
    double s = S[i * CH_LD + j];
    for (int k = 0; k < j; ++k) s -= S[i * CH_LD + k] * S[j * CH_LD + k];
    double d = __shfl(s, j, NB);  // the pivot
    if (!(d > 0.0) || !(d <= 1.79769313486231570815e+308)) {  // (wave-uniform) not positive or not finite
      bad = true;
      d = 1.0;
      if (i == j) s = 1.0;
    }
    const double l = sqrt(d);
    __syncthreads();
    if (i >= j) S[i * CH_LD + j] = i == j ? l : s / l;
    __syncthreads();
  }
  if (bad && i == 0 && err) atomicOr(err, 1);

  // column i of W: L w = e_i by forward substitution, rows i .. NB-1
  for (int r = 0; r < NB; ++r) {
    if (r < i) {
      W[r * CH_LD + i] = 0.0;
    } else if (r == i) {
      W[r * CH_LD + i] = 1.0 / S[r * CH_LD + r];
    } else {
      double s = 0.0;
      for (int k = i; k < r; ++k) s += S[r * CH_LD + k] * W[k * CH_LD + i];
      W[r * CH_LD + i] = -s / S[r * CH_LD + r];
    }
  }
  __syncthreads();
  for (int r = 0; r < NB; ++r) {
    A[(int64_t)r * ld + i] = S[r * CH_LD + i];
    Wout[(int64_t)r * ld + i] = W[r * CH_LD + i];
  }
}

// ---------------------------------------------------------------------------------------------------- fp64 GEMM
typedef double ease_d4 __attribute__((ext_vector_type(4)));

constexpr int GM_KB = 16;       // K per LDS stage
constexpr int GM_LD = NB + 16;  // LDS row stride in doubles: rows k and k + 1 of a stage start 128 B apart mod 256

enum { EASE_K_ALL = 0, EASE_K_FROM_COL = 1, EASE_K_FROM_MAX = 2 };

struct EaseGemm {
  const double* A;  // op(A) is (M, K): TA ? A is (K, M) : (M, K), row stride lda
  const double* B;  // op(B) is (K, N): TB ? B is (N, K) : (K, N), row stride ldb
  double* C;        // (M, N), row stride ldc; may be the memory of one operand where the launcher says so
  int64_t lda, ldb, ldc;
  int64_t K;        // a multiple of NB
  double alpha, beta;
  int lower;        // 1: only the tiles with tile row >= tile column
  int kmode;        // where the K loop starts: 0 | NB * tile column | NB * max(tile row, tile column)
};

// one K stage of one operand into registers: 64 x 16 doubles, four per thread.
//   CONTIG_K (the stored matrix has K along its rows): thread t reads row t / 4, k = 4 (t % 4) .. + 3
//   otherwise (K along its columns):                   thread t reads k = t / 16, columns 4 (t % 16) .. + 3
template <bool CONTIG_K>
__device__ __forceinline__ void ease_fetch(const double* base, int64_t ld, int64_t k0, double (&v)[4]) {  // (may alias C)
  const int t = threadIdx.x;
  const double* p = CONTIG_K ? base + (int64_t)(t >> 2) * ld + k0 + 4 * (t & 3)
                             : base + (k0 + (t >> 4)) * ld + 4 * (t & 15);
  const double2 a = *reinterpret_cast<const double2*>(p);
  const double2 b = *reinterpret_cast<const double2*>(p + 2);
  v[0] = a.x;
  v[1] = a.y;
  v[2] = b.x;
  v[3] = b.y;
}
// ... and from the registers into the stage image S[k][row or column]
template <bool CONTIG_K>
__device__ __forceinline__ void ease_stash(double* __restrict__ S, const double (&v)[4]) {
  const int t = threadIdx.x;
  if (CONTIG_K) {
#pragma unroll
    for (int c = 0; c < 4; ++c) S[(4 * (t & 3) + c) * GM_LD + (t >> 2)] = v[c];
  } else {
    double* q = S + (t >> 4) * GM_LD + 4 * (t & 15);
    *reinterpret_cast<double2*>(q) = make_double2(v[0], v[1]);
    *reinterpret_cast<double2*>(q + 2) = make_double2(v[2], v[3]);
  }
}

template <bool TA, bool TB>
__global__ __launch_bounds__(TRS_BLOCK) void ease_gemm_kernel(const EaseGemm g) {
  __shared__ __attribute__((aligned(16))) double As[GM_KB * GM_LD];
  __shared__ __attribute__((aligned(16))) double Bs[GM_KB * GM_LD];
  const int ti = blockIdx.y, tj = blockIdx.x;
  if (g.lower && ti < tj) return;  // (uniform)
  int64_t k_begin = 0;
  if (g.kmode == EASE_K_FROM_COL) k_begin = (int64_t)tj * NB;
  if (g.kmode == EASE_K_FROM_MAX) k_begin = (int64_t)(ti > tj ? ti : tj) * NB;

  // the tile's rows of op(A) and columns of op(B)
  const double* Ab = TA ? g.A + (int64_t)ti * NB : g.A + (int64_t)ti * NB * g.lda;
  const double* Bb = TB ? g.B + (int64_t)tj * NB * g.ldb : g.B + (int64_t)tj * NB;

  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int wm = (wave >> 1) * 32, wn = (wave & 1) * 32;
  const int lr = lane & 15, lk = lane >> 4;

  ease_d4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = ease_d4{0.0, 0.0, 0.0, 0.0};

  double ra[4], rb[4];
  if (k_begin < g.K) {
    ease_fetch<!TA>(Ab, g.lda, k_begin, ra);
    ease_fetch<TB>(Bb, g.ldb, k_begin, rb);
  }
  for (int64_t k0 = k_begin; k0 < g.K; k0 += GM_KB) {
    __syncthreads();  // the previous stage has been read
    ease_stash<!TA>(As, ra);
    ease_stash<TB>(Bs, rb);
    __syncthreads();
    if (k0 + GM_KB < g.K) {  // (uniform) the next stage, in flight during this stage's MFMAs
      ease_fetch<!TA>(Ab, g.lda, k0 + GM_KB, ra);
      ease_fetch<TB>(Bb, g.ldb, k0 + GM_KB, rb);
    }
#pragma unroll
    for (int kk = 0; kk < GM_KB; kk += 4) {
      double a[2], b[2];
#pragma unroll
      for (int x = 0; x < 2; ++x) {
        a[x] = As[(kk + lk) * GM_LD + wm + 16 * x + lr];  // A[row lr][k lk]
        b[x] = Bs[(kk + lk) * GM_LD + wn + 16 * x + lr];  // B[k lk][column lr]
      }
#pragma unroll
      for (int x = 0; x < 2; ++x)
#pragma unroll
        for (int y = 0; y < 2; ++y) acc[x][y] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[x], b[y], acc[x][y], 0, 0, 0);
    }
  }

  // C/D of the fp64 MFMA: column = lane & 15, row = (lane >> 4) + 4 * register
#pragma unroll
  for (int x = 0; x < 2; ++x)
#pragma unroll
    for (int y = 0; y < 2; ++y)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = (int64_t)ti * NB + wm + 16 * x + lk + 4 * r;
        const int64_t col = (int64_t)tj * NB + wn + 16 * y + lr;
        double* c = g.C + row * g.ldc + col;
        const double v = g.alpha * acc[x][y][r];
        *c = g.beta == 0.0 ? v : g.beta * *c + v;
      }
}

// M x N (multiples of NB) tiles of C.  An operand may alias C only tile for tile with K == NB (the panel products): a
// workgroup then reads exactly the tile it writes, and has read all of it before its first store.
template <bool TA, bool TB>
static void ease_gemm(int64_t M, int64_t N, int64_t K, double alpha, const double* A, int64_t lda, const double* B,
                      int64_t ldb, double beta, double* C, int64_t ldc, int lower, int kmode, hipStream_t s) {
  if (M <= 0 || N <= 0) return;
  EaseGemm g = {A, B, C, lda, ldb, ldc, K, alpha, beta, lower, kmode};
  hipLaunchKernelGGL((ease_gemm_kernel<TA, TB>), dim3((unsigned)(N / NB), (unsigned)(M / NB)), dim3(TRS_BLOCK), 0, s, g);
}

__global__ __launch_bounds__(TRS_BLOCK) void ease_mirror_kernel(double* __restrict__ P, int64_t nbar) {
  // a 16 x 16 tile per workgroup: upper entry (r, c), r < c, from (c, r), turned through LDS
  __shared__ double T[16][17];
  if (blockIdx.x < blockIdx.y) return;  // (uniform)
  const int a = threadIdx.x / 16, b = threadIdx.x % 16;
  T[a][b] = P[((int64_t)blockIdx.x * 16 + a) * nbar + (int64_t)blockIdx.y * 16 + b];
  __syncthreads();
  const int64_t r = (int64_t)blockIdx.y * 16 + a, c = (int64_t)blockIdx.x * 16 + b;
  if (r < c) P[r * nbar + c] = T[b][a];
}

// ---------------------------------------------------------------------------------------------------- weights
__global__ __launch_bounds__(TRS_BLOCK) void ease_weights_kernel(const double* __restrict__ P, int64_t n, int64_t ldp,
                                                                 float* __restrict__ B) {
  const int64_t j = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x;
  if (j >= n) return;
  const double d = P[j * ldp + j];
  for (int64_t i = blockIdx.y; i < n; i += gridDim.y)
    B[i * n + j] = i == j ? 0.f : (float)(-P[i * ldp + j] / d);
}

// ---------------------------------------------------------------------------------------------------- score rows
constexpr int SR_DEPTH = 4;  // rows of B requested together

template <bool VEC>
__global__ __launch_bounds__(TRS_BLOCK) void ease_rows_kernel(const float* __restrict__ B, int64_t n,
                                                              const int64_t* __restrict__ off,
                                                              const int32_t* __restrict__ items, int64_t csr_rows,
                                                              const int64_t* __restrict__ rows, float* __restrict__ out,
                                                              int32_t* __restrict__ err) {
  const int64_t r = blockIdx.x;
  const int64_t h = rows[r];
  int64_t o = 0, len = 0;
  if ((uint64_t)h < (uint64_t)csr_rows) {
    o = off[h];
    len = off[h + 1] - o;
    if (len < 0) len = 0;
  } else if (threadIdx.x == 0 && blockIdx.y == 0 && err) {
    atomicOr(err, 1);  // a row outside the CSR: an empty history
  }
  // VEC: columns 4t .. 4t+3 of a tile of 1024; otherwise column t of each of the tile's four quarters
  const int64_t c0 = (int64_t)blockIdx.y * (4 * TRS_BLOCK) + (VEC ? 4 * threadIdx.x : threadIdx.x);
  float acc[4] = {0.f, 0.f, 0.f, 0.f};
  auto col = [&](int q) { return VEC ? c0 + q : c0 + (int64_t)q * TRS_BLOCK; };

  for (int64_t p = 0; p < len; p += SR_DEPTH) {
    float v[SR_DEPTH][4];
    bool ok[SR_DEPTH];
#pragma unroll
    for (int d = 0; d < SR_DEPTH; ++d) {
      const bool has = p + d < len;
      const int64_t id = has ? (int64_t)items[o + p + d] : 0;
      ok[d] = has && (uint64_t)id < (uint64_t)n;
      if (has && !ok[d] && threadIdx.x == 0 && blockIdx.y == 0 && err) atomicOr(err, 1);  // never an address
      const float* row = B + (ok[d] ? id : 0) * n;
      if (VEC) {
        const float4 x = c0 < n ? *reinterpret_cast<const float4*>(row + c0) : make_float4(0.f, 0.f, 0.f, 0.f);
        v[d][0] = x.x;
        v[d][1] = x.y;
        v[d][2] = x.z;
        v[d][3] = x.w;
      } else {
#pragma unroll
        for (int q = 0; q < 4; ++q) v[d][q] = col(q) < n ? row[col(q)] : 0.f;
      }
    }
#pragma unroll
    for (int d = 0; d < SR_DEPTH; ++d)
      if (ok[d]) {
#pragma unroll
        for (int q = 0; q < 4; ++q) acc[q] += v[d][q];
      }
  }
  float* dst = out + r * n;
  if (VEC) {
    if (c0 < n) *reinterpret_cast<float4*>(dst + c0) = make_float4(acc[0], acc[1], acc[2], acc[3]);
  } else {
#pragma unroll
    for (int q = 0; q < 4; ++q)
      if (col(q) < n) dst[col(q)] = acc[q];
  }
}

static inline bool ease_lambda_ok(double lambda) { return lambda > 0.0 && lambda <= 1.79769313486231570815e+308; }

}  // namespace

extern "C" int trs_ease_gram(const trs_csr* hist, int64_t n_users, int64_t n, double lambda, double* A_out_dev,
                             int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_ease_gram";
  TRS_REQUIRE(n >= 1 && n <= TRS_EASE_NMAX, "%s: n=%lld outside 1..%d", who, (long long)n, TRS_EASE_NMAX);
  TRS_REQUIRE(ease_lambda_ok(lambda), "%s: lambda must be finite and > 0", who);
  TRS_REQUIRE(n_users >= 0 && n_users <= INT32_MAX, "%s: n_users=%lld outside 0..2^31-1", who, (long long)n_users);
  TRS_REQUIRE(A_out_dev != nullptr, "%s: A_out is NULL", who);
  TRS_REQUIRE(hist != nullptr && hist->off && (hist->items || n_users == 0), "%s: history CSR is NULL or has NULL arrays",
              who);
  TRS_REQUIRE(hist->n_rows == n_users, "%s: history CSR has %lld rows for n_users=%lld", who, (long long)hist->n_rows,
              (long long)n_users);
  hipStream_t s = (hipStream_t)stream;
  const int64_t nbar = ease_nbar(n);
  hipLaunchKernelGGL(ease_gram_init_kernel, dim3((unsigned)trs_grid(nbar * nbar, TRS_BLOCK)), dim3(TRS_BLOCK), 0, s,
                     A_out_dev, n, nbar);
  TRS_CHECK_LAUNCH("ease_gram_init_kernel");
  if (n_users > 0) {
    hipLaunchKernelGGL(ease_gram_pairs_kernel, dim3((unsigned)trs_grid(n_users, TRS_BLOCK / TRS_WAVE)), dim3(TRS_BLOCK),
                       0, s, hist->off, hist->items, n_users, n, nbar, A_out_dev, err_flag_dev);
    TRS_CHECK_LAUNCH("ease_gram_pairs_kernel");
  }
  hipLaunchKernelGGL(ease_gram_diag_kernel, dim3((unsigned)((n + TRS_BLOCK - 1) / TRS_BLOCK)), dim3(TRS_BLOCK), 0, s,
                     A_out_dev, n, nbar, lambda);
  TRS_CHECK_LAUNCH("ease_gram_diag_kernel");
  return TRS_OK;
}

extern "C" int64_t trs_ease_invert_workspace_bytes(int64_t n) {
  if (n < 1 || n > TRS_EASE_NMAX) return 0;
  const int64_t nbar = ease_nbar(n);
  return nbar * nbar * 8;
}

extern "C" int trs_ease_invert(double* A_inout_dev, int64_t n, void* workspace_dev, int64_t workspace_bytes,
                               int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_ease_invert";
  TRS_REQUIRE(n >= 1 && n <= TRS_EASE_NMAX, "%s: n=%lld outside 1..%d", who, (long long)n, TRS_EASE_NMAX);
  TRS_REQUIRE(A_inout_dev != nullptr, "%s: A_inout is NULL", who);
  TRS_REQUIRE(workspace_dev != nullptr, "%s: workspace is NULL", who);
  TRS_REQUIRE(err_flag_dev != nullptr, "%s: err_flag is NULL", who);
  TRS_REQUIRE(workspace_bytes >= trs_ease_invert_workspace_bytes(n), "%s: workspace of %lld bytes, %lld needed", who,
              (long long)workspace_bytes, (long long)trs_ease_invert_workspace_bytes(n));
  TRS_REQUIRE((reinterpret_cast<uintptr_t>(A_inout_dev) & 15) == 0 && (reinterpret_cast<uintptr_t>(workspace_dev) & 15) == 0,
              "%s: A_inout / workspace must be 16-byte aligned", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t ld = ease_nbar(n), nb = ld / NB;
  double* A = A_inout_dev;
  double* M = (double*)workspace_dev;
  auto blk = [&](double* X, int64_t i, int64_t j) { return X + (i * ld + j) * NB; };  // block (i, j) of X
  const int stages = trs_tuning().ease_stages;
  TRS_REQUIRE(stages >= 1 && stages <= 7, "%s: EASE_STAGES=%d outside 1..7", who, stages);

  // 1. A = L L^T, right-looking; W_kk = L_kk^-1 goes to block (k, k) of M
  for (int64_t k = 0; k < nb && (stages & 1); ++k) {
    hipLaunchKernelGGL(ease_chol_block_kernel, dim3(1), dim3(NB), 0, s, blk(A, k, k), blk(M, k, k), ld, err_flag_dev);
    const int64_t rest = (nb - k - 1) * NB;
    // panel L_ik = A_ik W_kk^T, in place (tile for tile, K == NB)
    ease_gemm<false, true>(rest, NB, NB, 1.0, blk(A, k + 1, k), ld, blk(M, k, k), ld, 0.0, blk(A, k + 1, k), ld, 0,
                           EASE_K_ALL, s);
    // trailing A_ij -= L_ik L_jk^T, i >= j > k
    ease_gemm<false, true>(rest, rest, NB, -1.0, blk(A, k + 1, k), ld, blk(A, k + 1, k), ld, 1.0, blk(A, k + 1, k + 1),
                           ld, 1, EASE_K_ALL, s);
  }
  TRS_CHECK_LAUNCH("ease_chol_block_kernel / ease_gemm_kernel (factor)");
  // 2. M = L^-1 by block rows: T_ik = sum_{j=k}^{i-1} L_ij M_jk into M's block row i, then M_ik = -W_ii T_ik in place
  for (int64_t i = 1; i < nb && (stages & 2); ++i) {
    ease_gemm<false, false>(NB, i * NB, i * NB, 1.0, blk(A, i, 0), ld, M, ld, 0.0, blk(M, i, 0), ld, 0,
                            EASE_K_FROM_COL, s);
    ease_gemm<false, false>(NB, i * NB, NB, -1.0, blk(M, i, i), ld, blk(M, i, 0), ld, 0.0, blk(M, i, 0), ld, 0,
                            EASE_K_ALL, s);
  }
  TRS_CHECK_LAUNCH("ease_gemm_kernel (triangular inverse)");
  // 3. P = M^T M into A: lower tiles (block row l of M contributes from l = max(i, j) on), then the mirror image
  if (stages & 4) {
    ease_gemm<true, false>(ld, ld, ld, 1.0, M, ld, M, ld, 0.0, A, ld, 1, EASE_K_FROM_MAX, s);
    hipLaunchKernelGGL(ease_mirror_kernel, dim3((unsigned)(ld / 16), (unsigned)(ld / 16)), dim3(TRS_BLOCK), 0, s, A, ld);
  }
  TRS_CHECK_LAUNCH("ease_gemm_kernel / ease_mirror_kernel (product)");
  return TRS_OK;
}

extern "C" int trs_ease_weights(const double* P_dev, int64_t n, float* B_out_dev, void* stream) {
  const char* who = "trs_ease_weights";
  TRS_REQUIRE(n >= 1 && n <= TRS_EASE_NMAX, "%s: n=%lld outside 1..%d", who, (long long)n, TRS_EASE_NMAX);
  TRS_REQUIRE(P_dev != nullptr && B_out_dev != nullptr, "%s: P / B_out is NULL", who);
  const unsigned gy = (unsigned)(n < 1024 ? n : 1024);
  hipLaunchKernelGGL(ease_weights_kernel, dim3((unsigned)((n + TRS_BLOCK - 1) / TRS_BLOCK), gy), dim3(TRS_BLOCK), 0,
                     (hipStream_t)stream, P_dev, n, ease_nbar(n), B_out_dev);
  TRS_CHECK_LAUNCH("ease_weights_kernel");
  return TRS_OK;
}

extern "C" int trs_ease_scores(const float* B_dev, int64_t n, const trs_csr* hist, const int64_t* rows_dev,
                               int64_t n_rows, float* out_dev, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_ease_scores";
  TRS_REQUIRE(n >= 1 && n <= TRS_EASE_NMAX, "%s: n=%lld outside 1..%d", who, (long long)n, TRS_EASE_NMAX);
  TRS_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "%s: n_rows=%lld outside 0..2^31-1", who, (long long)n_rows);
  if (n_rows == 0) return TRS_OK;
  TRS_REQUIRE(B_dev != nullptr && rows_dev != nullptr && out_dev != nullptr, "%s: B / rows / out is NULL", who);
  TRS_REQUIRE(hist != nullptr && hist->off && hist->items, "%s: history CSR is NULL or has NULL arrays", who);
  TRS_REQUIRE(hist->n_rows >= 1, "%s: history CSR has %lld rows", who, (long long)hist->n_rows);
  const dim3 grid((unsigned)n_rows, (unsigned)((n + 4 * TRS_BLOCK - 1) / (4 * TRS_BLOCK)));
  const bool vec = (n & 3) == 0 && (reinterpret_cast<uintptr_t>(B_dev) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(out_dev) & 15) == 0;
  if (vec)
    hipLaunchKernelGGL(ease_rows_kernel<true>, grid, dim3(TRS_BLOCK), 0, (hipStream_t)stream, B_dev, n, hist->off,
                       hist->items, hist->n_rows, rows_dev, out_dev, err_flag_dev);
  else
    hipLaunchKernelGGL(ease_rows_kernel<false>, grid, dim3(TRS_BLOCK), 0, (hipStream_t)stream, B_dev, n, hist->off,
                       hist->items, hist->n_rows, rows_dev, out_dev, err_flag_dev);
  TRS_CHECK_LAUNCH("ease_rows_kernel");
  return TRS_OK;
}
