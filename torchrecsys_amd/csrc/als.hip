// als.hip — implicit-feedback alternating least squares (model.py fit_als; the rule is the contract in include/trs.h
// "implicit ALS", the design in DESIGN.md 4.16): the Gram matrix of the frozen table and one half-sweep of per-row
// conjugate gradient.
//
// als_gram_partial_kernel   G = Y^T Y in two deterministic stages.  The rows are cut into chunks of a size that depends
// als_gram_reduce_kernel    on (n, D) only; a workgroup forms one 64 x 64 tile of one chunk's partial Gram matrix (rows
//                           staged 16 at a time in LDS, a 4 x 4 register tile per thread, one fmaf chain per entry in
//                           ascending row order), the reduce kernel adds the chunks in ascending order.  No atomics.
// als_solve_kernel<G, VEC, GLDS>  one row per aligned lane group of G = Dp / 4 lanes (Dp = D rounded up to a power of
//                           two >= 16), as fold_in_kernel: lane l keeps columns 4l .. 4l+3 of x, r and p in registers,
//                           dot products by trs_group_sum<G>.  Workgroups are persistent (a grid-stride loop over tiles
//                           of rows), so the Gram matrix is staged once per workgroup, not once per row tile.
//   G v        lane l accumulates sum_e G[e][4l..4l+3] * v_e for e ascending; v_e comes from its owner lane by a
//              shuffle, the row of G from LDS (GLDS: Dp <= 128, Dp * Dp * 4 <= 64 KiB, padding zero) or from L2 (Dp = 256:
//              256 KiB does not fit; every lane group of a wave reads the same addresses).
//   walk       A v needs sum_{i in N} (y_i . v) y_i: one pass over the neighbour rows per CG step and one for the set-up,
//              which also sums the rows for b.  ALS_DEPTH rows are kept requested in a ring of registers; the ids of G
//              neighbours are loaded by the G lanes at once, one chunk ahead, and handed out by shuffle.  No branch
//              around a row load (see fold_in_kernel): a neighbour that is off reads row 0 and is dropped.
//   lock-step  the rows of a wave have different list lengths and stop at different steps; every lane runs to the
//              longest list and the last active row of its wave with its updates predicated off.  No early return.
#include "trs_common.h"

namespace {

constexpr int ALS_DEPTH = 4;            // neighbour rows kept requested per lane group
constexpr float ALS_RHO_STOP = 1e-20f;  // r.r below this: the row has converged

// ---------------------------------------------------------------------------------------------------- Gram
constexpr int GR_TILE = 64;  // output tile edge of a workgroup
constexpr int GR_KB = 16;    // rows staged per trip

static inline int64_t gram_chunk_rows(int64_t n, int D) {
  const int64_t cap = D > 128 ? 256 : 512;  // most chunks: bounds the workspace (cap * D * D * 4 bytes <= 64 MiB)
  int64_t r = (n + cap - 1) / cap;
  r = (r + GR_KB - 1) / GR_KB * GR_KB;
  return r < GR_KB ? GR_KB : r;
}
static inline int64_t gram_chunks(int64_t n, int D) {
  const int64_t r = gram_chunk_rows(n, D);
  return (n + r - 1) / r;
}

__global__ __launch_bounds__(TRS_BLOCK) void als_gram_partial_kernel(const float* __restrict__ Y, int64_t n, int D,
                                                                     int64_t ld, int64_t chunk_rows,
                                                                     float* __restrict__ part) {
  __shared__ __attribute__((aligned(16))) float As[GR_KB][GR_TILE], Bs[GR_KB][GR_TILE];
  const int64_t c = blockIdx.x;
  const int ci = blockIdx.y * GR_TILE, cj = blockIdx.z * GR_TILE;
  const int64_t r0 = c * chunk_rows;
  const int64_t r1 = r0 + chunk_rows < n ? r0 + chunk_rows : n;
  const int ty = threadIdx.x / 16, tx = threadIdx.x % 16;
  float acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = 0.f;

  for (int64_t k0 = r0; k0 < r1; k0 += GR_KB) {
#pragma unroll
    for (int q = 0; q < GR_KB * GR_TILE / TRS_BLOCK; ++q) {
      const int idx = threadIdx.x + TRS_BLOCK * q;
      const int kk = idx / GR_TILE, cc = idx % GR_TILE;
      const int64_t row = k0 + kk;
      const bool in = row < r1;
      As[kk][cc] = in && ci + cc < D ? Y[row * ld + ci + cc] : 0.f;
      Bs[kk][cc] = in && cj + cc < D ? Y[row * ld + cj + cc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int kk = 0; kk < GR_KB; ++kk) {
      const float4 a = *reinterpret_cast<const float4*>(&As[kk][4 * ty]);
      const float4 b = *reinterpret_cast<const float4*>(&Bs[kk][4 * tx]);
      const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = fmaf(av[i], bv[j], acc[i][j]);
    }
    __syncthreads();
  }
  float* out = part + c * (int64_t)D * D;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int row = ci + 4 * ty + i, col = cj + 4 * tx + j;
      if (row < D && col < D) out[(int64_t)row * D + col] = acc[i][j];
    }
}

__global__ __launch_bounds__(TRS_BLOCK) void als_gram_reduce_kernel(const float* __restrict__ part, int64_t chunks,
                                                                    int D, float* __restrict__ G) {
  const int e = blockIdx.x * TRS_BLOCK + threadIdx.x;
  if (e >= D * D) return;
  float s = 0.f;
  for (int64_t c = 0; c < chunks; ++c) s += part[c * (int64_t)D * D + e];
  G[e] = s;
}

// ---------------------------------------------------------------------------------------------------- solve
struct AlsArgs {
  const float* Y;  // (n_other, D) the frozen table
  int64_t n_other;
  const float* G;  // (D, D)
  const int64_t* off;
  const int32_t* nbr;
  float lambda, alpha;
  int steps, D;
  float* X;  // (n_rows, D)
  int64_t n_rows;
  int32_t* err;  // or NULL
};

__device__ __forceinline__ float als_dot4(const float4& a, const float4& b) {
  float d = a.x * b.x;
  d += a.y * b.y;
  d += a.z * b.z;
  d += a.w * b.w;
  return d;
}

template <int G, bool GLDS>
constexpr int als_block() {
  return GLDS && G == 32 ? 1024 : TRS_BLOCK;  // 64 KiB of G per workgroup: two workgroups of 16 waves fill a CU
}

template <int G, bool VEC, bool GLDS>
__global__ __launch_bounds__((als_block<G, GLDS>())) void als_solve_kernel(const AlsArgs a) {
  constexpr int Dp = 4 * G;
  constexpr int BLOCK = als_block<G, GLDS>();
  constexpr int ROWS = BLOCK / G;  // rows per tile
  __shared__ __attribute__((aligned(16))) float Gs[GLDS ? Dp * Dp : 4];
  const int D = a.D;
  const int l = threadIdx.x & (G - 1);
  const int d0 = 4 * l;
  const float lambda = a.lambda, alpha = a.alpha;
  const float one_alpha = 1.0f + alpha;

  if constexpr (GLDS) {
    for (int idx = threadIdx.x; idx < Dp * Dp; idx += BLOCK) {
      const int r = idx / Dp, c = idx % Dp;
      Gs[idx] = r < D && c < D ? a.G[(int64_t)r * D + c] : 0.f;
    }
    __syncthreads();
  }

  // this lane's four columns of row `row` (a valid row) of a table with row stride D, columns >= D as 0
  auto row4 = [&](const float* base, int64_t row) __attribute__((always_inline)) {
    const float* p = base + row * (int64_t)D;
    float4 x;
    if constexpr (VEC) {
      const bool in = d0 < D;  // D % 4 == 0: a lane's four columns are inside together
      x = *reinterpret_cast<const float4*>(p + (in ? d0 : 0));
      if (!in) x = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const float x0 = p[d0 < D ? d0 : 0], x1 = p[d0 + 1 < D ? d0 + 1 : 0];
      const float x2 = p[d0 + 2 < D ? d0 + 2 : 0], x3 = p[d0 + 3 < D ? d0 + 3 : 0];
      x = make_float4(d0 < D ? x0 : 0.f, d0 + 1 < D ? x1 : 0.f, d0 + 2 < D ? x2 : 0.f, d0 + 3 < D ? x3 : 0.f);
    }
    return x;
  };

  // columns 4l .. 4l+3 of G v: sum over e ascending, from 0
  auto gmul = [&](const float4& v) __attribute__((always_inline)) {
    float4 o = make_float4(0.f, 0.f, 0.f, 0.f);
    for (int e4 = 0; 4 * e4 < D; ++e4) {
      const float ve[4] = {__shfl(v.x, e4, G), __shfl(v.y, e4, G), __shfl(v.z, e4, G), __shfl(v.w, e4, G)};
#pragma unroll
      for (int c = 0; c < 4; ++c) {
        const int e = 4 * e4 + c;
        if (e < D) {  // (uniform)
          float4 g;
          if constexpr (GLDS)
            g = *reinterpret_cast<const float4*>(&Gs[e * Dp + d0]);
          else
            g = row4(a.G, e);
          o.x += g.x * ve[c];
          o.y += g.y * ve[c];
          o.z += g.z * ve[c];
          o.w += g.w * ve[c];
        }
      }
    }
    return o;
  };

  const int64_t n_tiles = (a.n_rows + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t h = tile * ROWS + threadIdx.x / G;
    const bool live = h < a.n_rows;
    int64_t off0 = 0, n_h = 0;
    if (live) {
      off0 = a.off[h];
      n_h = a.off[h + 1] - off0;
      if (n_h < 0) n_h = 0;
    }
    long long nmax = n_h;  // the longest list of the wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const long long other = __shfl_xor(nmax, o, 64);
      nmax = other > nmax ? other : nmax;
    }

    // acc = sum_{i in N} (y_i . v) y_i in CSR order; with_s: also s = sum_{i in N} y_i
    auto walk = [&](const float4& v, const bool with_s, float4& acc, float4& s) __attribute__((always_inline)) {
      acc = make_float4(0.f, 0.f, 0.f, 0.f);
      int cur = -1, nxt = -1;  // this lane's entry of the id chunk in use / of the one after: -1 = no neighbour
      // lane l: neighbour base + l of its row (base wave-uniform, a multiple of G)
      auto chunk = [&](long long base) __attribute__((always_inline)) {
        int id = -1;
        if (base < nmax) {  // (uniform) some row of the wave has a neighbour there, so the CSR holds one entry at least
          const long long mv = base + l;
          const bool has = mv < n_h;
          const int32_t t = a.nbr[has ? off0 + mv : 0];
          const bool in = (uint64_t)(int64_t)t < (uint64_t)a.n_other;
          if (has && in) id = t;
          if (has && !in && a.err) atomicOr(a.err, 1);  // never an address: the neighbour is skipped
        }
        return id;
      };
      float4 ring[ALS_DEPTH];
      bool ok[ALS_DEPTH];
      auto fetch = [&](long long vi, float4& q, bool& good) __attribute__((always_inline)) {
        if ((vi & (G - 1)) == 0) {
          cur = nxt;
          nxt = chunk(vi + G);
        }
        const int id = __shfl(cur, (int)(vi & (G - 1)), G);
        good = id >= 0;
        q = row4(a.Y, good ? id : 0);
      };
      nxt = chunk(0);
#pragma unroll
      for (int k = 0; k < ALS_DEPTH; ++k) fetch(k, ring[k], ok[k]);
      for (long long j = 0; j < nmax; j += ALS_DEPTH) {
#pragma unroll
        for (int k = 0; k < ALS_DEPTH; ++k) {
          const float4 y = ring[k];
          const bool good = ok[k];
          fetch(j + k + ALS_DEPTH, ring[k], ok[k]);
          const float d = trs_group_sum<G>(als_dot4(y, v));
          if (good) {
            acc.x += d * y.x;
            acc.y += d * y.y;
            acc.z += d * y.z;
            acc.w += d * y.w;
            if (with_s) {
              s.x += y.x;
              s.y += y.y;
              s.z += y.z;
              s.w += y.w;
            }
          }
        }
      }
    };

    // A v = (G v + lambda v) + alpha sum_{i in N} (y_i . v) y_i
    auto amul = [&](const float4& v, const bool with_s, float4& s) __attribute__((always_inline)) {
      const float4 g = gmul(v);
      float4 acc;
      walk(v, with_s, acc, s);
      return make_float4((g.x + lambda * v.x) + alpha * acc.x, (g.y + lambda * v.y) + alpha * acc.y,
                         (g.z + lambda * v.z) + alpha * acc.z, (g.w + lambda * v.w) + alpha * acc.w);
    };

    float4 x = row4(a.X, live ? h : 0);  // row 0 is always there (n_rows >= 1)
    float4 s = make_float4(0.f, 0.f, 0.f, 0.f);
    const float4 ax = amul(x, true, s);
    float4 r = make_float4(one_alpha * s.x - ax.x, one_alpha * s.y - ax.y, one_alpha * s.z - ax.z,
                           one_alpha * s.w - ax.w);
    float4 p = r;
    float rho = trs_group_sum<G>(als_dot4(r, r));
    bool active = live && n_h > 0 && !(rho < ALS_RHO_STOP);
    if (n_h == 0) x = make_float4(0.f, 0.f, 0.f, 0.f);  // an empty list: the row is exactly 0

    for (int k = 0; k < a.steps; ++k) {
      if (!__any(active)) break;  // (wave-uniform)
      const float4 ap = amul(p, false, s);
      const float pap = trs_group_sum<G>(als_dot4(p, ap));
      const float step = rho / pap;
      float4 rn = r;
      if (active) {
        x.x += step * p.x;
        x.y += step * p.y;
        x.z += step * p.z;
        x.w += step * p.w;
        rn = make_float4(r.x - step * ap.x, r.y - step * ap.y, r.z - step * ap.z, r.w - step * ap.w);
      }
      const float rho2 = trs_group_sum<G>(als_dot4(rn, rn));
      if (active) {
        r = rn;
        if (rho2 < ALS_RHO_STOP) {
          active = false;
        } else {
          const float beta = rho2 / rho;
          p = make_float4(r.x + beta * p.x, r.y + beta * p.y, r.z + beta * p.z, r.w + beta * p.w);
          rho = rho2;
        }
      }
    }

    if (live) {
      float* row = a.X + h * (int64_t)D + d0;
      if (VEC) {
        if (d0 < D) *reinterpret_cast<float4*>(row) = x;
      } else if (d0 < D) {
        row[0] = x.x;
        if (d0 + 1 < D) row[1] = x.y;
        if (d0 + 2 < D) row[2] = x.z;
        if (d0 + 3 < D) row[3] = x.w;
      }
    }
  }
}

template <int G, bool VEC, bool GLDS>
static void launch_als(const AlsArgs& a, hipStream_t s) {
  constexpr int BLOCK = als_block<G, GLDS>();
  const int64_t n_tiles = (a.n_rows + BLOCK / G - 1) / (BLOCK / G);
  const int64_t cap = 256 * (2048 / BLOCK);  // 256 CUs x the workgroups that fit one at 32 waves
  const unsigned blocks = (unsigned)(n_tiles < cap ? n_tiles : cap);
  hipLaunchKernelGGL((als_solve_kernel<G, VEC, GLDS>), dim3(blocks), dim3(BLOCK), 0, s, a);
}
template <bool VEC>
static void launch_als_g(int G, const AlsArgs& a, hipStream_t s) {
  switch (G) {
    case 4: launch_als<4, VEC, true>(a, s); break;
    case 8: launch_als<8, VEC, true>(a, s); break;
    case 16: launch_als<16, VEC, true>(a, s); break;
    case 32: launch_als<32, VEC, true>(a, s); break;
    default: launch_als<64, VEC, false>(a, s); break;
  }
}

}  // namespace

extern "C" int64_t trs_als_gram_workspace_bytes(int64_t n, int32_t D) {
  if (n < 0 || D < 1 || D > TRS_RETRIEVE_DMAX) return 0;
  return gram_chunks(n, D) * (int64_t)D * D * 4;
}

extern "C" int trs_als_gram(const float* rows_dev, int64_t n, int32_t D, int64_t ld, float* G_out_dev,
                            void* workspace_dev, void* stream) {
  const char* who = "trs_als_gram";
  TRS_REQUIRE(D >= 1 && D <= TRS_RETRIEVE_DMAX, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(n >= 0 && n <= INT32_MAX, "%s: n=%lld outside 0..2^31-1", who, (long long)n);
  TRS_REQUIRE(ld >= D, "%s: ld=%lld is below D=%d", who, (long long)ld, D);
  TRS_REQUIRE(G_out_dev != nullptr, "%s: G_out is NULL", who);
  TRS_REQUIRE(n == 0 || (rows_dev && workspace_dev), "%s: rows / workspace is NULL with n > 0", who);
  hipStream_t s = (hipStream_t)stream;
  const int64_t chunks = gram_chunks(n, D);
  const unsigned tiles = (unsigned)((D + GR_TILE - 1) / GR_TILE);
  if (chunks > 0) {
    hipLaunchKernelGGL(als_gram_partial_kernel, dim3((unsigned)chunks, tiles, tiles), dim3(TRS_BLOCK), 0, s, rows_dev,
                       n, (int)D, ld, gram_chunk_rows(n, D), (float*)workspace_dev);
    TRS_CHECK_LAUNCH("als_gram_partial_kernel");
  }
  hipLaunchKernelGGL(als_gram_reduce_kernel, dim3((unsigned)((D * D + TRS_BLOCK - 1) / TRS_BLOCK)), dim3(TRS_BLOCK), 0,
                     s, (const float*)workspace_dev, chunks, (int)D, G_out_dev);
  TRS_CHECK_LAUNCH("als_gram_reduce_kernel");
  return TRS_OK;
}

extern "C" int trs_als_solve(const float* other_rows_dev, int64_t n_other, int32_t D, const float* G_dev,
                             const trs_csr* nbr, float lambda, float alpha, int32_t cg_steps, float* rows_inout_dev,
                             int64_t n_rows, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_als_solve";
  TRS_REQUIRE(D >= 1 && D <= TRS_RETRIEVE_DMAX, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(cg_steps >= 1 && cg_steps <= 256, "%s: cg_steps=%d outside 1..256", who, cg_steps);
  TRS_REQUIRE(lambda > 0.f && lambda <= 3.402823466e+38f, "%s: lambda must be finite and > 0", who);
  TRS_REQUIRE(alpha >= 0.f && alpha <= 3.402823466e+38f, "%s: alpha must be finite and >= 0", who);
  TRS_REQUIRE(n_rows >= 0, "%s: n_rows=%lld is negative", who, (long long)n_rows);
  if (n_rows == 0) return TRS_OK;
  TRS_REQUIRE(n_other >= 1 && n_other <= INT32_MAX, "%s: n_other=%lld outside 1..2^31-1", who, (long long)n_other);
  TRS_REQUIRE(other_rows_dev && G_dev && rows_inout_dev, "%s: other_rows / G / rows_inout is NULL", who);
  TRS_REQUIRE(nbr != nullptr && nbr->off && nbr->items, "%s: neighbour CSR is NULL or has NULL arrays", who);
  TRS_REQUIRE(nbr->n_rows == n_rows, "%s: neighbour CSR has %lld rows for n_rows=%lld", who, (long long)nbr->n_rows,
              (long long)n_rows);
  TRS_REQUIRE(n_rows < ((int64_t)1 << 40), "%s: too many rows in one call", who);

  AlsArgs a = {};
  a.Y = other_rows_dev;
  a.n_other = n_other;
  a.G = G_dev;
  a.off = nbr->off;
  a.nbr = nbr->items;
  a.lambda = lambda;
  a.alpha = alpha;
  a.steps = cg_steps;
  a.D = D;
  a.X = rows_inout_dev;
  a.n_rows = n_rows;
  a.err = err_flag_dev;
  int Dp = 16;
  while (Dp < D) Dp <<= 1;
  const bool vec = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(a.Y) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.X) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.G) & 15) == 0;
  if (vec)
    launch_als_g<true>(Dp / 4, a, (hipStream_t)stream);
  else
    launch_als_g<false>(Dp / 4, a, (hipStream_t)stream);
  TRS_CHECK_LAUNCH("als_solve_kernel");
  return TRS_OK;
}
