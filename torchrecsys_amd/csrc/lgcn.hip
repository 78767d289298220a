// lgcn.hip — LightGCN (model.py fit_lightgcn; the rule is the contract in include/trs.h "LightGCN", the design in
// DESIGN.md 4.19): the degree-normalised neighbour sum that the Horner forward and backward are built from, and the
// dense Adam rule of its gradient.
//
// lgcn_propagate_kernel<G, VEC>  one output row per aligned lane group of G = Dp / 4 lanes (Dp = D rounded up to a power
//                           of two >= 16), as als_solve_kernel: lane l keeps columns 4l .. 4l+3 of the sum in registers.
//                           A workgroup takes tiles of BLOCK / G rows in a grid-stride loop; the grid is capped at 2048
//                           workgroups, of which 1024 are resident at once (128 VGPRs: 4 workgroups per CU).
//   walk       one segment's partial sum_c dinv_in[c] * in[c] in CSR order.  LGCN_DEPTH rows are kept requested in a
//              ring of registers: there is no arithmetic to hide behind, the kernel lives on loads in flight.  The ids
//              of G neighbours are loaded by the G lanes at once TWO chunks ahead and their dinv_in ONE chunk ahead (a
//              gather that depends on the ids: a chunk's distance keeps it off the ring's critical path); both are
//              handed out by shuffle.  No branch around a row load: a slot that is off reads row 0 and is dropped by a
//              select.  Every lane of a wave runs to the wave's longest segment with its sums predicated off.
//   short rows a list of at most TRS_LGCN_SEG neighbours is one segment: its lane group walks it and writes the row.
//   long rows  are left out of the lane-group pass (length 0, nothing written) and then taken one at a time by the WHOLE
//              workgroup: its BLOCK / G lane groups walk BLOCK / G consecutive segments at once, park the partials in
//              LDS, and every lane adds them to s in ascending segment order — the sum the rule pins, whatever the
//              schedule.  A row of 50 000 neighbours costs its workgroup about six tiles of average rows, not one lane
//              group the whole launch.
// lgcn_adam_kernel          torch.optim.Adam's rule on every element of a table, grid-stride, 16-byte lanes.
#include <math.h>

#include "trs_common.h"

namespace {

constexpr int LGCN_DEPTH = 8;         // neighbour rows kept requested per lane group, 16-byte lanes
constexpr int LGCN_DEPTH_SMALL = 4;  // ... on the scalar path (four loads per row and lane) and for rows of 64 bytes
constexpr int LGCN_SEG = TRS_LGCN_SEG;

struct LgcnArgs {
  const float* in;  // (n_in, D)
  int64_t n_in;
  const int64_t* off;
  const int32_t* nbr;
  const float* dinv_out;  // (n_out)
  const float* dinv_in;   // (n_in)
  const float* add;       // (n_out, D) or NULL
  float scale;
  float* out;  // (n_out, D)
  int64_t n_out;
  int accumulate, D;
  int32_t* err;  // or NULL
};

template <int G, bool VEC>
__global__ __launch_bounds__(TRS_BLOCK) __attribute__((amdgpu_waves_per_eu(4)))  // at most 128 VGPRs
void lgcn_propagate_kernel(const LgcnArgs a) {
  constexpr int DEPTH = VEC && G > 4 ? LGCN_DEPTH : LGCN_DEPTH_SMALL;
  constexpr int ROWS = TRS_BLOCK / G;  // rows per tile = lane groups per workgroup
  __shared__ __attribute__((aligned(16))) float4 part[TRS_BLOCK];  // a round's partials: lane l of group g at g * G + l
  __shared__ int is_long[ROWS];
  const int D = a.D;
  const int l = threadIdx.x & (G - 1);
  const int grp = threadIdx.x / G;
  const int d0 = 4 * l;

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

  // the partial of the segment nbr[start .. start + len) of this lane group: sum of dinv_in[c] * in[c] in CSR order,
  // from 0 (len == 0: nothing is read for this group)
  auto walk = [&](const int64_t start, const int len) __attribute__((always_inline)) {  // len <= TRS_LGCN_SEG
    int nmax = len;  // the longest segment of the wave
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const int other = __shfl_xor(nmax, o, 64);
      nmax = other > nmax ? other : nmax;
    }
    float4 acc = make_float4(0.f, 0.f, 0.f, 0.f);
    bool bad = false;  // this lane met an id outside [0, n_in)
    // lane l: neighbour base + l of its segment (base wave-uniform, a multiple of G); -1 = no neighbour
    auto ids = [&](int base) __attribute__((always_inline)) {
      int id = -1;
      if (base < nmax) {  // (uniform) some group of the wave has a neighbour there, so the CSR holds one entry at least
        const int mv = base + l;
        const bool has = mv < len;
        const int32_t t = a.nbr[has ? start + mv : 0];
        const bool in = (uint64_t)(int64_t)t < (uint64_t)a.n_in;
        if (has && in) id = t;
        bad |= has && !in;  // never an address: the neighbour is skipped
      }
      return id;
    };
    auto weight = [&](int id) __attribute__((always_inline)) { return a.dinv_in[id >= 0 ? id : 0]; };
    int id_cur = -1, id_nxt = ids(0), id_far = ids(G);
    float w_cur = 0.f, w_nxt = weight(id_nxt);
    float4 ring[DEPTH];
    float wr[DEPTH];
    bool ok[DEPTH];
    auto fetch = [&](int vi, float4& q, float& w, bool& good) __attribute__((always_inline)) {
      if ((vi & (G - 1)) == 0) {
        id_cur = id_nxt;
        w_cur = w_nxt;
        id_nxt = id_far;
        w_nxt = weight(id_nxt);
        id_far = ids(vi + 2 * G);
      }
      const int id = __shfl(id_cur, vi & (G - 1), G);
      w = __shfl(w_cur, vi & (G - 1), G);
      good = id >= 0;
      q = row4(a.in, good ? id : 0);
    };
#pragma unroll
    for (int k = 0; k < DEPTH; ++k) fetch(k, ring[k], wr[k], ok[k]);
    for (int j = 0; j < nmax; j += DEPTH) {
#pragma unroll
      for (int k = 0; k < DEPTH; ++k) {
        const float4 y = ring[k];
        const float w = wr[k];
        const bool good = ok[k];
        fetch(j + k + DEPTH, ring[k], wr[k], ok[k]);
        if (good) {
          acc.x += w * y.x;
          acc.y += w * y.y;
          acc.z += w * y.z;
          acc.w += w * y.w;
        }
      }
    }
    if (bad && a.err) atomicOr(a.err, 1);
    return acc;
  };

  // row h (valid) from its neighbour sum s: out = [out +] scale * ([add +] dinv_out * s)
  auto finish = [&](const int64_t h, const float4& s) __attribute__((always_inline)) {
    const float dr = a.dinv_out[h];
    float4 v = make_float4(dr * s.x, dr * s.y, dr * s.z, dr * s.w);
    if (a.add) {
      const float4 e = row4(a.add, h);
      v = make_float4(e.x + v.x, e.y + v.y, e.z + v.z, e.w + v.w);
    }
    v = make_float4(a.scale * v.x, a.scale * v.y, a.scale * v.z, a.scale * v.w);
    if (a.accumulate) {
      const float4 o = row4(a.out, h);
      v = make_float4(o.x + v.x, o.y + v.y, o.z + v.z, o.w + v.w);
    }
    float* row = a.out + h * (int64_t)D + d0;
    if (VEC) {
      if (d0 < D) *reinterpret_cast<float4*>(row) = v;
    } else if (d0 < D) {
      row[0] = v.x;
      if (d0 + 1 < D) row[1] = v.y;
      if (d0 + 2 < D) row[2] = v.z;
      if (d0 + 3 < D) row[3] = v.w;
    }
  };

  const int64_t n_tiles = (a.n_out + ROWS - 1) / ROWS;
  for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
    const int64_t h = tile * ROWS + grp;
    const bool live = h < a.n_out;
    int64_t off0 = 0, n_h = 0;
    if (live) {
      off0 = a.off[h];
      n_h = a.off[h + 1] - off0;
      if (n_h < 0) n_h = 0;
    }
    const bool lng = n_h > LGCN_SEG;
    const float4 s = walk(off0, lng ? 0 : (int)n_h);
    if (live && !lng) finish(h, s);

    if (__syncthreads_or(lng)) {  // (workgroup-uniform) the tile has a long row: the workgroup takes them one by one
      if (l == 0) is_long[grp] = lng;
      __syncthreads();
      for (int r = 0; r < ROWS; ++r) {
        if (!is_long[r]) continue;  // (workgroup-uniform)
        const int64_t hh = tile * ROWS + r;
        const int64_t o0 = a.off[hh];
        const int64_t n = a.off[hh + 1] - o0;
        const int64_t n_seg = (n + LGCN_SEG - 1) / LGCN_SEG;
        float4 t = make_float4(0.f, 0.f, 0.f, 0.f);
        for (int64_t base = 0; base < n_seg; base += ROWS) {
          const int64_t seg = base + grp;
          int len = 0;
          if (seg < n_seg) len = n - seg * LGCN_SEG < LGCN_SEG ? (int)(n - seg * LGCN_SEG) : LGCN_SEG;
          part[threadIdx.x] = walk(o0 + seg * LGCN_SEG, len);
          __syncthreads();
          const int cnt = n_seg - base < ROWS ? (int)(n_seg - base) : ROWS;
          for (int k = 0; k < cnt; ++k) {  // ascending segment order; every lane group forms the same sum
            const float4 p = part[k * G + l];
            t.x += p.x;
            t.y += p.y;
            t.z += p.z;
            t.w += p.w;
          }
          __syncthreads();
        }
        if (grp == 0) finish(hh, t);
      }
      __syncthreads();  // is_long is rewritten by the next tile
    }
  }
}

template <int G, bool VEC>
static void launch_lgcn(const LgcnArgs& a, hipStream_t s) {
  const int64_t n_tiles = (a.n_out + TRS_BLOCK / G - 1) / (TRS_BLOCK / G);
  // als_solve_kernel's cap.  At up to 128 VGPRs 16 waves = 4 workgroups fit a CU, so a full grid runs as two rounds of
  // 1024 resident workgroups, each striding over its tiles; the measurements of DESIGN.md 4.19 were taken with it.
  const int64_t cap = 256 * (2048 / TRS_BLOCK);
  const unsigned blocks = (unsigned)(n_tiles < cap ? n_tiles : cap);
  hipLaunchKernelGGL((lgcn_propagate_kernel<G, VEC>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a);
}
template <bool VEC>
static void launch_lgcn_g(int G, const LgcnArgs& a, hipStream_t s) {
  switch (G) {
    case 4: launch_lgcn<4, VEC>(a, s); break;
    case 8: launch_lgcn<8, VEC>(a, s); break;
    case 16: launch_lgcn<16, VEC>(a, s); break;
    case 32: launch_lgcn<32, VEC>(a, s); break;
    default: launch_lgcn<64, VEC>(a, s); break;
  }
}

// ---------------------------------------------------------------------------------------------------- dense Adam
struct LgcnAdamArgs {
  float* p;
  const float* g;
  float* m;
  float* v;
  int64_t n;
  float one_b1, b2, one_b2, step, bc2_sqrt, eps;
};

// torch/optim/adam.py _single_tensor_adam, operation by operation (no amsgrad, no weight decay, not maximize)
__device__ __forceinline__ void lgcn_adam_one(const LgcnAdamArgs& a, float& p, const float g, float& m, float& v) {
  m = m + a.one_b1 * (g - m);                      // exp_avg.lerp_(grad, 1 - beta1)
  v = v * a.b2 + (a.one_b2 * g) * g;               // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, value=1 - beta2)
  const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;  // (exp_avg_sq.sqrt() / bias_correction2_sqrt).add_(eps)
  p = p + (-a.step * m) / denom;                   // param.addcdiv_(exp_avg, denom, value=-step_size)
}

template <bool VEC>
__global__ __launch_bounds__(TRS_BLOCK) void lgcn_adam_kernel(const LgcnAdamArgs a) {
  const int64_t stride = (int64_t)gridDim.x * TRS_BLOCK;
  if constexpr (VEC) {
    const int64_t n4 = a.n / 4;
    for (int64_t i = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x; i < n4; i += stride) {
      float4 p = reinterpret_cast<float4*>(a.p)[i], m = reinterpret_cast<float4*>(a.m)[i];
      float4 v = reinterpret_cast<float4*>(a.v)[i];
      const float4 g = reinterpret_cast<const float4*>(a.g)[i];
      lgcn_adam_one(a, p.x, g.x, m.x, v.x);
      lgcn_adam_one(a, p.y, g.y, m.y, v.y);
      lgcn_adam_one(a, p.z, g.z, m.z, v.z);
      lgcn_adam_one(a, p.w, g.w, m.w, v.w);
      reinterpret_cast<float4*>(a.p)[i] = p;
      reinterpret_cast<float4*>(a.m)[i] = m;
      reinterpret_cast<float4*>(a.v)[i] = v;
    }
    for (int64_t i = 4 * n4 + (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x; i < a.n; i += stride)  // the last 0..3
      lgcn_adam_one(a, a.p[i], a.g[i], a.m[i], a.v[i]);
  } else {
    for (int64_t i = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x; i < a.n; i += stride)
      lgcn_adam_one(a, a.p[i], a.g[i], a.m[i], a.v[i]);
  }
}

}  // namespace

extern "C" int trs_lgcn_propagate(const float* in_rows_dev, int64_t n_in, int32_t D, const trs_csr* nbr,
                                  const float* dinv_out_dev, const float* dinv_in_dev, const float* add_rows_dev,
                                  float scale, float* out_rows_dev, int64_t n_out, int32_t accumulate,
                                  int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_lgcn_propagate";
  TRS_REQUIRE(D >= 1 && D <= TRS_RETRIEVE_DMAX, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(scale >= -3.402823466e+38f && scale <= 3.402823466e+38f, "%s: scale must be finite", who);
  TRS_REQUIRE(accumulate == 0 || accumulate == 1, "%s: accumulate=%d is not 0 or 1", who, accumulate);
  TRS_REQUIRE(n_out >= 0 && n_in >= 0, "%s: negative count (n_out=%lld, n_in=%lld)", who, (long long)n_out,
              (long long)n_in);
  TRS_REQUIRE(nbr != nullptr, "%s: neighbour CSR is NULL", who);
  TRS_REQUIRE(nbr->n_rows == n_out, "%s: neighbour CSR has %lld rows for n_out=%lld", who, (long long)nbr->n_rows,
              (long long)n_out);
  if (n_out == 0) return TRS_OK;
  TRS_REQUIRE(nbr->off && nbr->items, "%s: neighbour CSR has NULL arrays", who);
  TRS_REQUIRE(in_rows_dev && dinv_out_dev && dinv_in_dev && out_rows_dev,
              "%s: in_rows / dinv_out / dinv_in / out_rows is NULL", who);
  TRS_REQUIRE(n_in >= 1 && n_in <= INT32_MAX, "%s: n_in=%lld outside 1..2^31-1 with rows to write", who,
              (long long)n_in);
  TRS_REQUIRE(n_out < ((int64_t)1 << 40), "%s: too many rows in one call", who);
  TRS_REQUIRE((const float*)out_rows_dev != in_rows_dev, "%s: out_rows aliases in_rows", who);

  LgcnArgs a = {};
  a.in = in_rows_dev;
  a.n_in = n_in;
  a.off = nbr->off;
  a.nbr = nbr->items;
  a.dinv_out = dinv_out_dev;
  a.dinv_in = dinv_in_dev;
  a.add = add_rows_dev;
  a.scale = scale;
  a.out = out_rows_dev;
  a.n_out = n_out;
  a.accumulate = accumulate;
  a.D = D;
  a.err = err_flag_dev;
  int Dp = 16;
  while (Dp < D) Dp <<= 1;
  const bool vec = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(a.in) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.out) & 15) == 0 && (reinterpret_cast<uintptr_t>(a.add) & 15) == 0;
  if (vec)
    launch_lgcn_g<true>(Dp / 4, a, (hipStream_t)stream);
  else
    launch_lgcn_g<false>(Dp / 4, a, (hipStream_t)stream);
  TRS_CHECK_LAUNCH("lgcn_propagate_kernel");
  return TRS_OK;
}

extern "C" int trs_lgcn_adam(float* param_dev, const float* grad_dev, float* exp_avg_dev, float* exp_avg_sq_dev,
                             int64_t n, float lr, float beta1, float beta2, float eps, int64_t step_count,
                             void* stream) {
  const char* who = "trs_lgcn_adam";
  TRS_REQUIRE(n >= 0, "%s: n=%lld is negative", who, (long long)n);
  TRS_REQUIRE(step_count >= 1, "%s: step_count must be >= 1", who);
  TRS_REQUIRE(lr >= 0.f && lr <= 3.402823466e+38f, "%s: lr must be finite and >= 0", who);
  TRS_REQUIRE(beta1 >= 0.f && beta1 < 1.f && beta2 >= 0.f && beta2 < 1.f, "%s: betas must be in [0, 1)", who);
  TRS_REQUIRE(eps >= 0.f && eps <= 3.402823466e+38f, "%s: eps must be finite and >= 0", who);
  if (n == 0) return TRS_OK;
  TRS_REQUIRE(param_dev && grad_dev && exp_avg_dev && exp_avg_sq_dev, "%s: param / grad / exp_avg / exp_avg_sq is NULL",
              who);
  // 1 - beta, lr / (1 - beta1^t) and sqrt(1 - beta2^t) in double, as the Python floats of torch (trs_common.h)
  const double b1_w = trs_as_written(beta1), b2_w = trs_as_written(beta2);
  const double bc1 = 1.0 - pow(b1_w, (double)step_count);
  const double bc2 = 1.0 - pow(b2_w, (double)step_count);
  const LgcnAdamArgs a = {param_dev, grad_dev, exp_avg_dev, exp_avg_sq_dev, n, (float)(1.0 - b1_w), (float)b2_w,
                          (float)(1.0 - b2_w), (float)(trs_as_written(lr) / bc1), (float)sqrt(bc2), eps};
  const bool vec = ((reinterpret_cast<uintptr_t>(param_dev) | reinterpret_cast<uintptr_t>(grad_dev) |
                     reinterpret_cast<uintptr_t>(exp_avg_dev) | reinterpret_cast<uintptr_t>(exp_avg_sq_dev)) & 15) == 0;
  const int grid = trs_grid(n / 4 + 1, TRS_BLOCK);
  if (vec)
    hipLaunchKernelGGL(lgcn_adam_kernel<true>, dim3(grid), dim3(TRS_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(lgcn_adam_kernel<false>, dim3(grid), dim3(TRS_BLOCK), 0, (hipStream_t)stream, a);
  TRS_CHECK_LAUNCH("lgcn_adam_kernel");
  return TRS_OK;
}
