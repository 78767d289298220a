// softmax.hip — in-batch softmax training loss of the Linear / FM scorers (model.py fit(loss='softmax'); math in
// include/trs.h "in-batch softmax", design in DESIGN.md §4.6).
//
// The logits of a batch are one inner product plus a per-column constant: z_ij = <U_ui, S_pj> + c_pj (+ a per-row
// constant that cancels in the row softmax).  The matrix work runs on trs_gemm_f32, driven chunk by chunk from the host
// (torchrecsys_amd/ops.py InBatchSoftmax); the three kernels here do everything else:
//
// softmax_stage_kernel  one wave per batch position j: query row Q_j = user row (+ a ones column at Dp), key row
//                       K_j = S_pj = item + sum of metadata rows, the column constant cc_j = c_pj / tau - L_j, the
//                       position's item id for the accidental-hit mask.  Ids are range-checked into err bit 0.
// softmax_rows_kernel   one workgroup per logit row i of a chunk: zh_ij = z_ij / tau + cc_j, accidental hits -> -inf,
//                       online max / sum of exponentials, lse, loss_i = lse - zh_ii, then G_ij = (P_ij - [i == j]) / B
//                       written over the logits (P = row softmax).  Fixed thread order: bit-identical from run to run.
// softmax_grads_kernel  one wave per batch position: the chain rule from dQ = G K, dK = G^T Q (its ones column gives
//                       dc_j = sum_i G_ij) into per-field gradient rows; workgroup 0 adds the row losses in a fixed order.
#include "trs_common.h"

namespace {

constexpr int SM_PAD = 4;  // Dq = Dp + SM_PAD: the ones column of Q, rows 16-byte aligned

static inline int sm_dp(int D) {
  int p = 16;
  while (p < D) p <<= 1;
  return p;
}
static inline int64_t sm_blk(int64_t n) { return (n + 63) / 64 * 64; }  // 256-byte aligned blocks of 4-byte words

// Workspace layout (4-byte words): Q, K, dQ, dK (B, Dq) fp32 | cc (B) fp32 | row losses (B) fp32 | item ids (B) int32.
struct SmLayout {
  int Dp, Dq;
  int64_t q, k, dq, dk, cc, loss, pid, words;
};
static inline SmLayout sm_layout(int64_t B, int D) {
  SmLayout L;
  L.Dp = sm_dp(D);
  L.Dq = L.Dp + SM_PAD;
  const int64_t mat = sm_blk(B * L.Dq), vec = sm_blk(B);
  L.q = 0;
  L.k = mat;
  L.dq = 2 * mat;
  L.dk = 3 * mat;
  L.cc = 4 * mat;
  L.loss = L.cc + vec;
  L.pid = L.loss + vec;
  L.words = L.pid + vec;
  return L;
}

struct StageArgs {
  trs_tables T;
  trs_batch Bt;
  int net, Dp, Dq;
  float inv_tau;
  const float* logq;  // (n_items) log q of each item, or NULL
  float *Q, *K, *cc;
  int32_t* pid;
};

__global__ __launch_bounds__(TRS_BLOCK) void softmax_stage_kernel(const StageArgs a) {
  const int lane = threadIdx.x & 63;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const trs_tables& T = a.T;
  const int M = T.M, D = T.D;
  for (int64_t j = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6; j < a.Bt.B; j += nwave) {
    const int64_t u = trs_ld_idx(a.Bt.user, a.Bt.idx_bytes, j);
    const int64_t p = trs_ld_idx(a.Bt.pos, a.Bt.idx_bytes, j);
    const bool uok = (uint64_t)u < (uint64_t)T.n_users, pok = (uint64_t)p < (uint64_t)T.n_items;
    bool bad = !uok || !pok;
    int64_t mid[TRS_MAX_META];
    for (int m = 0; m < M; ++m) {
      mid[m] = trs_ld_idx(a.Bt.pos_meta, a.Bt.idx_bytes, j * M + m);
      if ((uint64_t)mid[m] >= (uint64_t)T.n_meta[m]) {
        bad = true;
        mid[m] = -1;  // skipped below
      }
    }
    if (bad && lane == 0 && a.Bt.err_flag_dev) atomicOr(a.Bt.err_flag_dev, 1);
    float part = 0.f;  // FM: sum_d (S_d^2 - item_d^2 - sum_m meta_md^2)
    for (int d = lane; d < a.Dq; d += 64) {
      float q = d == a.Dp ? 1.f : 0.f, s = 0.f, sq = 0.f;
      if (d < D) {
        if (uok) q = T.user[u * D + d];
        if (pok) {
          const float v = T.item[p * D + d];
          s = v;
          sq = v * v;
          for (int m = 0; m < M; ++m) {
            if (mid[m] < 0) continue;
            const float x = T.meta[m][mid[m] * D + d];
            s += x;
            sq += x * x;
          }
        }
      }
      a.Q[j * a.Dq + d] = q;
      a.K[j * a.Dq + d] = s;
      part += s * s - sq;
    }
    if (a.net == TRS_NET_FM) part = trs_wave_sum(part);
    if (lane == 0) {
      float c = 0.f, L = 0.f;
      if (pok) {
        c = T.item_lin[p];
        if (a.net == TRS_NET_FM) {
          for (int m = 0; m < M; ++m)
            if (mid[m] >= 0) c += T.meta_lin[m][mid[m]];
          c += 0.5f * part;
        }
        if (a.logq) L = a.logq[p];
      }
      a.cc[j] = c * a.inv_tau - L;
      a.pid[j] = pok ? (int32_t)p : -1;
    }
  }
}

struct RowsArgs {
  float* Z;  // (n_rows, B) logits of rows row0 .. row0 + n_rows - 1, overwritten by G
  int64_t row0, n_rows, B;
  float inv_tau, inv_B;
  const float* cc;
  const int32_t* pid;
  float* loss;
};

// running (max, sum of exp(x - max)) of a thread's share of a row; m = -inf: nothing seen yet
__device__ __forceinline__ void sm_push(float& m, float& s, float x) {
  if (x > m) {
    s = s * expf(m - x) + 1.f;
    m = x;
  } else {
    s += expf(x - m);
  }
}
__device__ __forceinline__ void sm_merge(float& m, float& s, float m2, float s2) {
  const float mx = fmaxf(m, m2);
  if (mx == -INFINITY) return;  // both empty
  s = s * expf(m - mx) + s2 * expf(m2 - mx);
  m = mx;
}

template <bool VEC>
__global__ __launch_bounds__(TRS_BLOCK) void softmax_rows_kernel(const RowsArgs a) {
  __shared__ float red_m[TRS_BLOCK / 64], red_s[TRS_BLOCK / 64];
  const int tid = threadIdx.x, lane = tid & 63, wid = tid >> 6;
  const int64_t B = a.B;
  for (int64_t r = blockIdx.x; r < a.n_rows; r += gridDim.x) {
    const int64_t i = a.row0 + r;
    float* __restrict__ z = a.Z + r * B;
    const int32_t pi = a.pid[i];
    float m = -INFINITY, s = 0.f;
    if (VEC) {
      for (int64_t j = 4 * (int64_t)tid; j < B; j += 4 * TRS_BLOCK) {
        const float4 v = *(const float4*)(z + j);
        const float4 c = *(const float4*)(a.cc + j);
        const int4 q = *(const int4*)(a.pid + j);
        const float x[4] = {v.x, v.y, v.z, v.w}, cv[4] = {c.x, c.y, c.z, c.w};
        const int32_t id[4] = {q.x, q.y, q.z, q.w};
#pragma unroll
        for (int e = 0; e < 4; ++e)
          if (id[e] != pi || j + e == i) sm_push(m, s, x[e] * a.inv_tau + cv[e]);
      }
    } else {
      for (int64_t j = tid; j < B; j += TRS_BLOCK)
        if (a.pid[j] != pi || j == i) sm_push(m, s, z[j] * a.inv_tau + a.cc[j]);
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float m2 = __shfl_xor(m, o, 64), s2 = __shfl_xor(s, o, 64);
      sm_merge(m, s, m2, s2);
    }
    if (lane == 0) {
      red_m[wid] = m;
      red_s[wid] = s;
    }
    __syncthreads();
    m = red_m[0];
    s = red_s[0];
#pragma unroll
    for (int w = 1; w < TRS_BLOCK / 64; ++w) sm_merge(m, s, red_m[w], red_s[w]);
    const float lse = m + logf(s);
    if (tid == 0) a.loss[i] = lse - (z[i] * a.inv_tau + a.cc[i]);
    __syncthreads();  // z[i] was read before it is overwritten; red_* free for the next row
    if (VEC) {
      for (int64_t j = 4 * (int64_t)tid; j < B; j += 4 * TRS_BLOCK) {
        const float4 v = *(const float4*)(z + j);
        const float4 c = *(const float4*)(a.cc + j);
        const int4 q = *(const int4*)(a.pid + j);
        const float x[4] = {v.x, v.y, v.z, v.w}, cv[4] = {c.x, c.y, c.z, c.w};
        const int32_t id[4] = {q.x, q.y, q.z, q.w};
        float g[4];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float pr = (id[e] != pi || j + e == i) ? expf(x[e] * a.inv_tau + cv[e] - lse) : 0.f;
          g[e] = (pr - (j + e == i ? 1.f : 0.f)) * a.inv_B;
        }
        *(float4*)(z + j) = make_float4(g[0], g[1], g[2], g[3]);
      }
    } else {
      for (int64_t j = tid; j < B; j += TRS_BLOCK) {
        const float pr = (a.pid[j] != pi || j == i) ? expf(z[j] * a.inv_tau + a.cc[j] - lse) : 0.f;
        z[j] = (pr - (j == i ? 1.f : 0.f)) * a.inv_B;
      }
    }
  }
}

struct GradsArgs {
  trs_tables T;
  trs_batch Bt;
  int net, Dp, Dq;
  float inv_tau;
  const float *K, *dQ, *dK, *rowloss;
  float* grad_rows;  // (2 + M, B, D) or NULL (loss only)
  float* grad_lin;   // (2 + M, B)
  float* loss_sum;
};

__global__ __launch_bounds__(TRS_BLOCK) void softmax_grads_kernel(const GradsArgs a) {
  const int lane = threadIdx.x & 63;
  const trs_tables& T = a.T;
  const int M = T.M, D = T.D;
  const int64_t B = a.Bt.B;
  const bool fm = a.net == TRS_NET_FM;
  if (a.grad_rows) {
    const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
    for (int64_t j = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6; j < B; j += nwave) {
      const int64_t p = trs_ld_idx(a.Bt.pos, a.Bt.idx_bytes, j);
      const bool pok = (uint64_t)p < (uint64_t)T.n_items;
      const float dc = a.dK[j * a.Dq + a.Dp] * a.inv_tau;  // ones column of Q: sum_i G_ij, times 1/tau
      const float* kj = a.K + j * a.Dq;
      float* gu = a.grad_rows + j * D;
      float* gi = a.grad_rows + (B + j) * D;
      for (int d = lane; d < D; d += 64) {
        gu[d] = a.dQ[j * a.Dq + d] * a.inv_tau;
        const float gk = a.dK[j * a.Dq + d] * a.inv_tau;
        // FM: d c_j / d item = S_j - item_j (an out-of-range id was staged as a zero row: no gradient)
        gi[d] = fm ? (pok ? gk + dc * (kj[d] - T.item[p * D + d]) : 0.f) : gk;
        for (int m = 0; m < M; ++m) {
          const int64_t mid = trs_ld_idx(a.Bt.pos_meta, a.Bt.idx_bytes, j * M + m);
          const bool mok = pok && (uint64_t)mid < (uint64_t)T.n_meta[m];
          a.grad_rows[((2 + m) * B + j) * D + d] = fm ? (mok ? gk + dc * (kj[d] - T.meta[m][mid * D + d]) : 0.f) : gk;
        }
      }
      if (lane == 0) {
        a.grad_lin[j] = 0.f;  // per-row constants cancel in the row softmax
        a.grad_lin[B + j] = dc;
        for (int m = 0; m < M; ++m) a.grad_lin[(2 + m) * B + j] = fm ? dc : 0.f;
      }
    }
  }
  if (blockIdx.x == 0) {  // loss_sum += sum_i loss_i, one fixed order
    __shared__ float part[TRS_BLOCK];
    float s = 0.f;
    for (int64_t i = threadIdx.x; i < B; i += TRS_BLOCK) s += a.rowloss[i];
    part[threadIdx.x] = s;
    __syncthreads();
    for (int w = TRS_BLOCK / 2; w > 0; w >>= 1) {
      if ((int)threadIdx.x < w) part[threadIdx.x] += part[threadIdx.x + w];
      __syncthreads();
    }
    if (threadIdx.x == 0) *a.loss_sum += part[0];
  }
}

// shared argument checks of the three entry points
static int sm_check_common(const char* who, int64_t B, int32_t D, float tau, const void* ws, int64_t ws_bytes) {
  TRS_REQUIRE(B >= 1, "%s: B=%lld < 1", who, (long long)B);
  TRS_REQUIRE(D >= 1, "%s: D=%d < 1", who, (int)D);
  TRS_REQUIRE(tau > 0.f && tau < INFINITY, "%s: temperature %g must be positive and finite", who, (double)tau);
  TRS_REQUIRE(ws != nullptr, "%s: workspace is NULL", who);
  const int64_t need = trs_softmax_workspace_bytes(B, D);
  TRS_REQUIRE(ws_bytes >= need, "%s: workspace too small (%lld < %lld)", who, (long long)ws_bytes, (long long)need);
  return TRS_OK;
}

// need_ids: the kernel reads the tables and the batch's ids (softmax: no 1-wide user table — it cancels in every
// row — and item ids that fit the int32 id column of the workspace)
static int sm_check_tables(const char* who, int net, const trs_tables* T, const trs_batch* b, bool need_ids) {
  TRS_TRY(need_ids ? trs_check_tables(who, net, T, TRS_SKIP_USER_LIN, INT32_MAX) : trs_check_net(who, net, T));
  TRS_REQUIRE(b != nullptr, "%s: batch is NULL", who);
  TRS_REQUIRE(b->idx_bytes == 4 || b->idx_bytes == 8, "%s: idx_bytes must be 4 or 8", who);
  if (!need_ids) return TRS_OK;
  TRS_REQUIRE(b->user && b->pos, "%s: user/pos ids are NULL", who);
  TRS_REQUIRE(T->M == 0 || b->pos_meta, "%s: pos_meta ids are NULL but M=%d", who, T->M);
  return TRS_OK;
}

}  // namespace

extern "C" int64_t trs_softmax_workspace_bytes(int64_t B, int32_t D) {
  if (B < 1 || D < 1) return 0;
  return sm_layout(B, D).words * 4;
}

extern "C" int trs_softmax_stage(int net, const trs_tables* tables, const trs_batch* batch, float tau,
                                 const float* logq_dev, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const char* who = "trs_softmax_stage";
  TRS_TRY(sm_check_tables(who, net, tables, batch, true));
  TRS_TRY(sm_check_common(who, batch->B, tables->D, tau, workspace_dev, workspace_bytes));
  const SmLayout L = sm_layout(batch->B, tables->D);
  float* w = (float*)workspace_dev;
  StageArgs a;
  a.T = *tables;
  a.Bt = *batch;
  a.net = net;
  a.Dp = L.Dp;
  a.Dq = L.Dq;
  a.inv_tau = 1.f / tau;
  a.logq = logq_dev;
  a.Q = w + L.q;
  a.K = w + L.k;
  a.cc = w + L.cc;
  a.pid = (int32_t*)(w + L.pid);
  hipLaunchKernelGGL(softmax_stage_kernel, dim3(trs_grid(batch->B, TRS_BLOCK / 64)), dim3(TRS_BLOCK), 0,
                     (hipStream_t)stream, a);
  TRS_CHECK_LAUNCH("softmax_stage_kernel");
  return TRS_OK;
}

extern "C" int trs_softmax_rows(float* z_dev, int64_t z_bytes, int64_t row0, int64_t n_rows, int64_t B, int32_t D,
                                float tau, void* workspace_dev, int64_t workspace_bytes, void* stream) {
  const char* who = "trs_softmax_rows";
  TRS_TRY(sm_check_common(who, B, D, tau, workspace_dev, workspace_bytes));
  TRS_REQUIRE(z_dev != nullptr, "%s: logits are NULL", who);
  TRS_REQUIRE(row0 >= 0 && n_rows >= 1 && row0 + n_rows <= B, "%s: rows [%lld, %lld) outside [0, %lld)", who,
              (long long)row0, (long long)(row0 + n_rows), (long long)B);
  TRS_REQUIRE(z_bytes >= n_rows * B * 4, "%s: logit buffer too small (%lld < %lld)", who, (long long)z_bytes,
              (long long)(n_rows * B * 4));
  const SmLayout L = sm_layout(B, D);
  float* w = (float*)workspace_dev;
  RowsArgs a;
  a.Z = z_dev;
  a.row0 = row0;
  a.n_rows = n_rows;
  a.B = B;
  a.inv_tau = 1.f / tau;
  a.inv_B = 1.f / (float)B;
  a.cc = w + L.cc;
  a.pid = (const int32_t*)(w + L.pid);
  a.loss = w + L.loss;
  const dim3 grid((unsigned)(n_rows < 65536 ? n_rows : 65536));
  if (B % 4 == 0 && ((uintptr_t)z_dev & 15) == 0)
    hipLaunchKernelGGL(softmax_rows_kernel<true>, grid, dim3(TRS_BLOCK), 0, (hipStream_t)stream, a);
  else
    hipLaunchKernelGGL(softmax_rows_kernel<false>, grid, dim3(TRS_BLOCK), 0, (hipStream_t)stream, a);
  TRS_CHECK_LAUNCH("softmax_rows_kernel");
  return TRS_OK;
}

extern "C" int trs_softmax_grads(int net, const trs_tables* tables, const trs_batch* batch, float tau,
                                 const void* workspace_dev, int64_t workspace_bytes, float* grad_rows_dev,
                                 float* grad_lin_dev, float* loss_sum_dev, void* stream) {
  const char* who = "trs_softmax_grads";
  const bool grads = grad_rows_dev || grad_lin_dev;
  TRS_TRY(sm_check_tables(who, net, tables, batch, grads));
  TRS_TRY(sm_check_common(who, batch->B, tables->D, tau, workspace_dev, workspace_bytes));
  TRS_REQUIRE(loss_sum_dev != nullptr, "%s: loss_sum is NULL", who);
  TRS_REQUIRE(!grads || (grad_rows_dev && grad_lin_dev), "%s: grad_rows and grad_lin must both be given or both NULL",
              who);
  const SmLayout L = sm_layout(batch->B, tables->D);
  const float* w = (const float*)workspace_dev;
  GradsArgs a;
  a.T = *tables;
  a.Bt = *batch;
  a.net = net;
  a.Dp = L.Dp;
  a.Dq = L.Dq;
  a.inv_tau = 1.f / tau;
  a.K = w + L.k;
  a.dQ = w + L.dq;
  a.dK = w + L.dk;
  a.rowloss = w + L.loss;
  a.grad_rows = grad_rows_dev;
  a.grad_lin = grad_lin_dev;
  a.loss_sum = loss_sum_dev;
  const int grid = grads ? trs_grid(batch->B, TRS_BLOCK / 64) : 1;
  hipLaunchKernelGGL(softmax_grads_kernel, dim3(grid), dim3(TRS_BLOCK), 0, (hipStream_t)stream, a);
  TRS_CHECK_LAUNCH("softmax_grads_kernel");
  return TRS_OK;
}
