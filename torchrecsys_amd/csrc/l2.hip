// l2.hip — per-sample L2 regularisation of the embedding rows a batch references (trs_stage_add_l2; include/trs.h,
// DESIGN.md §4.10): one pass over the field-major staging buffer every per-step path fills, between the staging kernel
// and the first row update.  For every staged reference (field f, row t) of a group whose coefficient is not 0,
//   grad_rows[f, t, :] += c_group * W_pre[id, :]      and      grad_lin[f, t] += c_group * w_pre[id]
// where id is the reference's id, W the group's D-wide table and w the 1-wide table with the same ids (where it exists).
//
// l2_kernel (wave = 64): blockIdx.y is the field (so the table, its 1-wide table, its id block and the coefficient are
// wave-uniform scalars), one aligned group of G lanes per reference of the field, 16-byte lanes, grid-stride over the
// field's B references along x.  The id, the table row and the staged row are independent unconditional loads (an id
// outside its table, or a lane group past the batch, reads row 0 / reference 0 and stores nothing).  Every staged row
// has exactly one writer: no atomics but the err flag's.  No LDS, no scratch memory.
#include "score_kernels.h"

using namespace trs;

namespace {

struct L2Args {
  trs_tables T;
  const int32_t* user;   // (B)
  const int32_t* items;  // (S, B)
  const int32_t* meta;   // (S, B, M) or NULL
  int64_t B;
  int S;
  float c_user, c_item, c_meta;  // each already holds the 1/B of the mean; a group at 0 has no field in the grid
  float* grad_rows;              // (F, B, D), F = 1 + S(1+M)
  float* grad_lin;               // (F, B)
  int32_t* err;
};

template <int NET, int VEC, int G, int K>
__global__ __launch_bounds__(TRS_BLOCK) void l2_kernel(const L2Args a) {
  constexpr int N = K * VEC;
  constexpr int TPW = TRS_WAVE / G;  // references per wave per iteration
  const trs_tables& T = a.T;
  const int D = T.D;
  const int M = T.M;
  const int S = a.S;
  const int64_t B = a.B;

  // blockIdx.y counts the fields of the groups that take part, in field order: user, S item slots, M x S metadata slots
  int y = blockIdx.y;
  int f = 0;                      // the field in the staging buffer
  const float* tab = nullptr;     // its D-wide table
  const float* lin = nullptr;     // the 1-wide table with the same ids, or NULL (Linear's metadata columns have none)
  const int32_t* ids = nullptr;   // id of reference t at ids[t * id_stride]
  int id_stride = 1;
  int64_t n_rows = 0;
  float c = 0.f;
  bool found = false;
  if (a.c_user > 0.f) {
    if (y == 0) {
      found = true;
      f = 0; tab = T.user; lin = T.user_lin; ids = a.user; n_rows = T.n_users; c = a.c_user;
    }
    y -= 1;
  }
  if (!found && a.c_item > 0.f) {
    if (y < S) {
      found = true;
      f = 1 + y; tab = T.item; lin = T.item_lin; ids = a.items + (int64_t)y * B; n_rows = T.n_items; c = a.c_item;
    }
    y -= S;
  }
  if (!found) {  // (the host launched metadata fields only with c_meta > 0 and M > 0)
    const int m = y / S, s = y - m * S;
    if (m >= M) return;
    f = 1 + S + m * S + s; tab = T.meta[m]; lin = NET == TRS_NET_FM ? T.meta_lin[m] : nullptr;
    ids = a.meta + (int64_t)s * B * M + m; id_stride = M; n_rows = T.n_meta[m]; c = a.c_meta;
  }

  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  float* const gr = a.grad_rows + (int64_t)f * B * D;
  float* const gl = a.grad_lin + (int64_t)f * B;

  const int64_t niter = (B + TPW - 1) / TPW;
  for (int64_t it_ = wave; it_ < niter; it_ += nwave) {
    const int64_t t = it_ * TPW + lane / G;
    const bool valid = t < B;
    const int64_t tc = valid ? t : 0;  // loads stay unconditional
    int64_t id = ids[tc * id_stride];
    bool ok = true;
    if ((uint64_t)id >= (uint64_t)n_rows) { ok = false; id = 0; }  // never an address; reported below
    RowReg<VEC, K> w, g;
    row_load<VEC, G, K>(w, tab, id, D, lig);
    row_load<VEC, G, K>(g, gr, tc, D, lig);
    float wl = 0.f, glv = 0.f;
    if (lin) {  // wave-uniform
      wl = lin[id];
      glv = gl[tc];
    }
    if (valid && !ok && lig == 0 && a.err) atomicOr(a.err, 1);
    if (valid && ok) {
      // -ffp-contract=off (Makefile): the product and the sum are two operations, each rounded once — with a power-of-two
      // coefficient the product is exact and the result is numpy float32's g + c * w bit for bit
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const float p = c * w.v[n];
        g.v[n] = g.v[n] + p;
      }
      row_store<VEC, G, K>(g, gr + t * (int64_t)D, D, lig);
      if (lin && lig == 0) {
        const float p = c * wl;
        gl[t] = glv + p;
      }
    }
  }
}

template <int NET>
int launch_l2(const L2Args& a, int n_fields, hipStream_t s) {
  RowCfg c;
  TRS_TRY(row_cfg_for("trs_stage_add_l2", a.T.D, c));
  const int tpw = TRS_WAVE / c.g;
  const int64_t waves = (a.B + tpw - 1) / tpw;
  // the grid's workgroup cap is for the whole launch: shared between the fields
  int gx = trs_grid(waves, TRS_BLOCK / TRS_WAVE);
  const int64_t per_field = trs_tuning().grid_cap / n_fields;
  if (gx > per_field) gx = per_field < 1 ? 1 : (int)per_field;
  const dim3 gr(gx, n_fields), bl(TRS_BLOCK);
  return for_row_shape(c, [&](auto V, auto G, auto K) {
    hipLaunchKernelGGL((l2_kernel<NET, V(), G(), K()>), gr, bl, 0, s, a);
    TRS_CHECK_LAUNCH("l2_kernel");
    return TRS_OK;
  });
}

}  // namespace

extern "C" int trs_stage_add_l2(int net, const trs_tables* tables, const int32_t* user_dev, const int32_t* items_dev,
                                const int32_t* meta_dev, int64_t B, int32_t S, int32_t M, float c_user, float c_item,
                                float c_meta, float* grad_rows_dev, float* grad_lin_dev, int32_t* err_flag_dev,
                                void* stream) {
  const char* who = "trs_stage_add_l2";
  TRS_TRY(trs_check_tables(who, net, tables));
  TRS_REQUIRE(S >= 1 && S <= 65, "%s: S=%d outside 1..65", who, S);
  TRS_REQUIRE(M == tables->M, "%s: M=%d does not match the tables' M=%d", who, M, tables->M);
  RowCfg cfg;
  TRS_TRY(row_cfg_for(who, tables->D, cfg));
  const float cs[3] = {c_user, c_item, c_meta};
  for (int i = 0; i < 3; ++i)  // (a NaN fails the first comparison)
    TRS_REQUIRE(cs[i] >= 0.f && cs[i] <= 3.0e38f, "%s: coefficient %d must be non-negative and finite", who, i);
  TRS_REQUIRE(grad_rows_dev, "%s: grad_rows is NULL", who);
  TRS_REQUIRE(grad_lin_dev, "%s: grad_lin is NULL", who);
  TRS_REQUIRE(B >= 0, "%s: negative batch size", who);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(user_dev && items_dev, "%s: user/item ids are NULL", who);
  const bool meta = M > 0 && c_meta > 0.f;
  TRS_REQUIRE(!meta || meta_dev, "%s: metadata ids are NULL but M=%d and c_meta > 0", who, M);
  const int n_fields = (c_user > 0.f ? 1 : 0) + (c_item > 0.f ? S : 0) + (meta ? S * M : 0);
  if (n_fields == 0) return TRS_OK;  // every coefficient 0: nothing to add, nothing launched
  L2Args a = {};
  a.T = *tables;
  a.user = user_dev;
  a.items = items_dev;
  a.meta = meta_dev;
  a.B = B;
  a.S = S;
  a.c_user = c_user;
  a.c_item = c_item;
  a.c_meta = meta ? c_meta : 0.f;
  a.grad_rows = grad_rows_dev;
  a.grad_lin = grad_lin_dev;
  a.err = err_flag_dev;
  if (net == TRS_NET_FM) return launch_l2<TRS_NET_FM>(a, n_fields, (hipStream_t)stream);
  return launch_l2<TRS_NET_LINEAR>(a, n_fields, (hipStream_t)stream);
}
