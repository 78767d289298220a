// seq.hip — the sequence model (include/trs.h "sequence model"): a factorised Markov chain over the
// last L items of a user's ordered history on the Linear scorer's tables plus one context table C (n_items, D).
//
//   q(u, k) = U[u] + sum_{l < min(L, k)} w_l * C[s_u[k-1-l]]     z(u, k, i) = <q, V[i]> + b[i]
//
// seq_stage_kernel (trs_seq_fwd_bwd): one aligned group of G lanes per triple (user, entry, negative), 16-byte lanes
// where D % 4 == 0 — score_kernel's mapping, every shape of TRS_ROW_SHAPES.  The triple's ids come from the ordered
// CSR itself (k = entry - off[user], p = ids[entry], context ids[entry-1-l]); there is no (N, L) context array.  The
// rows U[u], V[p], V[n] are requested first, then the context rows in rounds of ctx_round() rows, all of a round in
// flight before the first is consumed (L <= ctx_round(): L + 3 loads in flight per lane group).  A context row is
// folded into q as it arrives and not kept: its gradient is the user's gradient times w_l, so q, V[p] and V[n] (and the
// user's gradient while it is staged) are the row data that stay in registers.  Gradients are staged, never added to a
// table here: every gradient of a step comes from the pre-update tables.  No LDS (but block_add_loss_auc), no scratch.
//
// seq_rows_kernel (trs_seq_user_rows): the same q, one lane group and one writer per output row, for retrieval.
#include "score_kernels.h"

using namespace trs;

namespace {

#ifndef SEQ_ROW_VGPRS
// VGPRs of context rows in flight per round (beside q, V[p], V[n])
#define SEQ_ROW_VGPRS 32
#endif

// Context rows per round: at most 8 and SEQ_ROW_VGPRS registers of rows in flight, at least one.
template <int VEC, int K>
constexpr int ctx_round() {
  constexpr int c = SEQ_ROW_VGPRS / (K * VEC);
  return c < 1 ? 1 : (c > 8 ? 8 : c);
}

struct SeqArgs {
  trs_tables T;
  const float* ctx;       // C (n_items, D)
  const int64_t* off;     // ordered CSR: (seq_rows + 1)
  const int32_t* ids;     // item ids in order
  int64_t seq_rows;
  const int32_t* user;    // (B)
  const int64_t* entry;   // (B) positions in ids
  const int32_t* neg;     // (B)
  int64_t B;
  int L;
  const float* w;         // (L)
  int loss;
  float inv_B;
  float* loss_sum;
  int32_t* auc_count;
  float* grad_rows;       // (3 + L, B, D); NULL: forward only
  float* grad_lin;        // (3, B)
  int32_t* ctx_ids_out;   // (L, B)
  int32_t* err;
};

// Folds context slots r0 .. r0 + C - 1 into q: the ids first, then C unconditional row loads, then the sums in slot
// order.  cbase points at ids[entry - 1] (slot l reads cbase[-l]); slot l is present iff l < nctx.  An absent slot
// loads row 0 and adds nothing (a select: q keeps its bits).  Returns 1 when a present id is outside the table.
template <int VEC, int G, int K, int C>
__device__ __forceinline__ int fold_ctx_round(RowReg<VEC, K>& q, const float* __restrict__ ctx, int64_t n_items, int D,
                                              const int32_t* cbase, int nctx, int r0, const float* __restrict__ w, int L,
                                              int lig) {
  constexpr int N = K * VEC;
  int bad = 0;
  int64_t cid[C];
  float wl[C];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int l = r0 + c;
    const bool present = l < nctx;
    int64_t id = present ? (int64_t)cbase[-(int64_t)l] : 0;
    if ((uint64_t)id >= (uint64_t)n_items) { bad = 1; id = 0; }
    cid[c] = id;
    wl[c] = l < L ? w[l] : 0.f;
  }
  RowReg<VEC, K> cr[C];
#pragma unroll
  for (int c = 0; c < C; ++c) row_load<VEC, G, K>(cr[c], ctx, cid[c], D, lig);
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const bool present = r0 + c < nctx;
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const float s = q.v[n] + wl[c] * cr[c].v[n];
      q.v[n] = present ? s : q.v[n];
    }
  }
  return bad;
}

template <int VEC, int G, int K>
__global__ __launch_bounds__(TRS_BLOCK) void seq_stage_kernel(const SeqArgs a) {
  constexpr int N = K * VEC;
  constexpr int C = ctx_round<VEC, K>();
  constexpr int TPW = TRS_WAVE / G;  // triples per wave per iteration
  const trs_tables& T = a.T;
  const int D = T.D;
  const int64_t B = a.B;
  const int L = a.L;
  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const int64_t BD = B * (int64_t)D;
  const int64_t n_seq_users = a.seq_rows < T.n_users ? a.seq_rows : T.n_users;

  float loss_acc = 0.f;
  int auc_acc = 0;

  const int64_t niter = (B + TPW - 1) / TPW;
  for (int64_t it_ = wave; it_ < niter; it_ += nwave) {
    const int64_t t = it_ * TPW + lane / G;
    const bool valid = t < B;
    const int64_t tc = valid ? t : 0;  // loads stay unconditional
    int bad = 0;
    int64_t uid = a.user[tc], nid = a.neg[tc], e = a.entry[tc];
    if ((uint64_t)uid >= (uint64_t)n_seq_users) { bad = 1; uid = 0; }
    if ((uint64_t)nid >= (uint64_t)T.n_items) { bad = 1; nid = 0; }
    const int64_t lo = a.off[uid], hi = a.off[uid + 1];
    if (e < lo || e >= hi) { bad = 1; e = lo; }
    // (a clamped user without entries has no position to address: no id is read, the row is dead already)
    const bool has = lo < hi;
    int64_t pid = has ? (int64_t)a.ids[e] : 0;
    if ((uint64_t)pid >= (uint64_t)T.n_items) { bad = 1; pid = 0; }
    const int64_t k = e - lo;  // predecessors of the entry in its user's sequence
    const int nctx = has ? (int)(k < (int64_t)L ? k : (int64_t)L) : 0;
    const int32_t* cbase = a.ids + e - 1;  // slot l is cbase[-l], read for l < nctx only

    RowReg<VEC, K> q, pi, ni;
    row_load<VEC, G, K>(q, T.user, uid, D, lig);
    row_load<VEC, G, K>(pi, T.item, pid, D, lig);
    row_load<VEC, G, K>(ni, T.item, nid, D, lig);
    const float p_lin = T.item_lin[pid], n_lin = T.item_lin[nid];
    for (int r0 = 0; r0 < L; r0 += C) {
      if (__all(r0 >= nctx)) break;  // wave-uniform: no triple of the wave has a slot left
      bad |= fold_ctx_round<VEC, G, K, C>(q, a.ctx, T.n_items, D, cbase, nctx, r0, a.w, L, lig);
    }
    if (valid && bad && lig == 0 && a.err) atomicOr(a.err, 1);
    const bool live = valid && !bad;

    float pp = 0.f, pn = 0.f;
#pragma unroll
    for (int n = 0; n < N; ++n) pp += q.v[n] * pi.v[n];
#pragma unroll
    for (int n = 0; n < N; ++n) pn += q.v[n] * ni.v[n];
    const float zp = trs_group_sum<G>(pp) + p_lin;
    const float zn = trs_group_sum<G>(pn) + n_lin;

    float lval, dneg;
    trs_pair_loss(a.loss, zp, zn, lval, dneg);
    const float act = live ? dneg : 0.f;
    const float gp = -act * a.inv_B, gn = act * a.inv_B;
    if (live && lig == 0) {
      loss_acc += lval;
      auc_acc += (zp > zn) ? 1 : 0;
    }

    if (a.grad_rows && valid) {
      float* const gr = a.grad_rows;
      RowReg<VEC, K> gu;  // the user's gradient; a context slot's is w_l times it
      pair_user_field<TRS_NET_LINEAR>(gu, false, gp, gn, q, pi, ni, pi, ni);
      row_store<VEC, G, K>(gu, gr + t * (int64_t)D, D, lig);
      const auto no_meta = [](int) -> int64_t { return 0; };
      stage_item_slot<TRS_NET_LINEAR, VEC, G, K>(T, 0, 2, 0, gp, q, pi, pi, no_meta, gr, a.grad_lin, B, t, lig);
      stage_item_slot<TRS_NET_LINEAR, VEC, G, K>(T, 0, 2, 1, gn, q, ni, ni, no_meta, gr, a.grad_lin, B, t, lig);
      if (lig == 0) a.grad_lin[t] = gp + gn;  // the user's 1-wide term: exactly 0 under a pair loss
      for (int l = 0; l < L; ++l) {
        const bool present = l < nctx;
        int64_t id = present ? (int64_t)cbase[-(int64_t)l] : 0;  // (again: L1-hot; no register array indexed by l)
        if ((uint64_t)id >= (uint64_t)T.n_items) id = 0;
        const float wl = a.w[l];
        RowReg<VEC, K> gc;
#pragma unroll
        for (int n = 0; n < N; ++n) gc.v[n] = present ? wl * gu.v[n] : 0.f;
        row_store<VEC, G, K>(gc, gr + (int64_t)(3 + l) * BD + t * (int64_t)D, D, lig);
        if (lig == 0) a.ctx_ids_out[(int64_t)l * B + t] = (int32_t)id;
      }
    }
  }

  if (a.loss_sum) block_add_loss_auc(loss_acc, auc_acc, a.loss_sum, a.auc_count);
}

struct SeqRowsArgs {
  const float* user;     // U (n_users, D)
  int64_t n_users;
  const float* ctx;      // C (n_items, D)
  int64_t n_items;
  int D;
  const int64_t* off;    // (n + 1)
  const int32_t* ids;
  const int64_t* users;  // (n) or NULL: no user row anywhere
  int64_t n;
  int L;
  const float* w;
  float* out;
  int64_t ld;
  int32_t* err;
};

template <int VEC, int G, int K>
__global__ __launch_bounds__(TRS_BLOCK) void seq_rows_kernel(const SeqRowsArgs a) {
  constexpr int N = K * VEC;
  constexpr int C = ctx_round<VEC, K>();
  constexpr int TPW = TRS_WAVE / G;
  const int D = a.D;
  const int L = a.L;
  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const int64_t niter = (a.n + TPW - 1) / TPW;
  for (int64_t it_ = wave; it_ < niter; it_ += nwave) {
    const int64_t r = it_ * TPW + lane / G;
    const bool valid = r < a.n;
    const int64_t rc = valid ? r : 0;
    int bad = 0;
    int64_t uid = a.users ? a.users[rc] : -1;
    const bool with_user = uid >= 0;
    if (with_user && uid >= a.n_users) bad = 1;
    if (!with_user || bad) uid = 0;
    const int64_t lo = a.off[rc], hi = a.off[rc + 1];
    const int64_t len = hi > lo ? hi - lo : 0;
    const int nctx = (int)(len < (int64_t)L ? len : (int64_t)L);
    const int32_t* cbase = a.ids + hi - 1;  // the row's last item; slot l is cbase[-l], read for l < nctx only

    RowReg<VEC, K> q;
    row_load<VEC, G, K>(q, a.user, uid, D, lig);
#pragma unroll
    for (int n = 0; n < N; ++n) q.v[n] = with_user ? q.v[n] : 0.f;
    for (int r0 = 0; r0 < L; r0 += C) {
      if (__all(r0 >= nctx)) break;
      bad |= fold_ctx_round<VEC, G, K, C>(q, a.ctx, a.n_items, D, cbase, nctx, r0, a.w, L, lig);
    }
    if (valid && bad && lig == 0 && a.err) atomicOr(a.err, 1);
    if (bad) {
#pragma unroll
      for (int n = 0; n < N; ++n) q.v[n] = 0.f;
    }
    if (valid) row_store<VEC, G, K>(q, a.out + r * a.ld, D, lig);
  }
}

template <typename A, typename KernelOf>
int launch_seq(const char* who, const char* kernel, const A& a, int D, int64_t rows, hipStream_t s, KernelOf kernel_of) {
  RowCfg c;
  TRS_TRY(row_cfg_for(who, D, c));
  const int tpw = TRS_WAVE / c.g;
  const int64_t waves = (rows + tpw - 1) / tpw;
  const dim3 gr(trs_grid(waves, TRS_BLOCK / TRS_WAVE)), bl(TRS_BLOCK);
  return for_row_shape(c, [&](auto V, auto G, auto K) {
    hipLaunchKernelGGL(kernel_of(V, G, K), gr, bl, 0, s, a);
    TRS_CHECK_LAUNCH(kernel);
    return TRS_OK;
  });
}

// what the two entry points check alike
int check_seq_common(const char* who, const trs_tables* tables, const float* ctx_dev, const trs_csr* seq, int32_t L,
                     const float* ctx_weight_dev) {
  TRS_TRY(trs_check_tables(who, TRS_NET_LINEAR, tables));
  TRS_REQUIRE(tables->M == 0, "%s: the sequence model takes no metadata columns (tables->M=%d)", who, tables->M);
  RowCfg cfg;
  TRS_TRY(row_cfg_for(who, tables->D, cfg));
  TRS_REQUIRE(ctx_dev, "%s: the context table is NULL", who);
  TRS_REQUIRE(seq && seq->off && seq->n_rows >= 0, "%s: the sequence CSR is NULL or has no offsets", who);
  TRS_REQUIRE(L >= 0 && L <= TRS_SEQ_LMAX, "%s: L=%d outside 0..%d", who, L, TRS_SEQ_LMAX);
  TRS_REQUIRE(L == 0 || ctx_weight_dev, "%s: ctx_weight is NULL but L=%d", who, L);
  return TRS_OK;
}

}  // namespace

extern "C" int trs_seq_fwd_bwd(const trs_tables* tables, const float* ctx_dev, const trs_csr* seq,
                               const int32_t* user_dev, const int64_t* entry_dev, const int32_t* neg_dev, int64_t B,
                               int32_t L, const float* ctx_weight_dev, int32_t loss, float inv_B, float* loss_sum_dev,
                               int32_t* auc_count_dev, float* grad_rows_dev, float* grad_lin_dev,
                               int32_t* ctx_ids_out_dev, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_seq_fwd_bwd";
  TRS_TRY(check_seq_common(who, tables, ctx_dev, seq, L, ctx_weight_dev));
  TRS_REQUIRE(seq->n_rows > 0 && seq->items, "%s: the sequence CSR has no rows or no item ids", who);
  TRS_REQUIRE(loss == TRS_LOSS_HINGE || loss == TRS_LOSS_BPR, "%s: loss id %d is not a pair loss (hinge / bpr)", who,
              loss);
  TRS_REQUIRE(loss_sum_dev, "%s: loss_sum is NULL", who);
  TRS_REQUIRE((grad_rows_dev == nullptr) == (grad_lin_dev == nullptr),
              "%s: grad_rows and grad_lin must both be given or both NULL (forward only)", who);
  TRS_REQUIRE(!grad_rows_dev || L == 0 || ctx_ids_out_dev, "%s: ctx_ids_out is NULL but gradients of L=%d slots are staged",
              who, L);
  TRS_REQUIRE(B >= 0, "%s: negative batch size", who);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(user_dev && entry_dev && neg_dev, "%s: user/entry/neg ids are NULL", who);
  SeqArgs a = {};
  a.T = *tables;
  a.ctx = ctx_dev;
  a.off = seq->off;
  a.ids = seq->items;
  a.seq_rows = seq->n_rows;
  a.user = user_dev;
  a.entry = entry_dev;
  a.neg = neg_dev;
  a.B = B;
  a.L = L;
  a.w = ctx_weight_dev;
  a.loss = loss;
  a.inv_B = inv_B;
  a.loss_sum = loss_sum_dev;
  a.auc_count = auc_count_dev;
  a.grad_rows = grad_rows_dev;
  a.grad_lin = grad_lin_dev;
  a.ctx_ids_out = ctx_ids_out_dev;
  a.err = err_flag_dev;
  return launch_seq(who, "seq_stage_kernel", a, tables->D, B, (hipStream_t)stream,
                    [](auto V, auto G, auto K) { return seq_stage_kernel<V(), G(), K()>; });
}

extern "C" int trs_seq_user_rows(const trs_tables* tables, const float* ctx_dev, const trs_csr* seq,
                                 const int64_t* users_dev, int64_t n, int32_t L, const float* ctx_weight_dev,
                                 float* out_dev, int64_t ld, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_seq_user_rows";
  TRS_TRY(check_seq_common(who, tables, ctx_dev, seq, L, ctx_weight_dev));
  TRS_REQUIRE(n >= 0 && seq->n_rows == n, "%s: the sequence CSR has %lld rows for n=%lld output rows", who,
              (long long)seq->n_rows, (long long)n);
  TRS_REQUIRE(ld >= tables->D, "%s: row stride ld=%lld below D=%d", who, (long long)ld, tables->D);
  TRS_REQUIRE(tables->D % 4 != 0 || ld % 4 == 0, "%s: row stride ld=%lld must be a multiple of 4 floats when D is", who,
              (long long)ld);
  if (n == 0) return TRS_OK;
  TRS_REQUIRE(out_dev, "%s: out is NULL", who);
  TRS_REQUIRE(seq->items || L == 0, "%s: the sequence CSR has no item ids", who);
  SeqRowsArgs a = {};
  a.user = tables->user;
  a.n_users = tables->n_users;
  a.ctx = ctx_dev;
  a.n_items = tables->n_items;
  a.D = tables->D;
  a.off = seq->off;
  a.ids = seq->items;
  a.users = users_dev;
  a.n = n;
  a.L = L;
  a.w = ctx_weight_dev;
  a.out = out_dev;
  a.ld = ld;
  a.err = err_flag_dev;
  return launch_seq(who, "seq_rows_kernel", a, tables->D, n, (hipStream_t)stream,
                    [](auto V, auto G, auto K) { return seq_rows_kernel<V(), G(), K()>; });
}
