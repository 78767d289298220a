// multineg.hip — training on K sampled negatives per positive (trs_batch_prepare_multi, trs_score_multi_fwd_bwd;
// include/trs.h): sampled softmax over {positive, c_0 .. c_{K-1}} and the mean of K hinge / BPR pairs.
//
// prepare_multi_kernel: integer work only — one thread per (candidate j, row t), rows along the lanes, so the slot-major
// (1+K, B) id block is written in whole lines; the threads of candidate 0 also write the user and the positive.
//
// The two candidate kernels, multineg_kernel and warp_kernel (wave = 64), share their mapping and the parts written
// once below: one aligned group of G lanes per row, 16-byte lanes, as score_kernel; cand_row_head checks the row's ids
// and leaves the user row, its 1-wide term and the positive's pass in registers; candidates go in rounds of C =
// cand_round() (round_forward: C independent unconditional passes in flight before the first reduction, mine_kernel's
// pattern; slots past the last candidate load it again).  Every z is pass_forward_z's.  Gradients are staged — item
// slots through stage_item_slot in the layout of staged_item_field / staged_meta_field (score_kernels.h) —, never added
// to a table here: every gradient of a step comes from the pre-update tables.  No LDS (but block_add_loss_auc), no
// scratch memory.  What is each kernel's own:
//
// multineg_kernel (S = 1 + K item slots)
//   pair losses     one sweep: candidate j's weight needs only its own score and the positive's; the user row's
//                   gradient and the positive's weight are accumulated and written after the sweep.
//   sampled softmax every zh before any weight: sweep 1 keeps the running (maximum, sum of exponentials) of the row.
//                   K <= C: the single round's rows are still in registers and the gradients follow at once.
//                   Otherwise sweep 2 re-reads the rows (L2-hot), recomputes each z — bit-identical, the same code on
//                   the same tables — and stages the gradients.  Forward-only mode stops after sweep 1.
//
// warp_kernel (trs_score_warp_fwd_bwd; S = 2, the pair layout): the first candidate that violates the
// margin is trained on alone, weighted by a rank estimate; described above the kernel.
#include "score_kernels.h"

using namespace trs;

namespace {

#ifndef MULTI_ROW_VGPRS
// VGPRs of candidate item rows in flight per round (with metadata the field sums take as many again).  mine_kernel holds 32;
// here the rows stay live until their weights are known: at 32 the FM softmax kernels spill into AGPRs and run one wave
// per SIMD, at 16 every instantiation runs at least two and the whole-row FM shapes three or four
#define MULTI_ROW_VGPRS 16
#endif

struct PrepMultiArgs {
  const int32_t* su;
  const int32_t* si;
  int64_t N;
  uint64_t shuffle_key;
  int hb;
  int64_t t0, B, n_items;
  uint64_t seed, offset;
  const int32_t* item_meta;
  int M, Kn;
  int32_t *user, *items, *meta;
  TrsSampler S;
};

__global__ __launch_bounds__(TRS_BLOCK) void prepare_multi_kernel(const PrepMultiArgs a) {
  const int64_t stride = (int64_t)gridDim.x * TRS_BLOCK;
  const int64_t total = a.B * a.Kn;
  for (int64_t w = (int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x; w < total; w += stride) {
    const int64_t j = w / a.B;
    const int64_t t = w - j * a.B;
    const int64_t p = trs_feistel_perm(a.t0 + t, a.N * a.S.k_neg, a.shuffle_key, a.hb) % a.N;
    const int32_t u = a.su[p];
    const int32_t i = a.si[p];
    int32_t c;
    if (a.S.max_tries != 0 && (uint64_t)(int64_t)i >= (uint64_t)a.n_items)
      c = 0;  // (reported by the scorer; the option paths index tables by the ids)
    else
      c = (int32_t)trs_sample_neg_opt(a.seed + (uint64_t)j * TRS_CANDIDATE_KEY_STEP, a.offset + (uint64_t)t,
                                      (int64_t)u, (int64_t)i, a.n_items, a.S);
    a.items[(1 + j) * a.B + t] = c;
    if (j == 0) {
      a.user[t] = u;
      a.items[t] = i;
    }
    if (a.M > 0) {
      // an id outside the item table is reported by the scorer kernel; keep this lookup in range
      const int64_t cc = ((uint64_t)(int64_t)c < (uint64_t)a.n_items) ? c : 0;
      for (int m = 0; m < a.M; ++m) a.meta[((1 + j) * a.B + t) * a.M + m] = a.item_meta[cc * a.M + m];
      if (j == 0) {
        const int64_t ic = ((uint64_t)(int64_t)i < (uint64_t)a.n_items) ? i : 0;
        for (int m = 0; m < a.M; ++m) a.meta[t * a.M + m] = a.item_meta[ic * a.M + m];
      }
    }
  }
}

struct MultiArgs {
  trs_tables T;
  const int32_t* user;   // (B)
  const int32_t* items;  // (1+K, B): row 0 the positives, row 1+j candidate j
  const int32_t* meta;   // (1+K, B, M) or NULL
  int64_t B;
  int Kn;    // sampled negatives per row, 1..64
  int loss;  // TRS_LOSS_HINGE | TRS_LOSS_BPR (SM == false)
  float inv_tau, inv_B;
  float* loss_sum;
  int32_t* auc_count;
  float* grad_rows;  // (F, B, D), F = 1 + (1+K)(1+M); NULL: forward only
  float* grad_lin;   // (F, B)
  int32_t* err;
};

// ---------------------------------------------------------------------- what the two candidate kernels share
// (A: MultiArgs or WarpArgs — the id blocks, B, Kn, err and the tables are named alike)

// Candidates per round (a power of two): at most 8, the lane group, and MULTI_ROW_VGPRS of item rows in flight.
template <int VEC, int G, int K>
constexpr int cand_round() {
  constexpr int CR = MULTI_ROW_VGPRS / (K * VEC) < 8 ? (MULTI_ROW_VGPRS / (K * VEC) < 1 ? 1 : MULTI_ROW_VGPRS / (K * VEC)) : 8;
  return G < CR ? G : CR;
}

// The head of a row: every id of the row against its table first (integer work, spread over the group) — a row with
// an id out of range sets the error flag and carries no loss and zero gradients (live = false), as score_kernel's dead
// triples —, then the user row with its 1-wide term and the positive's pass (z0; sp = pass_forward's score).
template <int NET, int VEC, int G, int K, typename A>
__device__ __forceinline__ void cand_row_head(const A& a, int M, int64_t tc, bool valid, int lig, bool& live,
                                              RowReg<VEC, K>& ur, float& u_lin, RowReg<VEC, K>& pr,
                                              RowReg<VEC, K>& Sp, float& z0, float& sp) {
  const trs_tables& T = a.T;
  int64_t uid = a.user[tc];
  int bad = 0;
  if ((uint64_t)uid >= (uint64_t)T.n_users) { bad = 1; uid = 0; }
  for (int s = lig; s < 1 + a.Kn; s += G) {
    const int64_t e = (int64_t)s * a.B + tc;
    if ((uint64_t)(int64_t)a.items[e] >= (uint64_t)T.n_items) bad = 1;
    for (int m = 0; m < M; ++m)
      if ((uint64_t)(int64_t)a.meta[e * M + m] >= (uint64_t)T.n_meta[m]) bad = 1;
  }
  bad = trs_group_or<G>(bad);
  if (valid && bad && lig == 0 && a.err) atomicOr(a.err, 1);
  live = valid && !bad;

  row_load<VEC, G, K>(ur, T.user, uid, T.D, lig);
  u_lin = T.user_lin[uid];
  int64_t pid = a.items[tc];
  if ((uint64_t)pid >= (uint64_t)T.n_items) pid = 0;
  float p_lin, lin_p;
  bool okp = true;
  z0 = pass_forward_z<NET, VEC, G, K>(T, ur, u_lin, pid, a.meta, 4, tc, true, lig, pr, Sp, p_lin, lin_p, okp);
  sp = NET == TRS_NET_FM ? sigmoidf_(z0) : z0;
}

// The metadata ids of row t's item slot `slot` (0 the positive, 1 + j candidate j) in the (1+K, B, M) block, as
// stage_item_slot takes them.
template <typename A>
__device__ __forceinline__ auto slot_meta_ids(const A& a, int M, int slot, int64_t t) {
  return [&a, M, slot, t](int m) -> int64_t { return a.meta[((int64_t)slot * a.B + t) * M + m]; };
}

// The forward part of one round: the ids of candidates r0 .. r0 + C - 1 (lane c of the group reads candidate r0 + c's,
// a shuffle hands them round) and their C independent passes.
template <int NET, int VEC, int G, int K, int C, typename A>
__device__ __forceinline__ void round_forward(const A& a, const RowReg<VEC, K>& ur, float u_lin, int r0,
                                              int64_t tc, int lig, int gbase, RowReg<VEC, K> (&ir)[C],
                                              RowReg<VEC, K> (&Ss)[C], float (&z)[C]) {
  const int Kn = a.Kn;
  int jm = r0 + (lig & (C - 1));
  jm = jm < Kn ? jm : Kn - 1;  // past the last candidate: load it again (its score is not used)
  const int32_t mine = a.items[(int64_t)(1 + jm) * a.B + tc];
#pragma unroll
  for (int c = 0; c < C; ++c) {
    const int32_t id = __shfl(mine, gbase + c, 64);
    const int64_t cl = (uint64_t)(int64_t)id < (uint64_t)a.T.n_items ? id : 0;
    const int jc = r0 + c < Kn ? r0 + c : Kn - 1;
    float il, ls;
    bool ok = true;  // (the row's ids were checked before the first load)
    z[c] = pass_forward_z<NET, VEC, G, K>(a.T, ur, u_lin, cl, a.meta + (int64_t)(1 + jc) * a.B * a.T.M, 4, tc, true,
                                          lig, ir[c], Ss[c], il, ls, ok);
  }
}

// META = false: the tables have no metadata columns (M == 0 at compile time: the field sums of a round die with its
// reduction instead of staying in registers beside the item rows).
template <int NET, int VEC, int G, int K, bool SM, bool META>
__global__ __launch_bounds__(TRS_BLOCK) void multineg_kernel(const MultiArgs a) {
  constexpr int N = K * VEC;
  constexpr int C = cand_round<VEC, G, K>();
  constexpr int TPW = TRS_WAVE / G;  // rows per wave per iteration
  const trs_tables& T = a.T;
  const int D = T.D;
  const int M = META ? T.M : 0;
  const int64_t B = a.B;
  const int Kn = a.Kn;
  const int S1 = 1 + Kn;  // item slots of the staged layout: the positive, then candidate j in slot 1 + j
  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int gbase = lane - lig;
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const bool grad = a.grad_rows != nullptr;
  const float invK = 1.0f / (float)Kn;
  const float wK = a.inv_B * invK;  // weight of one pair of the mean over B rows and K pairs
  float* const gr = a.grad_rows;
  float* const gl = a.grad_lin;

  float loss_acc = 0.f;
  int auc_acc = 0;

  const int64_t niter = (B + TPW - 1) / TPW;
  for (int64_t it_ = wave; it_ < niter; it_ += nwave) {
    const int64_t t = it_ * TPW + lane / G;
    const bool valid = t < B;
    const int64_t tc = valid ? t : 0;  // loads stay unconditional

    bool live;
    RowReg<VEC, K> ur, pr, Sp;
    float u_lin, z0, sp;
    cand_row_head<NET, VEC, G, K>(a, M, tc, valid, lig, live, ur, u_lin, pr, Sp, z0, sp);

    const float zh0 = z0 * a.inv_tau;
    float mx = zh0, sum = 1.f, inv_sum = 1.f;  // sampled softmax: running maximum and sum of exponentials of the row
    RowReg<VEC, K> acc;  // sum over the candidates of g_j * (the row the user's gradient multiplies)
#pragma unroll
    for (int n = 0; n < N; ++n) acc.v[n] = 0.f;
    float gp_acc = 0.f, gn_sum = 0.f, row_loss = 0.f, p_sum = 0.f;

    // sampled softmax, the statistics of one round: running (maximum, sum of exponentials) over zh_0 .. zh_K
    auto stats_round = [&](int r0, const float (&z)[C]) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        if (r0 + c < Kn) {
          const float zh = z[c] * a.inv_tau;
          const float mn = fmaxf(mx, zh);
          sum = sum * expf(mx - mn) + expf(zh - mn);
          mx = mn;
          if (r0 + c == 0 && live && lig == 0) auc_acc += (sp > (NET == TRS_NET_FM ? sigmoidf_(z[c]) : z[c])) ? 1 : 0;
        }
      }
    };
    // the weights and the staged gradients of one round (pair losses: also their forward)
    auto grad_round = [&](int r0, const RowReg<VEC, K> (&ir)[C], const RowReg<VEC, K> (&Ss)[C], const float (&z)[C]) {
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int j = r0 + c;
        if (j < Kn) {
          float g;  // d loss / d z_j
          if (SM) {
            const float pj = expf(z[c] * a.inv_tau - mx) * inv_sum;
            p_sum += pj;
            g = live ? (pj * a.inv_B) * a.inv_tau : 0.f;
          } else {
            const float sn = NET == TRS_NET_FM ? sigmoidf_(z[c]) : z[c];
            float lval, dneg;
            trs_pair_loss(a.loss, sp, sn, lval, dneg);
            const float act = live ? dneg : 0.f;
            gp_acc += -act * wK;
            g = act * wK;
            if (live && lig == 0) {
              row_loss += lval;
              if (j == 0) auc_acc += (sp > sn) ? 1 : 0;
            }
            if (NET == TRS_NET_FM) g = g * ((1.0f - sn) * sn);  // through the sigmoid
          }
          gn_sum += g;
          // the user's share.  FM: g*(S - u) (= g*item when M == 0); Linear: g*S
          if (NET == TRS_NET_FM) {
            if (M == 0) {
#pragma unroll
              for (int n = 0; n < N; ++n) acc.v[n] += g * ir[c].v[n];
            } else {
#pragma unroll
              for (int n = 0; n < N; ++n) acc.v[n] += g * (Ss[c].v[n] - ur.v[n]);
            }
          } else {
#pragma unroll
            for (int n = 0; n < N; ++n) acc.v[n] += g * Ss[c].v[n];
          }
          if (grad && valid)
            stage_item_slot<NET, VEC, G, K>(T, M, S1, 1 + j, g, ur, ir[c], Ss[c], slot_meta_ids(a, M, 1 + j, t), gr, gl,
                                            B, t, lig);
        }
      }
    };

    if (SM) {
      RowReg<VEC, K> ir[C], Ss[C];
      float z[C];
      const bool one_round = Kn <= C;  // the single round's rows stay in registers; otherwise sweep 2 re-reads them
      for (int r0 = 0; r0 < Kn; r0 += C) {
        round_forward<NET, VEC, G, K, C>(a, ur, u_lin, r0, tc, lig, gbase, ir, Ss, z);
        stats_round(r0, z);
      }
      // logsumexp - zh_0 with the maximum taken out of the difference first (zh grows as 1 / tau)
      if (live && lig == 0) loss_acc += (mx - zh0) + logf(sum);
      inv_sum = 1.0f / sum;
      if (grad) {
        if (one_round) {
          grad_round(0, ir, Ss, z);
        } else {
          for (int r0 = 0; r0 < Kn; r0 += C) {  // (each z again: bit-identical, the same code on the same tables)
            round_forward<NET, VEC, G, K, C>(a, ur, u_lin, r0, tc, lig, gbase, ir, Ss, z);
            grad_round(r0, ir, Ss, z);
          }
        }
      }
    } else {
      for (int r0 = 0; r0 < Kn; r0 += C) {
        RowReg<VEC, K> ir[C], Ss[C];
        float z[C];
        round_forward<NET, VEC, G, K, C>(a, ur, u_lin, r0, tc, lig, gbase, ir, Ss, z);
        grad_round(r0, ir, Ss, z);
      }
    }
    if (!SM && live && lig == 0) loss_acc += row_loss * invK;

    if (grad && valid) {
      float gp;  // d loss / d z of the positive
      if (SM) {
        gp = live ? (-p_sum * a.inv_B) * a.inv_tau : 0.f;  // softmax_0 - 1 = -(sum of the candidates' shares)
      } else {
        gp = gp_acc;
        if (NET == TRS_NET_FM) gp = gp * ((1.0f - sp) * sp);
      }
      RowReg<VEC, K> gv;
      // field 0: user
      if (NET == TRS_NET_FM) {
        if (M == 0) {
#pragma unroll
          for (int n = 0; n < N; ++n) gv.v[n] = gp * pr.v[n] + acc.v[n];
        } else {
#pragma unroll
          for (int n = 0; n < N; ++n) gv.v[n] = gp * (Sp.v[n] - ur.v[n]) + acc.v[n];
        }
      } else {
#pragma unroll
        for (int n = 0; n < N; ++n) gv.v[n] = gp * Sp.v[n] + acc.v[n];
      }
      row_store<VEC, G, K>(gv, gr + t * (int64_t)D, D, lig);
      stage_item_slot<NET, VEC, G, K>(T, M, S1, 0, gp, ur, pr, Sp, slot_meta_ids(a, M, 0, t), gr, gl, B, t, lig);
      // the user's 1-wide term enters every z of the row with derivative 1: the softmax weights sum to exactly 0
      if (lig == 0) gl[t] = SM ? 0.f : gp + gn_sum;
    }
  }

  if (a.loss_sum) block_add_loss_auc(loss_acc, auc_acc, a.loss_sum, a.auc_count);
}

// ------------------------------------------------------------------------------------------------ WARP
struct WarpArgs {
  trs_tables T;
  const int32_t* user;   // (B)
  const int32_t* items;  // (1+K, B): row 0 the positives, row 1+j candidate j
  const int32_t* meta;   // (1+K, B, M) or NULL
  int64_t B;
  int Kn;  // candidates per row, 1..64
  float margin, inv_B;
  const float* rank_weight;  // (K): the weight of a row whose first violator is candidate j
  float* loss_sum;
  int32_t* auc_count;
  int32_t* neg_out;       // (B): the chosen candidate's id (c_0 without a violator)
  int32_t* neg_meta_out;  // (B, M)
  int32_t* trials_out;    // (B) or NULL: J + 1, 0 without a violator
  float* grad_rows;       // (3 + 2M, B, D), trs_score_fwd_bwd's field order; NULL: forward only
  float* grad_lin;        // (3 + 2M, B)
  int32_t* err;
};

// warp_kernel: what differs from multineg_kernel (the shared parts: the head of this file):
//   first violator  within a round the lowest j with (z_j - z_p) + margin > 0, found by selects from the last slot down;
//                   a group that has its J keeps scoring with its wave (the loads and shuffles stay whole-wave) and
//                   ignores what it sees, again by select.
//   one sweep       the weight depends on J alone, so the group stages (user, positive, chosen candidate) in the round
//                   where it finds J, from that round's registers: the chosen row is picked by a chain of selects (a
//                   register array indexed at run time would go to scratch), the stores sit under the group-uniform
//                   predicate.  No user or item row is read twice; FM with metadata reads the chosen slot's metadata
//                   rows again, as score_kernel does (pass_forward_z does not hand them back).
//   early exit      the round loop ends when __all lanes of the wave are done (J found, t >= B or a bad id): the vote is
//                   wave-uniform, so no shuffle of a later round runs with part of a group inactive.
// rank_weight is read by an ordinary vector load.  No LDS (but the block's loss reduction), no scratch memory.
template <int NET, int VEC, int G, int K, bool META>
__global__ __launch_bounds__(TRS_BLOCK) void warp_kernel(const WarpArgs a) {
  constexpr int N = K * VEC;
  constexpr int C = cand_round<VEC, G, K>();
  constexpr int TPW = TRS_WAVE / G;
  constexpr bool FM = NET == TRS_NET_FM;
  const trs_tables& T = a.T;
  const int D = T.D;
  const int M = META ? T.M : 0;
  const int64_t B = a.B;
  const int Kn = a.Kn;
  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int gbase = lane - lig;
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const bool grad = a.grad_rows != nullptr;
  const int64_t BD = B * (int64_t)D;
  float* const gr = a.grad_rows;
  float* const gl = a.grad_lin;

  float loss_acc = 0.f;
  int auc_acc = 0;

  const int64_t niter = (B + TPW - 1) / TPW;
  for (int64_t it_ = wave; it_ < niter; it_ += nwave) {
    const int64_t t = it_ * TPW + lane / G;
    const bool valid = t < B;
    const int64_t tc = valid ? t : 0;  // loads stay unconditional

    bool live;
    RowReg<VEC, K> ur, pr, Sp;
    float u_lin, z0, sp;  // (sp: the AUC count is on the scores, the hinge on z)
    cand_row_head<NET, VEC, G, K>(a, M, tc, valid, lig, live, ur, u_lin, pr, Sp, z0, sp);

    bool done = !live;  // group-uniform: J found, the row past the batch, or a bad id
    int trials = 0;

    for (int r0 = 0; r0 < Kn; r0 += C) {
      if (__all(done)) break;  // wave-uniform
      RowReg<VEC, K> ir[C], Ss[C];
      float z[C];
      round_forward<NET, VEC, G, K, C>(a, ur, u_lin, r0, tc, lig, gbase, ir, Ss, z);
      if (r0 == 0 && live && lig == 0) auc_acc += (sp > (FM ? sigmoidf_(z[0]) : z[0])) ? 1 : 0;
      // the lowest violating slot of the round, its hinge operand and its rows (selects; a NaN does not violate)
      int cf = -1;
      float hJ = 0.f;
      RowReg<VEC, K> ni, Sn;
#pragma unroll
      for (int n = 0; n < N; ++n) ni.v[n] = Sn.v[n] = 0.f;
#pragma unroll
      for (int c = C - 1; c >= 0; --c) {
        const float h = (z[c] - z0) + a.margin;
        const bool v = r0 + c < Kn && h > 0.f;
        cf = v ? c : cf;
        hJ = v ? h : hJ;
#pragma unroll
        for (int n = 0; n < N; ++n) {
          if (FM) ni.v[n] = v ? ir[c].v[n] : ni.v[n];
          if (!FM || META) Sn.v[n] = v ? Ss[c].v[n] : Sn.v[n];
        }
      }
      const bool hit = !done && cf >= 0;
      const int J = hit ? r0 + cf : 0;
      const float w = a.rank_weight[J];  // unconditional, inside the table; used under `hit` only
      if (hit) {
        done = true;
        trials = J + 1;
        if (lig == 0) {
          loss_acc += w * hJ;
          a.neg_out[t] = a.items[(int64_t)(1 + J) * B + t];
          for (int m = 0; m < M; ++m) a.neg_meta_out[t * M + m] = a.meta[((int64_t)(1 + J) * B + t) * M + m];
        }
        if (grad) {
          // d loss / d z: + w / B at the chosen candidate, - w / B at the positive (no sigmoid factor: the hinge is on z)
          const float gn = w * a.inv_B, gp = -gn;
          RowReg<VEC, K> g;
          pair_user_field<NET>(g, M != 0, gp, gn, ur, pr, ni, Sp, Sn);
          row_store<VEC, G, K>(g, gr + t * (int64_t)D, D, lig);
          // the pair layout (S = 2): the positive, then the chosen candidate, whose ids are slot 1 + J's
          stage_item_slot<NET, VEC, G, K>(T, M, 2, 0, gp, ur, pr, Sp, slot_meta_ids(a, M, 0, t), gr, gl, B, t, lig);
          stage_item_slot<NET, VEC, G, K>(T, M, 2, 1, gn, ur, ni, Sn, slot_meta_ids(a, M, 1 + J, t), gr, gl, B, t, lig);
          if (lig == 0) gl[t] = 0.f;  // the user's 1-wide term enters both z with derivative 1: exactly 0
        }
      }
    }

    if (valid && lig == 0 && a.trials_out) a.trials_out[t] = trials;
    if (valid && trials == 0) {  // no violator (or a dead row): c_0 keeps the index lists valid, every gradient is 0
      if (lig == 0) {
        a.neg_out[t] = a.items[B + t];
        for (int m = 0; m < M; ++m) a.neg_meta_out[t * M + m] = a.meta[(B + t) * M + m];
      }
      if (grad) {
        RowReg<VEC, K> g;
#pragma unroll
        for (int n = 0; n < N; ++n) g.v[n] = 0.f;
        const int R = 3 + 2 * M;
        for (int f = 0; f < R; ++f) {
          row_store<VEC, G, K>(g, gr + (int64_t)f * BD + t * (int64_t)D, D, lig);
          if (lig == 0) gl[(int64_t)f * B + t] = 0.f;
        }
      }
    }
  }

  if (a.loss_sum) block_add_loss_auc(loss_acc, auc_acc, a.loss_sum, a.auc_count);
}

// One launcher for both candidate kernels: one lane group per row.  kernel_of(V, G, K, META) names the instance.
template <typename A, typename KernelOf>
int launch_cand(const char* who, const char* kernel, const A& a, hipStream_t s, KernelOf kernel_of) {
  RowCfg c;
  TRS_TRY(row_cfg_for(who, a.T.D, c));
  const int tpw = TRS_WAVE / c.g;
  const int64_t waves = (a.B + tpw - 1) / tpw;
  const dim3 gr(trs_grid(waves, TRS_BLOCK / TRS_WAVE)), bl(TRS_BLOCK);
  return for_row_shape(c, [&](auto V, auto G, auto K) {
    if (a.T.M > 0) hipLaunchKernelGGL(kernel_of(V, G, K, std::true_type{}), gr, bl, 0, s, a);
    else hipLaunchKernelGGL(kernel_of(V, G, K, std::false_type{}), gr, bl, 0, s, a);
    TRS_CHECK_LAUNCH(kernel);
    return TRS_OK;
  });
}
template <int NET, bool SM>
int launch_multi(const MultiArgs& a, hipStream_t s) {
  return launch_cand("trs_score_multi_fwd_bwd", "multineg_kernel", a, s, [](auto V, auto G, auto K, auto META) {
    return multineg_kernel<NET, V(), G(), K(), SM, META()>; });
}
template <int NET>
int launch_warp(const WarpArgs& a, hipStream_t s) {
  return launch_cand("trs_score_warp_fwd_bwd", "warp_kernel", a, s, [](auto V, auto G, auto K, auto META) {
    return warp_kernel<NET, V(), G(), K(), META()>; });
}

// The argument checks trs_score_multi_fwd_bwd and trs_score_warp_fwd_bwd share (everything but the loss's own
// parameters); B == 0 passes: the caller returns before it launches.
int check_multi_args(const char* who, int net, const trs_tables* tables, const int32_t* user_dev,
                     const int32_t* items_dev, const int32_t* meta_dev, int64_t B, int32_t M, int32_t K,
                     const float* loss_sum_dev, const float* grad_rows_dev, const float* grad_lin_dev) {
  TRS_TRY(trs_check_tables(who, net, tables));
  TRS_REQUIRE(K >= 1 && K <= 64, "%s: K=%d outside 1..64", who, K);
  TRS_REQUIRE(M == tables->M, "%s: M=%d does not match the tables' M=%d", who, M, tables->M);
  RowCfg cfg;
  TRS_TRY(row_cfg_for(who, tables->D, cfg));
  TRS_REQUIRE(loss_sum_dev, "%s: loss_sum is NULL", who);
  TRS_REQUIRE((grad_rows_dev == nullptr) == (grad_lin_dev == nullptr),
              "%s: grad_rows and grad_lin must both be given or both NULL (forward only)", who);
  TRS_REQUIRE(B >= 0, "%s: negative batch size", who);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(user_dev && items_dev, "%s: user/item ids are NULL", who);
  TRS_REQUIRE(M == 0 || meta_dev, "%s: metadata ids are NULL but M=%d", who, M);
  return TRS_OK;
}

}  // namespace

extern "C" int trs_batch_prepare_multi(const int32_t* stream_user_dev, const int32_t* stream_item_dev,
                                       const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key, int64_t t0,
                                       int64_t B, int64_t n_items, uint64_t sample_seed, uint64_t sample_offset,
                                       const int32_t* item_meta_dev, int32_t M, int32_t* user_out, int32_t* items_out,
                                       int32_t* meta_out, const trs_sampler* sampler, int32_t n_neg, void* stream) {
  const char* who = "trs_batch_prepare_multi";
  TRS_REQUIRE(n_neg >= 1 && n_neg <= 64, "%s: n_neg=%d outside 1..64", who, n_neg);
  TRS_REQUIRE(neg_static_dev == nullptr, "%s: no static negatives (neg_static must be NULL)", who);
  TRS_REQUIRE(M >= 0 && M <= TRS_MAX_META, "%s: M=%d outside 0..%d", who, M, TRS_MAX_META);
  TRS_REQUIRE(M == 0 || (item_meta_dev && meta_out), "%s: M=%d needs item_meta and the metadata output", who, M);
  int64_t kn;
  TRS_TRY(trs_check_slice(who, N, t0, B, sampler, kn));
  TRS_TRY(trs_check_sampler(who, sampler));
  TRS_REQUIRE(n_items >= 2, "%s: dynamic sampling needs n_items >= 2", who);
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(stream_user_dev && stream_item_dev, "%s: stream is NULL", who);
  TRS_REQUIRE(user_out && items_out, "%s: outputs are NULL", who);
  PrepMultiArgs a = {};
  a.su = stream_user_dev;
  a.si = stream_item_dev;
  a.N = N;
  a.shuffle_key = shuffle_key;
  a.hb = trs_feistel_half_bits(N * kn);
  a.t0 = t0;
  a.B = B;
  a.n_items = n_items;
  a.seed = sample_seed;
  a.offset = sample_offset;
  a.item_meta = item_meta_dev;
  a.M = M;
  a.Kn = n_neg;
  a.user = user_out;
  a.items = items_out;
  a.meta = meta_out;
  a.S = trs_sampler_args(sampler);
  hipLaunchKernelGGL(prepare_multi_kernel, dim3(trs_grid(B * n_neg, TRS_BLOCK)), dim3(TRS_BLOCK), 0,
                     (hipStream_t)stream, a);
  TRS_CHECK_LAUNCH("prepare_multi_kernel");
  return TRS_OK;
}

extern "C" int trs_score_multi_fwd_bwd(int net, const trs_tables* tables, const int32_t* user_dev,
                                       const int32_t* items_dev, const int32_t* meta_dev, int64_t B, int32_t M,
                                       int32_t K, int32_t loss, float tau, float inv_B, float* loss_sum_dev,
                                       int32_t* auc_count_dev, float* grad_rows_dev, float* grad_lin_dev,
                                       int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_score_multi_fwd_bwd";
  TRS_TRY(check_multi_args(who, net, tables, user_dev, items_dev, meta_dev, B, M, K, loss_sum_dev, grad_rows_dev,
                           grad_lin_dev));
  TRS_REQUIRE(loss == TRS_LOSS_HINGE || loss == TRS_LOSS_BPR || loss == TRS_LOSS_SAMPLED_SOFTMAX,
              "%s: unknown loss id %d", who, loss);
  TRS_REQUIRE(tau > 0.f && tau <= 3.0e38f, "%s: temperature must be positive and finite", who);
  if (B == 0) return TRS_OK;
  MultiArgs a = {};
  a.T = *tables;
  a.user = user_dev;
  a.items = items_dev;
  a.meta = meta_dev;
  a.B = B;
  a.Kn = K;
  a.loss = loss;
  a.inv_tau = 1.0f / tau;
  a.inv_B = inv_B;
  a.loss_sum = loss_sum_dev;
  a.auc_count = auc_count_dev;
  a.grad_rows = grad_rows_dev;
  a.grad_lin = grad_lin_dev;
  a.err = err_flag_dev;
  const bool sm = loss == TRS_LOSS_SAMPLED_SOFTMAX;
  if (net == TRS_NET_FM)
    return sm ? launch_multi<TRS_NET_FM, true>(a, (hipStream_t)stream) : launch_multi<TRS_NET_FM, false>(a, (hipStream_t)stream);
  return sm ? launch_multi<TRS_NET_LINEAR, true>(a, (hipStream_t)stream)
            : launch_multi<TRS_NET_LINEAR, false>(a, (hipStream_t)stream);
}

extern "C" int trs_score_warp_fwd_bwd(int net, const trs_tables* tables, const int32_t* user_dev,
                                      const int32_t* items_dev, const int32_t* meta_dev, int64_t B, int32_t M,
                                      int32_t K, float margin, const float* rank_weight_dev, float inv_B,
                                      float* loss_sum_dev, int32_t* auc_count_dev, int32_t* neg_out,
                                      int32_t* neg_meta_out, int32_t* trials_out, float* grad_rows_dev,
                                      float* grad_lin_dev, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_score_warp_fwd_bwd";
  TRS_TRY(check_multi_args(who, net, tables, user_dev, items_dev, meta_dev, B, M, K, loss_sum_dev, grad_rows_dev,
                           grad_lin_dev));
  TRS_REQUIRE(margin >= -3.0e38f && margin <= 3.0e38f, "%s: margin must be finite", who);
  TRS_REQUIRE(rank_weight_dev, "%s: rank_weight is NULL", who);
  TRS_REQUIRE(neg_out, "%s: neg_out is NULL", who);
  TRS_REQUIRE(M == 0 || neg_meta_out, "%s: neg_meta_out is NULL but M=%d", who, M);
  if (B == 0) return TRS_OK;
  WarpArgs a = {};
  a.T = *tables;
  a.user = user_dev;
  a.items = items_dev;
  a.meta = meta_dev;
  a.B = B;
  a.Kn = K;
  a.margin = margin;
  a.inv_B = inv_B;
  a.rank_weight = rank_weight_dev;
  a.loss_sum = loss_sum_dev;
  a.auc_count = auc_count_dev;
  a.neg_out = neg_out;
  a.neg_meta_out = neg_meta_out;
  a.trials_out = trials_out;
  a.grad_rows = grad_rows_dev;
  a.grad_lin = grad_lin_dev;
  a.err = err_flag_dev;
  if (net == TRS_NET_FM) return launch_warp<TRS_NET_FM>(a, (hipStream_t)stream);
  return launch_warp<TRS_NET_LINEAR>(a, (hipStream_t)stream);
}
