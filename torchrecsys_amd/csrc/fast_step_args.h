// fast_step_args.h — the argument block of the training-step kernels and the device helpers that read a triple's ids
// and rows: shared by fast_step.hip (fwd_stage_kernel and the update kernels behind it) and flag_step.hip
// (flag_step_kernel, the one-launch flag step of the whole-row shapes).  fast_step.hip's header describes the forms.
#pragma once
#include "score_kernels.h"
#include "opt_rows.h"

#include <math.h>
#include <stdlib.h>

namespace trs {

struct FastArgs {
  trs_tables T;
  // batch ids (int32): outputs of K1 when `from_stream`, inputs otherwise
  int32_t* user;
  int32_t* pos;
  int32_t* neg;
  int64_t B;
  int32_t* err;
  // resident stream (from_stream != 0)
  int from_stream;
  const int2* sui;  // (N) interleaved {user, item}: one 8-byte random read per triple instead of two 4-byte ones
  const int32_t* neg_static;
  int64_t N;
  uint64_t shuffle_key;
  int hb;
  int64_t t0;
  uint64_t sample_seed;
  uint64_t sample_offset;
  // staging
  float* gz;  // (2,B): score gradients of the positive / negative pass (after the FM sigmoid)
  float* du;  // (B,D)
  float inv_B;
  float lr;
  int loss;  // TRS_LOSS_HINGE | TRS_LOSS_BPR
  float* loss_sum;
  // duplicate detection (all NULL: every update is atomic)
  uint64_t* uown;  // (n_users) last reference of the step that named the row: (stamp << 32) | t
  uint64_t* iown;  // (n_items) (stamp << 32) | (2t + which)
  uint32_t* udup;  // (n_users) == stamp: the row has more than one reference in this step
  uint32_t* idup;  // (n_items)
  uint32_t stamp;
  // presorted mode with precomputed per-position user-duplicate flags (trs_epoch_presort): K1 applies the user update
  // itself for users referenced once in the batch and stages the OLD user row for K2 instead of the gradient
  const uint8_t* udup_pos;  // (B) 1: this triple's user has another reference in the batch; NULL: mode off
  // (B,2) {pos, neg}: 1 = that item row has another reference in the batch; NULL: every item reference goes through the
  // sorted runs.  Given: K1 applies the item update of a reference that is alone on its row itself (the user row is in
  // registers and nobody else reads or writes that item row this step) and K2 only walks rows with several references
  const uint8_t* idup_pos;
  float* ustage;            // (B,D) pre-update user rows, read by the sorted item update
  OptArgs o;                // update rule of the presorted mode (kind OPT_SGD: lr above)
  // INL 3 (flag mode, one launch per step): sync[0] = ONE monotonic arrival counter (zeroed by the host every 2^30 arrivals); a
  // launch counts its workgroups in and waits until the counter has reached sync_target = arrivals of all earlier
  // launches + its own grid (wrap-safe signed compare); sync[32 * (1 + g)], g < 8: flag lines that carry the last
  // completed target (TRS_SYNC_WORDS uint32 in all)
  uint32_t* sync;
  uint32_t sync_base, sync_target;
  // flagged-first order (trs_epoch_flags_ordered): *nflag = the batch's triples that carry a flagged reference, all of them
  // at its first positions; NULL = any order
  const int32_t* nflag;
  // INL 3, early mode (launch_fwd_stage fills them from TrsTuning): apply flagged references inside the main loop; count
  // the references applied in the loop / in the tail into sync[TRS_SYNC_WORDS - 2] / [TRS_SYNC_WORDS - 1]
  int apply_in_loop, apply_stats;
};

struct RawIds {   // loads issued, nothing consumed yet
  int32_t u, p, n;
  uint8_t dup;
  uint16_t idup;  // INL 2: {pos, neg} item-duplicate flags, one byte each
  int64_t v;      // SRC 1: uniform draw over n_items-1 values (the negative is v + (v >= pos))
  bool valid;
};

struct TripleIds {
  int32_t u, p, n;
  bool valid, ok, dup, pdup, ndup;
};

// SRC: 0 = ids given in user/pos/neg; 1 = resident stream + dynamic sampler; 2 = resident stream + static negatives.
// A template parameter, not a run-time branch: a conditional block that contains a load ends in s_waitcnt vmcnt(0),
// which would also drain the row gathers in flight.  issue_ids only ISSUES the loads (and does the id-independent
// Philox arithmetic); finalize_ids consumes them one iteration later, so the wait it implies covers loads that are
// older than every row gather still in flight (vmcnt is in-order).
template <int SRC, int INL>
__device__ __forceinline__ RawIds issue_ids(const FastArgs& a, int64_t t) {
  RawIds r;
  r.valid = t < a.B;
  const int64_t tc = r.valid ? t : a.B - 1;  // loads stay unconditional
  r.v = 0;
  if (SRC != 0) {
    const int64_t p = trs_feistel_perm(a.t0 + tc, a.N, a.shuffle_key, a.hb);
    const int2 ui = a.sui[p];
    r.u = ui.x;
    r.p = ui.y;
    if (SRC == 2) {
      r.n = a.neg_static[p];
    } else {
      const trs_u4 x = trs_philox4x32_10(a.sample_offset + (uint64_t)tc, a.sample_seed);
      const uint64_t x64 = ((uint64_t)x.y << 32) | (uint64_t)x.x;
      r.v = a.T.n_items > 1 ? (int64_t)trs_mulhi64(x64, (uint64_t)(a.T.n_items - 1)) : 0;
      r.n = 0;
    }
  } else {
    r.u = a.user[tc];
    r.p = a.pos[tc];
    r.n = a.neg[tc];
  }
  r.dup = 1;
  r.idup = 0x0101;
  if (INL) r.dup = a.udup_pos[tc];
  if (INL >= 2) r.idup = reinterpret_cast<const uint16_t*>(a.idup_pos)[tc];
  return r;
}

template <int SRC>
__device__ __forceinline__ TripleIds finalize_ids(const FastArgs& a, const RawIds& w) {
  TripleIds r;
  r.valid = w.valid;
  int64_t uid = w.u, pid = w.p;
  int64_t nid = SRC == 1 ? (a.T.n_items > 1 ? w.v + (w.v >= pid ? 1 : 0) : 0) : (int64_t)w.n;
  r.ok = true;
  if ((uint64_t)uid >= (uint64_t)a.T.n_users) { r.ok = false; uid = 0; }
  if ((uint64_t)pid >= (uint64_t)a.T.n_items) { r.ok = false; pid = 0; }
  if ((uint64_t)nid >= (uint64_t)a.T.n_items) { r.ok = false; nid = 0; }
  r.u = (int32_t)uid;
  r.p = (int32_t)pid;
  r.n = (int32_t)nid;
  r.dup = w.dup != 0;
  r.pdup = (w.idup & 0x00ffu) != 0;
  r.ndup = (w.idup & 0xff00u) != 0;
  return r;
}

template <int VEC, int K>
struct TripleRows {
  RowReg<VEC, K> u, pi, ni;
  float ul, pl, nl;
  RowReg<VEC, K> us1, us2;  // adaptive rules: the user row's optimiser state (exp_avg | sum, exp_avg_sq)
  float uls1, uls2;
};

template <int VEC, int G, int K, bool FULL, int OPT, int NTU = 0>
__device__ __forceinline__ void load_rows(TripleRows<VEC, K>& r, const trs_tables& T, const OptArgs& o,
                                          const TripleIds& id, int lig) {
  row_load<VEC, G, K, FULL, (NTU & 1) != 0>(r.u, T.user, id.u, T.D, lig);
  row_load<VEC, G, K, FULL>(r.pi, T.item, id.p, T.D, lig);
  row_load<VEC, G, K, FULL>(r.ni, T.item, id.n, T.D, lig);
  r.ul = T.user_lin[id.u];
  r.pl = T.item_lin[id.p];
  r.nl = T.item_lin[id.n];
  if (OPT != OPT_SGD) {  // compile-time: issued with the rows, unconditionally (duplicated users waste them: 6 % at c2)
    row_load<VEC, G, K, FULL>(r.us1, o.user_s1, id.u, T.D, lig);
    r.uls1 = o.user_lin_s1[id.u];
    if (OPT == OPT_ADAM) {
      row_load<VEC, G, K, FULL>(r.us2, o.user_s2, id.u, T.D, lig);
      r.uls2 = o.user_lin_s2[id.u];
    }
  }
}

constexpr int DEFER_ITERS = 8;  // iterations per lane group the per-wave list is sized for (launch_fwd_stage keeps to it)
struct DeferEntry {
  uint32_t tw;   // (t << 2) | which      which: 0 user (row staged in du), 1 positive, 2 negative (row staged in ustage)
  int32_t row;   // table row
  float c;       // coefficient of the staged row
  float clin;    // increment of the row's 1-wide term
};

// flag_step.hip: flag_step_kernel<NET, G, NTU> in place of fwd_stage_kernel<NET, 4, G, 1, 0, true, 3, OPT_SGD, NTU> for a
// flag-form step with an arrival counter and flagged-first batches.  > 0: not taken (knob off, not a whole-row shape,
// grid beyond the kernel's resident cap) and nothing was launched — the caller launches the old kernel.
int trs_launch_flag_step(int net, const FastArgs& a, const RowCfg& c, int ntu, int64_t grid, void* stream);

}  // namespace trs
