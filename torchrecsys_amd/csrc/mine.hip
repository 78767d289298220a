// mine.hip — score-aware hard-negative mining inside the device loader (trs_batch_prepare_mined, include/trs.h;
// DESIGN.md §4.7).  One launch: epoch shuffle -> (user, positive) -> K candidate negatives (the counter-based sampler
// of trs_batch_prepare under K keys) -> their scores under the CURRENT tables (pass_forward_z of score_kernels.h: the
// arithmetic of every scoring pass, before the FM sigmoid) -> the candidate of rank r in the project's score order
// (trs_topk_key) -> the triple's ids.
//
// Mapping (wave = 64): one aligned group of G lanes per triple, 16-byte lanes, as score_kernel.  The user row and its
// 1-wide term are loaded once and stay in registers.  Candidates go in rounds of C <= 8 (slots past the last
// candidate draw and load it again: loads stay unconditional): lane c of the group draws candidate r0 + c (integer
// work, spread over the lanes), a shuffle hands every id to the whole group, and the C item rows (+ 1-wide terms,
// + metadata rows) are independent unconditional loads, all in flight before the first reduction.  trs_group_sum
// leaves every score in every lane, so top = 1 is a running maximum of 64-bit keys; top > 1 keeps the keys spread over
// the group (candidate j in lane j % G, slot j / G — statically indexed) and finds the candidate of rank r by counting
// the larger keys.  No LDS, no atomics, no scratch memory; nothing is written but the triple's ids.
#include "score_kernels.h"

using namespace trs;

namespace {

struct MineArgs {
  const int32_t* su;
  const int32_t* si;
  int64_t N;
  uint64_t shuffle_key;
  int hb;
  int64_t t0, B, n_items;
  uint64_t seed, offset;
  const int32_t* item_meta;
  int32_t *user, *pos, *neg, *pos_meta, *neg_meta, *chosen;
  TrsSampler S;
  trs_tables T;
  int Kc;   // candidates per triple, 1..64
  int top;  // the negative is the candidate of rank mulhi64(x, top)
};

template <int NET, int VEC, int G, int K, bool FULL, bool NT>
__global__ __launch_bounds__(TRS_BLOCK) void mine_kernel(const MineArgs a) {
  constexpr int N = K * VEC;
  constexpr int CR = 32 / N < 8 ? 32 / N : 8;  // candidate rows in flight: at most 32 VGPRs of item rows
  constexpr int C = G < CR ? G : CR;           // candidates per round (a power of two)
  constexpr int SL = TRS_WAVE / G;             // key slots per lane: SL * G = 64 >= candidates
  constexpr int TPW = TRS_WAVE / G;
  const trs_tables& T = a.T;
  const int D = T.D;
  const int M = T.M;
  const int Kc = a.Kc;
  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int gbase = lane - lig;
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const bool ranked = a.top > 1;

  const int64_t niter = (a.B + TPW - 1) / TPW;
  for (int64_t it_ = wave; it_ < niter; it_ += nwave) {
    const int64_t t = it_ * TPW + lane / G;
    const bool valid = t < a.B;
    const int64_t tc = valid ? t : a.B - 1;  // loads stay unconditional
    const int64_t p = trs_feistel_perm(a.t0 + tc, a.N * a.S.k_neg, a.shuffle_key, a.hb) % a.N;
    const int32_t u = a.su[p];
    const int32_t i = a.si[p];
    const uint64_t ctr = a.offset + (uint64_t)tc;
    // as batch_prepare_kernel: the option paths index tables by the ids; the scorer reports the id later
    const bool bad_i = a.S.max_tries != 0 && (uint64_t)i >= (uint64_t)a.n_items;
    const int64_t uc = (uint64_t)u < (uint64_t)T.n_users ? u : 0;

    RowReg<VEC, K> ur;
    row_load<VEC, G, K, FULL, NT>(ur, T.user, uc, D, lig);
    const float u_lin = T.user_lin[uc];

    uint64_t best_key = 0;
    int32_t best_c = 0;
    uint64_t keys[SL];
#pragma unroll
    for (int s = 0; s < SL; ++s) keys[s] = 0;

    for (int r0 = 0; r0 < Kc; r0 += C) {
      int jm = r0 + (lig & (C - 1));
      jm = jm < Kc ? jm : Kc - 1;  // past the last candidate: draw it again (its score is not used)
      const int32_t cand =
          bad_i ? 0
                : (int32_t)trs_sample_neg_opt(a.seed + (uint64_t)jm * TRS_CANDIDATE_KEY_STEP, ctr, (int64_t)u,
                                              (int64_t)i, a.n_items, a.S);
      float z[C];
      int32_t cid[C];
#pragma unroll
      for (int c = 0; c < C; ++c) {
        cid[c] = __shfl(cand, gbase + c, 64);
        const int64_t cl = (uint64_t)cid[c] < (uint64_t)a.n_items ? cid[c] : 0;
        RowReg<VEC, K> ir, Ss;
        float il, ls;
        bool ok = true;
        z[c] = pass_forward_z<NET, VEC, G, K, FULL>(T, ur, u_lin, cl, a.item_meta, 4, cl, true, lig, ir, Ss, il, ls, ok);
      }
#pragma unroll
      for (int c = 0; c < C; ++c) {
        const int j = r0 + c;
        if (j < Kc) {
          const uint64_t key = trs_topk_key(z[c], (uint32_t)j);
          if (key > best_key) {
            best_key = key;
            best_c = cid[c];
          }
          if (ranked) {
#pragma unroll
            for (int s = 0; s < SL; ++s)
              if (s == j / G && lig == j % G) keys[s] = key;
          }
        }
      }
    }

    int chosen = (int)(0xFFFFFFFFu - (uint32_t)best_key);
    int32_t neg = best_c;
    if (ranked) {
      const trs_u4 rr = trs_philox4x32_10(ctr, a.seed + (uint64_t)Kc * TRS_CANDIDATE_KEY_STEP);
      const int r = (int)trs_mulhi64(((uint64_t)rr.y << 32) | (uint64_t)rr.x, (uint64_t)a.top);
      int cnt[SL];
#pragma unroll
      for (int s = 0; s < SL; ++s) cnt[s] = 0;
#pragma unroll
      for (int s = 0; s < SL; ++s) {
        for (int l = 0; l < G && s * G + l < Kc; ++l) {
          const uint32_t lo = __shfl((uint32_t)keys[s], gbase + l, 64);
          const uint32_t hi = __shfl((uint32_t)(keys[s] >> 32), gbase + l, 64);
          const uint64_t kb = ((uint64_t)hi << 32) | lo;
#pragma unroll
          for (int s2 = 0; s2 < SL; ++s2) cnt[s2] += kb > keys[s2] ? 1 : 0;
        }
      }
      int found = 0;  // the keys are distinct (they carry j): exactly one (lane, slot) of the group has rank r
#pragma unroll
      for (int s2 = 0; s2 < SL; ++s2) {
        const int j2 = s2 * G + lig;
        if (j2 < Kc && cnt[s2] == r) found = j2;
      }
      chosen = trs_group_sum_i<G>(found);
      neg = bad_i ? 0
                  : (int32_t)trs_sample_neg_opt(a.seed + (uint64_t)chosen * TRS_CANDIDATE_KEY_STEP, ctr, (int64_t)u,
                                                (int64_t)i, a.n_items, a.S);
    }

    if (valid && lig == 0) {
      a.user[t] = u;
      a.pos[t] = i;
      a.neg[t] = neg;
      if (a.chosen) a.chosen[t] = chosen;
      if (M > 0) {
        const int64_t ic = ((uint64_t)i < (uint64_t)a.n_items) ? i : 0;
        const int64_t jc = ((uint64_t)neg < (uint64_t)a.n_items) ? neg : 0;
        for (int m = 0; m < M; ++m) {
          a.pos_meta[t * M + m] = a.item_meta[ic * M + m];
          a.neg_meta[t * M + m] = a.item_meta[jc * M + m];
        }
      }
    }
  }
}

template <int NET>
int launch_mine(const MineArgs& a, hipStream_t s) {
  RowCfg c;
  TRS_TRY(row_cfg_for("trs_batch_prepare_mined", a.T.D, c));
  const int tpw = TRS_WAVE / c.g;
  const int64_t waves = (a.B + tpw - 1) / tpw;
  const dim3 gr(trs_grid(waves, TRS_BLOCK / TRS_WAVE)), bl(TRS_BLOCK);
  // whole rows in one 16-byte lane group: unmasked loads; user rows nontemporal when the user table is far beyond the
  // Infinity Cache (they are read once per launch), as the scoring pass does (trs_launch_pair_scores)
  const bool full = row_shape_is_whole(c.vec, c.g, c.k) && c.vec * c.g == a.T.D;
  const bool nt = full && (int64_t)a.T.n_users * a.T.D * 4 > ((int64_t)512 << 20);
  return for_row_shape(c, [&](auto V, auto G, auto K) {
    if constexpr (row_shape_is_whole(V(), G(), K())) {  // (the FULL kernels exist for these shapes only)
      if (nt) hipLaunchKernelGGL((mine_kernel<NET, V(), G(), K(), true, true>), gr, bl, 0, s, a);
      else if (full) hipLaunchKernelGGL((mine_kernel<NET, V(), G(), K(), true, false>), gr, bl, 0, s, a);
    }
    if (!full) hipLaunchKernelGGL((mine_kernel<NET, V(), G(), K(), false, false>), gr, bl, 0, s, a);
    TRS_CHECK_LAUNCH("mine_kernel");
    return TRS_OK;
  });
}

}  // namespace

extern "C" int trs_batch_prepare_mined(const int32_t* stream_user_dev, const int32_t* stream_item_dev,
                                       const int32_t* neg_static_dev, int64_t N, uint64_t shuffle_key, int64_t t0,
                                       int64_t B, int64_t n_items, uint64_t sample_seed, uint64_t sample_offset,
                                       const int32_t* item_meta_dev, int32_t M, int32_t* user_out, int32_t* pos_out,
                                       int32_t* neg_out, int32_t* pos_meta_out, int32_t* neg_meta_out,
                                       const trs_sampler* sampler, int net, const trs_tables* tables,
                                       int32_t candidates, int32_t top, int32_t* chosen_out, void* stream) {
  const char* who = "trs_batch_prepare_mined";
  TRS_TRY(trs_check_tables(who, net, tables));
  TRS_REQUIRE(candidates >= 1 && candidates <= 64, "%s: candidates=%d outside 1..64", who, candidates);
  TRS_REQUIRE(top >= 1 && top <= candidates, "%s: top=%d outside 1..candidates=%d", who, top, candidates);
  TRS_REQUIRE(neg_static_dev == nullptr, "%s: static negatives cannot be mined (neg_static must be NULL)", who);
  TRS_REQUIRE(M == tables->M, "%s: M=%d does not match the tables' M=%d", who, M, tables->M);
  TRS_REQUIRE(M == 0 || (item_meta_dev && pos_meta_out && neg_meta_out),
              "%s: M=%d needs item_meta and metadata outputs", who, M);
  RowCfg cfg;
  TRS_TRY(row_cfg_for(who, tables->D, cfg));
  TRS_REQUIRE(n_items >= 2 && n_items <= tables->n_items, "%s: needs 2 <= n_items <= the item table's rows", who);
  int64_t kn;
  TRS_TRY(trs_check_slice(who, N, t0, B, sampler, kn));
  TRS_TRY(trs_check_sampler(who, sampler));
  if (B == 0) return TRS_OK;
  TRS_REQUIRE(stream_user_dev && stream_item_dev, "%s: stream is NULL", who);
  TRS_REQUIRE(user_out && pos_out && neg_out, "%s: outputs are NULL", who);
  MineArgs a = {};
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
  a.user = user_out;
  a.pos = pos_out;
  a.neg = neg_out;
  a.pos_meta = pos_meta_out;
  a.neg_meta = neg_meta_out;
  a.chosen = chosen_out;
  a.S = trs_sampler_args(sampler);
  a.T = *tables;
  a.Kc = candidates;
  a.top = top;
  if (net == TRS_NET_FM) return launch_mine<TRS_NET_FM>(a, (hipStream_t)stream);
  return launch_mine<TRS_NET_LINEAR>(a, (hipStream_t)stream);
}
