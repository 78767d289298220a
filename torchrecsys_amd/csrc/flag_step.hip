// flag_step.hip — the one-launch flag step of the whole-row shapes as a kernel of its own.
//
// flag_step_kernel<NET, G, NTU> computes what fwd_stage_kernel<NET, 4, G, 1, 0, true, 3, OPT_SGD, NTU> (fast_step.hip)
// computes for the one form the engine runs in the sparse regime: ids given, plain SGD, whole rows (D = 4 * G, 16 bytes
// per lane), both flag arrays, an arrival counter and flagged-first batches (a.nflag).  It keeps that kernel's software
// pipeline, in-place updates of lone rows, arrival counting with one late look per wave, bounded fallback wait, error
// bits and loss reduction, and differs in three things:
//
//   * Flagged rows stay in registers.  A flagged-first batch puts every triple with a flagged reference into the wave's
//     first `fi` iterations (c4: fi = 1, sometimes 2).  Each lane group keeps the user row `u` and the user-gradient
//     row `g` of its triples of iterations 0 and 1 in two hold slots (8 registers each); such a triple stores nothing to
//     ustage / du, its list entries name the slot, and the apply forms c * u (item references) or -lr * g (the user)
//     from the held registers.  A held row is in group layout (4 consecutive floats per lane): it is turned through LDS
//     into one element per lane, so the float atomics keep the full-rate shape — a row = adjacent dwords across the
//     wave.  Triples flagged in iteration 2 or later (fi > 2) are staged through global memory and applied by the tail
//     as in fwd_stage_kernel: the overflow path.
//   * The in-loop apply has no loads: the wave looks at the arrival counter at the start of phase `ia` and issues the
//     atomics of its held references behind the reduces of phases ia, ia + 1 and ia + 2, FLAG_APPLY at a time.
//   * It is built for the waves it runs at: the launch runs two workgroups per CU (defer_resident_cap), so the bound is
//     __launch_bounds__(256, 3) = at most 168 VGPRs, which leaves occupancy - 1 = 2.  D, the trip structure and the
//     form are compile-time constants; the not-early grid wait, K > 1, ragged rows, SRC != 0 and the adaptive rules are
//     not here at all.
//
// A batch left in its order (nf = B) is only known on the device: it runs here too — every wave counts itself in behind
// its last iteration, the look finds the grid incomplete and the workgroup takes the bounded fallback wait.
#include "fast_step_args.h"

namespace trs {

// Ordering of the arrival add and the look (measurement builds set it; the shipped value is the default):
//   0  relaxed add, relaxed look; the add is pinned behind the reduce of the wave's last flagged triple
//   1  0 + the workgroup's arrival add is a release at agent scope
//   2  1 + an acquire fence at agent scope between a look that found the grid complete and the first atomic
#ifndef TRS_FLAG_STEP_ORDER
#define TRS_FLAG_STEP_ORDER 0
#endif

template <int NET, int G, int NTU>
__global__ __launch_bounds__(TRS_BLOCK, 3) void flag_step_kernel(const FastArgs a) {
  constexpr int VEC = 4, K = 1, N = 4, D = 4 * G;  // (the launcher checked a.T.D == D)
  constexpr int TPW = TRS_WAVE / G;
  constexpr int NWV = TRS_BLOCK / TRS_WAVE;
  constexpr int CAPW = DEFER_ITERS * TPW * 3, DU = 4, KDD = (D + TRS_WAVE - 1) / TRS_WAVE;
  // held references a wave applies behind one reduce: the in-loop share stays the one fwd_stage_kernel has and
  // tests/test_gpu_inloop_apply.py pins — 2 per phase (1 where a row is four dwords per lane), three phases
  constexpr int FLAG_APPLY = KDD >= 4 ? 1 : 2;
  __shared__ DeferEntry s_list[NWV * CAPW];  // a wave lists its flagged references in its own part (no LDS atomic)
  __shared__ float s_turn[NWV * D];          // per wave: one held row on its way from group layout to one element per lane
  __shared__ float s_loss[NWV];
  __shared__ int s_arr;   // waves of this workgroup that are past the flagged iterations
  __shared__ int s_left;  // some wave has not applied all its flagged references (the grid was not complete at its look)
  const trs_tables& T = a.T;
  const int64_t B = a.B;
  const int lane = threadIdx.x & 63;
  const int lig = lane % G;
  const int grp = lane / G;
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));  // (scalar)
  const int64_t wave = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) >> 6;
  const int64_t nwave = ((int64_t)gridDim.x * TRS_BLOCK) >> 6;
  const int64_t stride = nwave * TPW;  // triples between two iterations of one lane group
  float loss_acc = 0.f;

  if (threadIdx.x == 0) s_arr = s_left = 0;
  // every flagged row of the step is read in the launch's first fi iterations (nf = B, a batch left in its order: all)
  const int64_t fi = ((int64_t)*a.nflag + stride - 1) / stride;
  __syncthreads();
  bool arrived = false;
  // pin: a value the reduce of the wave's last flagged triple produced.  The empty asm needs it in a register and
  // clobbers memory, so in the ISA the add stands behind the waits that reduce made for its rows: no row of a flagged
  // triple is still in flight when the workgroup is counted in, whatever the scheduler does with the code around it.
  auto arrive = [&](float pin) __attribute__((always_inline)) {  // wave-uniform
    asm volatile("" ::"v"(pin) : "memory");
    int before = 0;
    if (lane == 0) before = atomicAdd(&s_arr, 1);
    before = __builtin_amdgcn_readfirstlane(before);
    if (before == NWV - 1 && lane == 0)  // the workgroup's last wave: count the workgroup in (result unused: no wait)
      (void)__hip_atomic_fetch_add(a.sync, 1u, TRS_FLAG_STEP_ORDER >= 1 ? __ATOMIC_RELEASE : __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT);
    arrived = true;
  };

  // The wave's list: entries [0, n_held) belong to triples of iterations 0 and 1 (rows in the hold slots), the rest to
  // later iterations (rows staged in global memory).  tw = which | 4 | slot << 3 | group << 4 (held) or which | t << 3.
  // (four variables, not arrays: an array selected by an entry's bits would be indexed in scratch memory)
  RowReg<VEC, K> hU0, hU1, hG0, hG1;
#pragma unroll
  for (int n = 0; n < N; ++n) hU0.v[n] = hU1.v[n] = hG0.v[n] = hG1.v[n] = 0.f;
  int my_cnt = 0, n_held = 0, next_e = 0;
  bool complete = false;

  // One held reference: the row goes from its group's registers through the wave's LDS row to one element per lane
  // (LDS operations of one wave execute in order: no barrier), then one float atomic per element.
  auto apply_held = [&](int e) __attribute__((always_inline)) {  // (wave-uniform)
    const DeferEntry ev = s_list[wv * CAPW + e];  // (same address in every lane: one LDS broadcast)
    const uint32_t tw = (uint32_t)__builtin_amdgcn_readfirstlane((int)ev.tw);
    const int row = __builtin_amdgcn_readfirstlane(ev.row);
    const float c = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ev.c)));
    const float clin = __int_as_float(__builtin_amdgcn_readfirstlane(__float_as_int(ev.clin)));
    const int which = (int)(tw & 3u);
    const bool s1 = (tw & 8u) != 0;
    const int eg = (int)(tw >> 4);
    float hv[N];  // (selected as values: a choice between the variables themselves would keep all four in memory)
#pragma unroll
    for (int n = 0; n < N; ++n) {
      const float g0 = hG0.v[n], g1 = hG1.v[n], u0 = hU0.v[n], u1 = hU1.v[n];
      const float gs = s1 ? g1 : g0, us = s1 ? u1 : u0;
      hv[n] = which == 0 ? gs : us;
    }
    const float4 h = make_float4(hv[0], hv[1], hv[2], hv[3]);
    float* turn = s_turn + wv * D;
    asm volatile("" ::: "memory");  // (behind the previous reference's reads of the same LDS row)
    if (grp == eg) *reinterpret_cast<float4*>(turn + 4 * lig) = h;
    asm volatile("" ::: "memory");
    float x[KDD];
#pragma unroll
    for (int q = 0; q < KDD; ++q) {
      const int el = q * TRS_WAVE + lane;
      x[q] = turn[el < D ? el : 0];
    }
    asm volatile("" ::: "memory");
    float* dst = (which == 0 ? T.user : T.item) + (int64_t)row * D;
#pragma unroll
    for (int q = 0; q < KDD; ++q) {
      const int el = q * TRS_WAVE + lane;
      if (el < D) atomicAdd(dst + el, c * x[q]);
    }
    if (lane == 0) atomicAdd((which == 0 ? T.user_lin : T.item_lin) + row, clin);
  };
  // The overflow path: staged rows, as fwd_stage_kernel's tail applies them (rounds of DU rows loaded together past L1)
  auto load_round = [&](float (&x)[DU][KDD], int e0, int n_mine) {
#pragma unroll
    for (int k = 0; k < DU; ++k) {
      const bool has = e0 + k < n_mine;
      const DeferEntry en = s_list[wv * CAPW + (has ? e0 + k : 0)];
      const int64_t tk = has ? (int64_t)(en.tw >> 3) : 0;
      const float* src = ((en.tw & 3u) == 0 ? a.du : a.ustage) + tk * (int64_t)D;
#pragma unroll
      for (int q = 0; q < KDD; ++q) {
        const int el = q * TRS_WAVE + lane;
        x[k][q] = __hip_atomic_load(src + (el < D ? el : 0), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);  // past L1
      }
    }
  };
  auto apply_round = [&](float (&x)[DU][KDD], int e0, int n_mine) {
#pragma unroll
    for (int k = 0; k < DU; ++k) {
      if (e0 + k >= n_mine) continue;  // (wave-uniform)
      const DeferEntry en = s_list[wv * CAPW + e0 + k];
      const int which = (int)(en.tw & 3u);
      float* dst = (which == 0 ? T.user : T.item) + (int64_t)en.row * D;
#pragma unroll
      for (int q = 0; q < KDD; ++q) {
        const int el = q * TRS_WAVE + lane;
        if (el < D) atomicAdd(dst + el, en.c * x[k][q]);
      }
      if (lane == 0) atomicAdd((which == 0 ? T.user_lin : T.item_lin) + en.row, en.clin);
    }
  };
  // everything from entry `from` on: held references first, then the staged ones
  auto apply_rest = [&](int from) __attribute__((always_inline)) {
#pragma nounroll
    for (int e = from; e < n_held; ++e) apply_held(e);
    float x[DU][KDD];
    for (int e0 = from > n_held ? from : n_held; e0 < my_cnt; e0 += DU) {
      load_round(x, e0, my_cnt);
      apply_round(x, e0, my_cnt);
    }
  };

  int64_t t = wave * TPW + grp;
  // wave-uniform trip count: the wave's first group decides (its t is the smallest of the wave)
  const int64_t t_first = wave * TPW;
  const int64_t niter = t_first < B ? (B - t_first + stride - 1) / stride : 0;
  const int nph = __builtin_amdgcn_readfirstlane((int)((niter + 1) & ~(int64_t)1));  // even: surplus phases run on clamped, invalid triples
  // One look per wave per launch, at the start of phase ia = the third from the end, if the wave counted itself in at
  // least a phase earlier (fi < ia) and holds something to apply (ia = 1, a trip count of 3 or 4: slot 0 alone).  The
  // atomics follow behind the reduces of phases ia, ia + 1, ia + 2; what is left then goes to the tail.
  const int ia = nph - 3;
  const bool inloop = __builtin_amdgcn_readfirstlane(a.apply_in_loop != 0 && ia >= 1 && fi < (int64_t)ia) != 0;
  uint32_t seen_l = 0;
  int n_loop = 0;  // held references listed at the look (0: no look)
  auto look = [&](int ph) __attribute__((always_inline)) {  // behind phase ia - 1 = in front of phase ia's loads: nothing is consumed here
    if (inloop && ph == ia && __builtin_amdgcn_readfirstlane(n_held) > 0) {
      seen_l = __hip_atomic_load(a.sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      n_loop = __builtin_amdgcn_readfirstlane(n_held);
    }
  };
  auto consume = [&](int ph) __attribute__((always_inline)) {  // behind the reduce of phases ia, ia + 1, ia + 2
    if (n_loop > next_e && ph >= ia) {
      if (ph == ia) {
        complete = (int32_t)((uint32_t)__builtin_amdgcn_readfirstlane((int)seen_l) - a.sync_target) >= 0;
        if (TRS_FLAG_STEP_ORDER >= 2 && complete) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      }
      if (complete) {  // every workgroup of the launch is past its flagged triples: nobody reads these rows any more
#pragma nounroll
        for (int k = 0; k < FLAG_APPLY && next_e < n_loop; ++k) apply_held(next_e++);
      }
    }
  };

  // Reduce one triple whose rows are in registers (stores only: no waits on loads in flight).  hold: the triple belongs
  // to iteration SLOT = 0 | 1 — its flagged references keep their rows in hold slot SLOT instead of staging them.
  auto reduce = [&](TripleRows<VEC, K>& r, const TripleIds& id, int64_t tt, auto SLOT, bool hold) __attribute__((always_inline)) -> float {
    const bool live = id.valid && id.ok;
    if (id.valid && !id.ok && lig == 0 && a.err) atomicOr(a.err, 1);
    float pp = 0.f, pn = 0.f;
    if (NET == TRS_NET_FM) {
      // (u+i)^2 - (u^2 + i^2) per element, exactly the reference's power_of_sum - sum_of_power (fm.py:83-86)
#pragma unroll
      for (int n = 0; n < N; ++n) {
        const float sp_ = r.u.v[n] + r.pi.v[n], sn_ = r.u.v[n] + r.ni.v[n];
        const float uu = r.u.v[n] * r.u.v[n];
        pp += sp_ * sp_ - (uu + r.pi.v[n] * r.pi.v[n]);
        pn += sn_ * sn_ - (uu + r.ni.v[n] * r.ni.v[n]);
      }
    } else {
#pragma unroll
      for (int n = 0; n < N; ++n) {
        pp += r.u.v[n] * r.pi.v[n];
        pn += r.u.v[n] * r.ni.v[n];
      }
    }
    pp = trs_group_sum<G>(pp);
    pn = trs_group_sum<G>(pn);
    float sp, sn;
    if (NET == TRS_NET_FM) {
      sp = sigmoidf_((r.ul + r.pl) + 0.5f * pp);
      sn = sigmoidf_((r.ul + r.nl) + 0.5f * pn);
    } else {
      sp = (pp + r.ul) + r.pl;
      sn = (pn + r.ul) + r.nl;
    }
    float lval, dneg;
    trs_pair_loss(a.loss, sp, sn, lval, dneg);
    const float act = live ? dneg : 0.f;
    float gp = -act * a.inv_B, gn = act * a.inv_B;
    if (live && lig == 0) loss_acc += lval;
    if (NET == TRS_NET_FM) {
      gp = gp * ((1.0f - sp) * sp);
      gn = gn * ((1.0f - sn) * sn);
    }
    RowReg<VEC, K> g;
#pragma unroll
    for (int n = 0; n < N; ++n) g.v[n] = gp * r.pi.v[n] + gn * r.ni.v[n];
    {  // list the flagged references of the wave's triples (one lane per group speaks for its triple); outside every
      // divergent branch: the ballots and the wave-uniform counter need all lanes
      const bool lead = lig == 0 && live;
      const uint64_t mu = __ballot(lead && id.dup), mp = __ballot(lead && id.pdup), mn = __ballot(lead && id.ndup);
      const uint64_t below = ((uint64_t)1 << lane) - 1;
      const int cu = __popcll(mu), cp = __popcll(mp), cn = __popcll(mn);
      const int bu = wv * CAPW + my_cnt;
      my_cnt += cu + cp + cn;
      // a flagged reference BEHIND the first nf triples: n_flagged_dev does not describe these id / flag arrays (they
      // are not the ones trs_epoch_flags_ordered wrote) — the workgroup has counted itself in already, so this step is
      // not exact: err bit 3
      if (arrived && (cu + cp + cn) && lane == 0 && a.err) atomicOr(a.err, 8);
      constexpr int slot = decltype(SLOT)::value;
      const uint32_t tw = hold ? (4u | ((uint32_t)slot << 3) | ((uint32_t)grp << 4)) : ((uint32_t)tt << 3);
      const int bp = bu + cu, bn = bp + cp;
      if (lead && id.dup) s_list[bu + __popcll(mu & below)] = {tw, id.u, -a.lr, -a.lr * (gp + gn)};
      if (lead && id.pdup) s_list[bp + __popcll(mp & below)] = {tw | 1u, id.p, -a.lr * gp, -a.lr * gp};
      if (lead && id.ndup) s_list[bn + __popcll(mn & below)] = {tw | 2u, id.n, -a.lr * gn, -a.lr * gn};
    }
    if (hold) {  // (scalar) the slot's registers: every lane keeps its four floats, flagged or not
      if constexpr (decltype(SLOT)::value == 0) {
        hU0 = r.u;
        hG0 = g;
      } else {
        hU1 = r.u;
        hG1 = g;
      }
    }
    if (id.valid) {
      if (!hold && (id.pdup || id.ndup)) row_store<VEC, G, K>(r.u, a.ustage + tt * (int64_t)D, D, lig);
      if (live) {
        const float cp = -a.lr * gp, cn = -a.lr * gn;
        if (!id.pdup) {
          RowReg<VEC, K> o;
#pragma unroll
          for (int n = 0; n < N; ++n) o.v[n] = r.pi.v[n] + cp * r.u.v[n];
          row_store<VEC, G, K>(o, T.item + id.p * (int64_t)D, D, lig);
          if (lig == 0) T.item_lin[id.p] = r.pl + cp;
        }
        if (!id.ndup) {
          RowReg<VEC, K> o;
#pragma unroll
          for (int n = 0; n < N; ++n) o.v[n] = r.ni.v[n] + cn * r.u.v[n];
          row_store<VEC, G, K>(o, T.item + id.n * (int64_t)D, D, lig);
          if (lig == 0) T.item_lin[id.n] = r.nl + cn;
        }
      }
      if (id.dup || !live) {
        if (!hold) row_store<VEC, G, K>(g, a.du + tt * (int64_t)D, D, lig);
      } else {
        RowReg<VEC, K> un;
#pragma unroll
        for (int n = 0; n < N; ++n) un.v[n] = r.u.v[n] + (-a.lr) * g.v[n];
        row_store<VEC, G, K, (NTU & 2) != 0>(un, T.user + id.u * (int64_t)D, D, lig);
        if (lig == 0) T.user_lin[id.u] = r.ul + (-a.lr) * (gp + gn);
      }
    }
    return gp + gn;
  };

  // Software pipeline, unrolled by two so that nothing in flight is ever copied between registers: triple k's rows live
  // in the "even" or "odd" register set by parity; in triple k's phase the ids of k+2 are issued, the ids of k+1
  // consumed and its rows issued, then triple k is reduced.  Program order = issue order, so each wait covers only
  // loads older than everything that should stay in flight.
  TripleIds idE, idO;
  TripleRows<VEC, K> rE, rO;
  {
    constexpr std::integral_constant<int, 0> S0{};
    constexpr std::integral_constant<int, 1> S1{};
    RawIds wE = issue_ids<0, 3>(a, t);
    RawIds wO = issue_ids<0, 3>(a, t + stride);
    idE = finalize_ids<0>(a, wE);
    load_rows<VEC, G, K, true, OPT_SGD, NTU>(rE, T, a.o, idE, lig);
    if (fi == 0) arrive(0.f);
    for (int it = 0; it < nph; it += 2) {
      const bool first = it == 0;
      wE = issue_ids<0, 3>(a, t + 2 * stride);
      idO = finalize_ids<0>(a, wO);
      load_rows<VEC, G, K, true, OPT_SGD, NTU>(rO, T, a.o, idO, lig);
      const float pe = reduce(rE, idE, t, S0, first);
      if (first) n_held = my_cnt;  // (slot 0 is final)
      if ((int64_t)it + 1 == fi) arrive(pe);  // (the rows already in flight belong to triples without a flagged reference)
      consume(it);
      look(it + 1);  // (ia is odd: the phase that follows may be phase ia)

      wO = issue_ids<0, 3>(a, t + 3 * stride);
      idE = finalize_ids<0>(a, wE);
      load_rows<VEC, G, K, true, OPT_SGD, NTU>(rE, T, a.o, idE, lig);
      const float po = reduce(rO, idO, t + stride, S1, first);
      if (first) n_held = my_cnt;  // (both slots are final)
      if ((int64_t)it + 2 == fi) arrive(po);
      consume(it + 1);
      t += 2 * stride;
    }
    if (!arrived) arrive(loss_acc);  // a wave with fewer iterations than fi (the batch's tail; a batch left in its order)
  }
  const float wl = trs_wave_sum(loss_acc);
  if (lane == 0) s_loss[wv] = wl;
  const int n_in_loop = next_e;  // (K1_APPLY_STATS)
  if (my_cnt > next_e) {  // (wave-uniform) what the loop has not applied: everything, without the in-loop path
    const uint32_t seen = __hip_atomic_load(a.sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    complete = (int32_t)((uint32_t)__builtin_amdgcn_readfirstlane((int)seen) - a.sync_target) >= 0;
    if (complete) {  // every workgroup of the launch is past its flagged triples: nobody reads these rows any more
      if (TRS_FLAG_STEP_ORDER >= 2) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
      apply_rest(next_e);
      next_e = my_cnt;
    } else if (lane == 0) {
      s_left = 1;  // (not yet: the workgroup waits below)
    }
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");  // this wave's row loads and staging stores are done
  __syncthreads();
  if (threadIdx.x == 0) {
    float L = 0.f;
#pragma unroll
    for (int w = 0; w < NWV; ++w) L += s_loss[w];
    if (L != 0.f) atomicAdd(a.loss_sum, L);
  }
  // K1_APPLY_STATS (tests): every reference of the wave's list is applied exactly once, in the loop or behind it
  if (a.apply_stats && lane == 0) {
    uint32_t* st = a.sync + (TRS_SYNC_WORDS - 2);
    if (n_in_loop) (void)__hip_atomic_fetch_add(st, (uint32_t)n_in_loop, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (my_cnt > n_in_loop)
      (void)__hip_atomic_fetch_add(st + 1, (uint32_t)(my_cnt - n_in_loop), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  }
  if (!s_left) return;  // (workgroup-uniform: written before the barrier above)
  if (threadIdx.x == 0) {
    // counted in long ago, and so has everybody else: one look at the counter — and a bounded wait if it is not so
    // (50 ms of s_memrealtime, none at all once a launch has timed out: err bit 2 is sticky until the host reads it)
    const uint64_t t_start = __builtin_amdgcn_s_memrealtime();
    const uint64_t limit = (a.err && (__hip_atomic_load(a.err, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & 4)) ? 0ull : 5000000ull;
    while ((int32_t)(__hip_atomic_load(a.sync, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) - a.sync_target) < 0) {
      __builtin_amdgcn_s_sleep(6);
      if (__builtin_amdgcn_s_memrealtime() - t_start > limit) {
        if (a.err) atomicOr(a.err, 4);
        break;
      }
    }
  }
  __syncthreads();
  // every row read of the step is behind us, chip-wide
  if (TRS_FLAG_STEP_ORDER >= 2) __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
  apply_rest(next_e);
}

// Workgroups of flag_step_kernel that are certainly resident at once: (occupancy - 1) per CU, at most K1_WGS_PER_CU
// (fast_step.hip defer_resident_cap: the API's answer can be one too high).
template <typename KernelT>
static int64_t flag_resident_cap(KernelT kernel) {
  int occ = 0, dev = 0, cus = 0;
  if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&occ, kernel, TRS_BLOCK, 0) != hipSuccess) return 0;
  if (hipGetDevice(&dev) != hipSuccess ||
      hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess)
    return 0;
  const int want = trs_tuning().k1_wgs_per_cu;
  const int per_cu = occ - 1 < want ? occ - 1 : want;
  return per_cu > 0 ? (int64_t)per_cu * cus : 0;
}

template <int NET>
static int launch_flag_step(const FastArgs& a, const RowCfg& c, int ntu, int64_t grid, hipStream_t s) {
  const dim3 gr((unsigned)grid), bl(TRS_BLOCK);
  return for_whole_row_shape(c, [&](auto V, auto G, auto K) {
    constexpr int GG = G();
    if (V() * GG * K() != a.T.D) return 1;  // ragged rows
    static const int64_t cap = flag_resident_cap(flag_step_kernel<NET, GG, 0>);  // (NTU changes no register class: asked once)
    if (grid > cap) return 1;
    FastArgs b = a;
    b.sync_target = a.sync_base + (uint32_t)grid;
    b.apply_in_loop = trs_tuning().k1_apply_in_loop != 0;
    b.apply_stats = trs_tuning().k1_apply_stats != 0;
    if (ntu == 1) hipLaunchKernelGGL((flag_step_kernel<NET, GG, 1>), gr, bl, 0, s, b);
    else if (ntu == 3) hipLaunchKernelGGL((flag_step_kernel<NET, GG, 3>), gr, bl, 0, s, b);
    else hipLaunchKernelGGL((flag_step_kernel<NET, GG, 0>), gr, bl, 0, s, b);
    TRS_CHECK_LAUNCH("flag_step_kernel");
    return TRS_OK;
  });
}

int trs_launch_flag_step(int net, const FastArgs& a, const RowCfg& c, int ntu, int64_t grid, void* stream) {
#ifdef TRS_K1_STAMPS  // the diagnostic build times fwd_stage_kernel's workgroups (tools/k1_stamps.py)
  return 1;
#endif
  if (trs_tuning().k1_flag_kernel == 0 || !a.nflag || !a.sync) return 1;
  // A batch the presort reports as left in its order (nf = B: more than 12 288 misplaced triples, presort.hip phase D)
  // makes every workgroup wait for the grid behind its loop: that is the old kernel's form, which polls flag lines
  // and not the counter.  The host does not see nf; a shuffled batch with a share f of flagged triples misplaces
  // B f (1 - f) <= B / 4 of them, so batches up to 4 * 12 288 come here and larger ones go to the old kernel.  (A
  // batch that reports nf = B all the same is still exact here: the bounded wait.  An entry keeps t in 29 bits.)
  if (a.B > 4 * 12288) return 1;
  hipStream_t s = (hipStream_t)stream;
  return net == TRS_NET_FM ? launch_flag_step<TRS_NET_FM>(a, c, ntu, grid, s)
                           : launch_flag_step<TRS_NET_LINEAR>(a, c, ntu, grid, s);
}

}  // namespace trs
