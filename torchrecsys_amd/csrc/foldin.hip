// foldin.hip — fold-in of unseen users: a few epochs of per-visit SGD on one new user row per item history, the item
// side frozen (model.py fold_in_users / recommend_for_histories; the update rule is the contract in include/trs.h
// "fold-in", the design in DESIGN.md 4.12).  The item side of the problem, fold_in_items_kernel, follows below it.
//
// fold_in_kernel<G, DEPTH>  one user per aligned lane group of G = Dp / 4 lanes (Dp = the folded buffer's row width), so a
//                           wave holds 64 / G users.  Lane l keeps columns 4l .. 4l+3 of u in registers, every lane of a
//                           group the same b and loss sum.  A visit reads the lane's 16 bytes of S_p and S_n and the two
//                           constants, forms both dot products (trs_group_sum<G>), and updates u and b in registers; the
//                           rows are stored once, after the last epoch.  No LDS, no atomics but the error flag's.
//   schedule   The ids of a visit (p, n) do not depend on u.  Once per G visits the lanes of a group derive the ids of
//              G visits at once — lane l the Feistel position, the history item and the negative draw of visit v0 + l —
//              and hand them out with a shuffle when the visit's rows are requested: the Philox rounds and the binary
//              searches of the rejection run G wide instead of once per visit on every lane.
//   ring       DEPTH visits' rows are kept requested: slot s of a ring in registers (fully unrolled, so every slot is a
//              fixed set of VGPRs) is refilled with visit j + DEPTH as soon as visit j has been taken out of it, before
//              j's update is computed.  DEPTH = 1 has only the next visit under way.
//   lock-step  the groups of a wave have different history lengths; every lane runs to the longest one of its wave
//              with its visits predicated off (ok = 0: row 0 is read and dropped, no update) — the shuffles of the dot
//              products and of the schedule need the whole wave.  No early return.
#include "trs_common.h"

namespace {

struct FoldinArgs {
  const float* S;  // (n_pad, Dp)
  const float* c;  // (n_pad)
  int64_t n_items;
  const int64_t* off;
  const int32_t* items;
  int64_t n_new;
  int net, loss, epochs, shuffle, D;
  float lr, l2;
  uint64_t seed;
  TrsSampler sampler;
  float* U;         // (n_new, D)
  float* b;         // (n_new)
  float* loss_out;  // (epochs, n_new) or NULL
  int32_t* err;     // or NULL
};

static inline int fi_dp(int D) {  // the folded buffer's row width (trs_item_fold_bytes)
  int p = 16;
  while (p < D) p <<= 1;
  return p;
}

template <int G, int DEPTH>
__global__ __launch_bounds__(TRS_BLOCK) void fold_in_kernel(const FoldinArgs a) {
  constexpr int Dp = 4 * G;
  const int l = threadIdx.x & (G - 1);
  const int64_t h = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) / G;
  const bool live = h < a.n_new;
  int64_t off0 = 0, n_h = 0;
  if (live) {
    off0 = a.off[h];
    n_h = a.off[h + 1] - off0;
    if (n_h < 0) n_h = 0;
  }
  long long nmax = n_h;  // the longest history of the wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long other = __shfl_xor(nmax, o, 64);
    nmax = other > nmax ? other : nmax;
  }
  const int hb = trs_feistel_half_bits(n_h);
  const bool fm = a.net == TRS_NET_FM;
  const float lr = a.lr, l2 = a.l2;
  const float* Sl = a.S + 4 * l;

  float4 u = make_float4(0.f, 0.f, 0.f, 0.f);
  float b = 0.f;

  for (int e = 0; e < a.epochs; ++e) {
    const trs_u4 kw = trs_philox4x32_10((uint64_t)e, a.seed + TRS_CANDIDATE_KEY_STEP);
    const uint64_t key = (((uint64_t)kw.y << 32) | (uint64_t)kw.x) | 1ull;
    float lsum = 0.f;
    int ps = -1, ns = -1;  // this lane's entry of the schedule chunk: visit (v & ~(G-1)) + l; -1 = no visit

    float4 rp[DEPTH], rn[DEPTH];
    float cp[DEPTH], cn[DEPTH];
    bool ok[DEPTH];

    // request the rows of visit v into (qp, kp, qn, kn, good); v is wave-uniform
    auto fetch = [&](long long v, float4& qp, float& kp, float4& qn, float& kn, bool& good) {
      if ((v & (G - 1)) == 0 && v < nmax) {  // a new chunk of G visits: lane l derives visit v + l
        const int64_t mv = v + l;
        ps = -1;
        ns = -1;
        if (mv < n_h) {
          const int64_t r = a.shuffle ? trs_feistel_perm(mv, n_h, key, hb) : mv;
          const int32_t p = a.items[off0 + r];
          if ((uint64_t)(int64_t)p < (uint64_t)a.n_items) {
            ns = (int)trs_sample_neg_opt(a.seed, ((uint64_t)e << 32) | (uint64_t)r, h, p, a.n_items, a.sampler);
            ps = p;
          } else if (a.err) {
            atomicOr(a.err, 1);  // never an address: the visit is skipped
          }
        }
      }
      const int src = (int)(v & (G - 1));
      const int p = __shfl(ps, src, G), n = __shfl(ns, src, G);
      good = p >= 0 && v < n_h;
      // No branch around the loads: a visit that is off reads row 0 (always there, n_items >= 2) and its values are
      // never used.  With the loads under a branch the compiler cannot count the requests behind a slot and waits for
      // all of them (vmcnt(0)) at every trip, which empties the ring.
      const int64_t pa = good ? p : 0, na = good ? n : 0;
      qp = *reinterpret_cast<const float4*>(Sl + pa * Dp);
      qn = *reinterpret_cast<const float4*>(Sl + na * Dp);
      kp = a.c[pa];
      kn = a.c[na];
    };

#pragma unroll
    for (int s = 0; s < DEPTH; ++s) fetch(s, rp[s], cp[s], rn[s], cn[s], ok[s]);

    for (long long j = 0; j < nmax; j += DEPTH) {
#pragma unroll
      for (int s = 0; s < DEPTH; ++s) {
        const float4 xp = rp[s], xn = rn[s];
        const float yp = cp[s], yn = cn[s];
        const bool good = ok[s];
        fetch(j + s + DEPTH, rp[s], cp[s], rn[s], cn[s], ok[s]);

        float dp = u.x * xp.x;
        dp += u.y * xp.y;
        dp += u.z * xp.z;
        dp += u.w * xp.w;
        float dn = u.x * xn.x;
        dn += u.y * xn.y;
        dn += u.z * xn.z;
        dn += u.w * xn.w;
        dp = trs_group_sum<G>(dp);
        dn = trs_group_sum<G>(dn);
        if (good) {
          const float zp = (dp + b) + yp, zn = (dn + b) + yn;
          const float sp = fm ? 1.0f / (1.0f + expf(-zp)) : zp;
          const float sn = fm ? 1.0f / (1.0f + expf(-zn)) : zn;
          float value, dneg;
          trs_pair_loss(a.loss, sp, sn, value, dneg);
          const float wp = fm ? sp * (1.0f - sp) : 1.0f;
          const float wn = fm ? sn * (1.0f - sn) : 1.0f;
          const float gp = -dneg * wp, gn = dneg * wn;
          u.x = u.x - lr * ((gp * xp.x + gn * xn.x) + l2 * u.x);
          u.y = u.y - lr * ((gp * xp.y + gn * xn.y) + l2 * u.y);
          u.z = u.z - lr * ((gp * xp.z + gn * xn.z) + l2 * u.z);
          u.w = u.w - lr * ((gp * xp.w + gn * xn.w) + l2 * u.w);
          b = b - lr * ((gp + gn) + l2 * b);
          lsum += value;
        }
      }
    }
    if (live && l == 0 && a.loss_out) a.loss_out[(int64_t)e * a.n_new + h] = n_h > 0 ? lsum / (float)n_h : 0.f;
  }

  if (live) {
    const int d0 = 4 * l;
    float* row = a.U + h * (int64_t)a.D + d0;
    if (d0 + 4 <= a.D && (a.D & 3) == 0 && (reinterpret_cast<uintptr_t>(a.U) & 15) == 0) {
      *reinterpret_cast<float4*>(row) = u;
    } else if (d0 < a.D) {
      row[0] = u.x;
      if (d0 + 1 < a.D) row[1] = u.y;
      if (d0 + 2 < a.D) row[2] = u.z;
      if (d0 + 3 < a.D) row[3] = u.w;
    }
    if (l == 0) a.b[h] = b;
  }
}

template <int G>
static void launch_fold_in(int depth, const FoldinArgs& a, unsigned blocks, hipStream_t s) {
  switch (depth) {
    case 1: hipLaunchKernelGGL((fold_in_kernel<G, 1>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
    case 2: hipLaunchKernelGGL((fold_in_kernel<G, 2>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
    case 4: hipLaunchKernelGGL((fold_in_kernel<G, 4>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL((fold_in_kernel<G, 8>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
  }
}

}  // namespace

extern "C" int trs_fold_in_users(int net, const void* fold_dev, int64_t fold_bytes, int64_t n_items, int32_t D,
                                 const trs_csr* hist, int32_t loss, int32_t epochs, float lr, float l2, uint64_t seed,
                                 int32_t shuffle, int32_t reject_seen, int32_t max_tries, float* user_out_dev,
                                 float* user_lin_out_dev, float* loss_out_dev, int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_fold_in_users";
  TRS_REQUIRE(net == TRS_NET_LINEAR || net == TRS_NET_FM, "%s: net must be TRS_NET_LINEAR or TRS_NET_FM", who);
  TRS_REQUIRE(D >= 1 && D <= TRS_RETRIEVE_DMAX, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(n_items >= 2 && n_items <= INT32_MAX, "%s: n_items=%lld outside 2..2^31-1", who, (long long)n_items);
  const int64_t need = trs_item_fold_bytes(n_items, D);
  TRS_REQUIRE(fold_dev && fold_bytes >= need, "%s: fold buffer too small (%lld < %lld)", who, (long long)fold_bytes,
              (long long)need);
  TRS_REQUIRE(loss == TRS_LOSS_HINGE || loss == TRS_LOSS_BPR, "%s: loss=%d is not TRS_LOSS_HINGE or TRS_LOSS_BPR", who,
              loss);
  TRS_REQUIRE(epochs >= 1 && epochs <= 1024, "%s: epochs=%d outside 1..1024", who, epochs);
  TRS_REQUIRE(lr > 0.f && lr <= 3.402823466e+38f, "%s: lr must be finite and > 0", who);
  TRS_REQUIRE(l2 >= 0.f && l2 <= 3.402823466e+38f, "%s: l2 must be finite and >= 0", who);
  TRS_REQUIRE(max_tries >= 0 && max_tries <= 64, "%s: max_tries=%d outside 0..64", who, max_tries);
  TRS_REQUIRE(!reject_seen || max_tries >= 1, "%s: reject_seen needs max_tries >= 1", who);
  TRS_REQUIRE(hist != nullptr && hist->n_rows >= 0, "%s: history CSR is NULL", who);
  const int depth = trs_tuning().foldin_depth;
  TRS_REQUIRE(depth == 1 || depth == 2 || depth == 4 || depth == 8, "%s: FOLDIN_DEPTH=%d is not 1, 2, 4 or 8", who,
              depth);
  if (hist->n_rows == 0) return TRS_OK;
  TRS_REQUIRE(hist->off && hist->items, "%s: history CSR has NULL arrays", who);
  TRS_REQUIRE(user_out_dev && user_lin_out_dev, "%s: user_out/user_lin_out is NULL", who);

  const int Dp = fi_dp(D), G = Dp / 4;
  const int64_t n_pad = need / ((int64_t)(Dp + 1) * 4);
  const int64_t blocks = (hist->n_rows + TRS_BLOCK / G - 1) / (TRS_BLOCK / G);
  TRS_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many users in one call", who);
  FoldinArgs a = {};
  a.S = (const float*)fold_dev;
  a.c = a.S + n_pad * Dp;
  a.n_items = n_items;
  a.off = hist->off;
  a.items = hist->items;
  a.n_new = hist->n_rows;
  a.net = net;
  a.loss = loss;
  a.epochs = epochs;
  a.shuffle = shuffle != 0;
  a.D = D;
  a.lr = lr;
  a.l2 = l2;
  a.seed = seed;
  a.sampler = TrsSampler{1, 0, max_tries, reject_seen ? hist->off : nullptr, reject_seen ? hist->items : nullptr,
                         nullptr, 0, hist->n_rows};
  a.U = user_out_dev;
  a.b = user_lin_out_dev;
  a.loss_out = loss_out_dev;
  a.err = err_flag_dev;
  hipStream_t s = (hipStream_t)stream;
  switch (G) {
    case 4: launch_fold_in<4>(depth, a, (unsigned)blocks, s); break;
    case 8: launch_fold_in<8>(depth, a, (unsigned)blocks, s); break;
    case 16: launch_fold_in<16>(depth, a, (unsigned)blocks, s); break;
    case 32: launch_fold_in<32>(depth, a, (unsigned)blocks, s); break;
    default: launch_fold_in<64>(depth, a, (unsigned)blocks, s); break;
  }
  TRS_CHECK_LAUNCH("fold_in_kernel");
  return TRS_OK;
}

// ---------------------------------------------------------------------------------------------- item fold-in
// fold_in_items_kernel<G, DEPTH, VEC>  the item side of the same problem (model.py fold_in_items; contract: include/trs.h
//                           "item fold-in", design: DESIGN.md 4.15): one new ITEM per aligned lane group, its row v and
//                           its metadata part T as four columns per lane, beta, kappa and the loss sum on every lane of
//                           the group.  A visit has one shape whichever role the new item plays — a user row, the user's
//                           constant, a catalogue fold row, its constant, and which of the two scores is the positive's —
//                           so ring and lock-step are those of fold_in_kernel, the schedule is derived lane-parallel
//                           in chunks of G visits like its (but at one place per ring trip, see the loop), and the
//                           loop body is written once.  The visit's role (t == 0: the new item is the positive) is
//                           wave-uniform: it is the visit number modulo 1 + nu, kept as a counter.
//   user rows  come from the unpadded user table (row stride D).  VEC (D % 4 == 0 and a 16-byte aligned base): one
//              16-byte load, a lane whose columns are >= D reads column 0 and drops it.  Otherwise four 4-byte loads,
//              each column >= D redirected to column 0 and dropped.  No branch around a load in either.
namespace {

struct ItemFoldinArgs {
  const float* U;     // (n_users, D), unpadded
  const float* ulin;  // (n_users)
  int64_t n_users;
  const float* S;  // (n_pad, Dp) the catalogue's fold
  const float* c;  // (n_pad)
  int64_t n_items;
  const float* T;      // (n_pad_new, Dp) the new items' metadata parts
  const float* kappa;  // (n_pad_new)
  const int64_t* off;
  const int32_t* users;  // the histories' user ids
  int64_t n_new;
  const int32_t* su;  // (n_stream) train users
  const int32_t* si;  // (n_stream) train items
  int64_t n_stream;
  int net, loss, epochs, shuffle, D, nu, reject, max_tries;
  float lr, l2;
  uint64_t seed;
  TrsSampler sampler;  // t == 0: the model's seen CSR (or none)
  float* V;            // (n_new, D)
  float* b;            // (n_new)
  float* loss_out;     // (epochs, n_new) or NULL
  int32_t* err;        // or NULL
};

constexpr uint64_t FI_TRY_STEP = 0x9E3779B97F4A7C15ull;  // candidate k of a draw: the step of trs_sample_neg_opt

template <int G, int DEPTH, bool VEC>
__global__ __launch_bounds__(TRS_BLOCK) void fold_in_items_kernel(const ItemFoldinArgs a) {
  constexpr int Dp = 4 * G;
  const int l = threadIdx.x & (G - 1);
  const int d0 = 4 * l;
  const int64_t h = ((int64_t)blockIdx.x * TRS_BLOCK + threadIdx.x) / G;
  const bool live = h < a.n_new;
  int64_t off0 = 0, n_h = 0;
  if (live) {
    off0 = a.off[h];
    n_h = a.off[h + 1] - off0;
    if (n_h < 0) n_h = 0;
  }
  const int per = 1 + a.nu;  // visits per history position
  const int64_t nv = n_h * per;
  long long nmax = nv;  // the longest trip count of the wave
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const long long other = __shfl_xor(nmax, o, 64);
    nmax = other > nmax ? other : nmax;
  }
  const int hb = trs_feistel_half_bits(n_h);
  const bool fm = a.net == TRS_NET_FM;
  const float lr = a.lr, l2 = a.l2;
  const float* Sl = a.S + d0;
  const int D = a.D;

  const int64_t hr = live ? h : 0;  // row 0 is always there (n_new >= 1)
  const float4 T = *reinterpret_cast<const float4*>(a.T + hr * Dp + d0);
  const float kappa = a.kappa[hr];
  float4 v = make_float4(0.f, 0.f, 0.f, 0.f);
  float beta = 0.f;

  // is user `u` in this item's history?
  auto in_history = [&](int64_t u) __attribute__((always_inline)) {
    int64_t lo = off0, hi = off0 + n_h;
    while (lo < hi) {
      const int64_t mid = (lo + hi) >> 1;
      const int64_t x = a.users[mid];
      if (x == u) return true;
      if (x < u) lo = mid + 1; else hi = mid;
    }
    return false;
  };

  // this lane's four columns of user row u (a valid row), columns >= D as 0
  auto user_row = [&](int64_t u) __attribute__((always_inline)) {
    const float* row = a.U + u * (int64_t)D;
    float4 x;
    if constexpr (VEC) {
      const bool in = d0 < D;  // D % 4 == 0: a lane's four columns are inside together
      x = *reinterpret_cast<const float4*>(row + (in ? d0 : 0));
      if (!in) x = make_float4(0.f, 0.f, 0.f, 0.f);
    } else {
      const float x0 = row[d0 < D ? d0 : 0], x1 = row[d0 + 1 < D ? d0 + 1 : 0];
      const float x2 = row[d0 + 2 < D ? d0 + 2 : 0], x3 = row[d0 + 3 < D ? d0 + 3 : 0];
      x = make_float4(d0 < D ? x0 : 0.f, d0 + 1 < D ? x1 : 0.f, d0 + 2 < D ? x2 : 0.f, d0 + 3 < D ? x3 : 0.f);
    }
    return x;
  };

  for (int e = 0; e < a.epochs; ++e) {
    const trs_u4 kw = trs_philox4x32_10((uint64_t)e, a.seed + TRS_CANDIDATE_KEY_STEP);
    const uint64_t key = (((uint64_t)kw.y << 32) | (uint64_t)kw.x) | 1ull;
    float lsum = 0.f;
    int tcur = 0;  // sub-visit t of the visit being taken out of the ring (wave-uniform)
    // The schedule: chunk k = visits kG .. kG + G - 1, lane l the entry of visit kG + l (user, catalogue item; user -1 =
    // no visit).  NCH chunks are held, as many as a trip of the ring requests from (DEPTH / G, at least one), and they
    // are derived at ONE place per trip, before its requests: derived inside every request the body is 2 DEPTH copies
    // of the Philox, Feistel and search code, too large to unroll at DEPTH = 8, and the ring then lives in scratch.
    constexpr int NCH = DEPTH > G ? DEPTH / G : 1;
    int us[NCH], os[NCH];

    float4 ru[DEPTH], rs[DEPTH];
    float cu[DEPTH], cs[DEPTH];
    bool ok[DEPTH];

    // lane l derives visit base + l (base wave-uniform, a multiple of G)
    auto derive = [&](long long base, int& uo, int& oo) __attribute__((always_inline)) {
      if (base >= nmax) return;
      const int64_t mv = base + l;
      uo = -1;
      oo = 0;
      if (mv < nv) {
        const int64_t q = mv / per;
        const int t = (int)(mv - q * per);
        const int64_t r = a.shuffle ? trs_feistel_perm(q, n_h, key, hb) : q;
        const uint64_t ctr = ((uint64_t)e << 32) | (uint64_t)r;
        int64_t u, o = 0;
        if (t == 0) {  // the new item is the positive of one of its own users
          u = a.users[off0 + r];
          if ((uint64_t)u < (uint64_t)a.n_users)
            o = trs_sample_neg_opt(a.seed, ctr, u, a.n_items, a.n_items + 1, a.sampler);
        } else {  // ... the negative of a train interaction
          const uint64_t kt = a.seed + (uint64_t)(1 + t) * TRS_CANDIDATE_KEY_STEP;
          const int tries = a.reject ? a.max_tries : 1;
          int64_t idx = 0;
          u = -1;
          for (int k = 0; k < tries; ++k) {
            const trs_u4 w = trs_philox4x32_10(ctr, kt + (uint64_t)k * FI_TRY_STEP);
            idx = (int64_t)trs_mulhi64(((uint64_t)w.y << 32) | (uint64_t)w.x, (uint64_t)a.n_stream);
            u = a.su[idx];
            if (!a.reject || !in_history(u)) break;
          }
          o = a.si[idx];
        }
        if ((uint64_t)u < (uint64_t)a.n_users && (uint64_t)o < (uint64_t)a.n_items) {
          uo = (int)u;
          oo = (int)o;
        } else if (a.err) {
          atomicOr(a.err, 1);  // never an address: the visit is skipped
        }
      }
    };

    // request the rows of visit vi (wave-uniform), whose schedule entry is in (uc, oc), into (qu, ku, qs, ks, good)
    auto fetch = [&](long long vi, int uc, int oc, float4& qu, float& ku, float4& qs, float& ks, bool& good)
        __attribute__((always_inline)) {
      const int src = (int)(vi & (G - 1));
      const int u = __shfl(uc, src, G), o = __shfl(oc, src, G);
      good = u >= 0 && vi < nv;
      // no branch around the loads (see fold_in_kernel): a visit that is off reads row 0 of both tables
      const int64_t ua = good ? u : 0, oa = good ? o : 0;
      qu = user_row(ua);
      qs = *reinterpret_cast<const float4*>(Sl + oa * Dp);
      ku = a.ulin[ua];
      ks = a.c[oa];
    };

#pragma unroll
    for (int k = 0; k < NCH; ++k) {
      us[k] = -1;
      os[k] = 0;
      derive((long long)k * G, us[k], os[k]);
    }
#pragma unroll
    for (int s = 0; s < DEPTH; ++s) fetch(s, us[(s / G) % NCH], os[(s / G) % NCH], ru[s], cu[s], rs[s], cs[s], ok[s]);

    for (long long j = 0; j < nmax; j += DEPTH) {
      // this trip requests visits j + DEPTH .. j + 2 DEPTH - 1; every earlier visit has been requested
      if (DEPTH >= G || ((j + DEPTH) & (G - 1)) == 0) {
#pragma unroll
        for (int k = 0; k < NCH; ++k) derive(j + DEPTH + (long long)k * G, us[k], os[k]);
      }
#pragma unroll
      for (int s = 0; s < DEPTH; ++s) {
        const float4 xu = ru[s], xs = rs[s];
        const float au = cu[s], co = cs[s];
        const bool good = ok[s];
        fetch(j + s + DEPTH, us[(s / G) % NCH], os[(s / G) % NCH], ru[s], cu[s], rs[s], cs[s], ok[s]);
        const bool positive = tcur == 0;
        tcur = tcur + 1 == per ? 0 : tcur + 1;

        const float4 x = make_float4(v.x + T.x, v.y + T.y, v.z + T.z, v.w + T.w);
        float dn = xu.x * x.x;
        dn += xu.y * x.y;
        dn += xu.z * x.z;
        dn += xu.w * x.w;
        float dold = xu.x * xs.x;
        dold += xu.y * xs.y;
        dold += xu.z * xs.z;
        dold += xu.w * xs.w;
        float vt = v.x * T.x;
        vt += v.y * T.y;
        vt += v.z * T.z;
        vt += v.w * T.w;
        dn = trs_group_sum<G>(dn);
        dold = trs_group_sum<G>(dold);
        if (fm) vt = trs_group_sum<G>(vt);  // wave-uniform
        if (good) {
          const float cnew = fm ? (beta + kappa) + vt : beta + kappa;
          const float znew = (dn + au) + cnew, zold = (dold + au) + co;
          const float snew = fm ? 1.0f / (1.0f + expf(-znew)) : znew;
          const float sold = fm ? 1.0f / (1.0f + expf(-zold)) : zold;
          float value, dneg;
          trs_pair_loss(a.loss, positive ? snew : sold, positive ? sold : snew, value, dneg);
          const float w = fm ? snew * (1.0f - snew) : 1.0f;
          const float g = (positive ? -dneg : dneg) * w;
          const float4 dir = fm ? make_float4(xu.x + T.x, xu.y + T.y, xu.z + T.z, xu.w + T.w) : xu;
          v.x = v.x - lr * ((g * dir.x) + l2 * v.x);
          v.y = v.y - lr * ((g * dir.y) + l2 * v.y);
          v.z = v.z - lr * ((g * dir.z) + l2 * v.z);
          v.w = v.w - lr * ((g * dir.w) + l2 * v.w);
          beta = beta - lr * (g + l2 * beta);
          lsum += value;
        }
      }
    }
    if (live && l == 0 && a.loss_out) a.loss_out[(int64_t)e * a.n_new + h] = nv > 0 ? lsum / (float)nv : 0.f;
  }

  if (live) {
    float* row = a.V + h * (int64_t)D + d0;
    if (VEC) {
      if (d0 < D) *reinterpret_cast<float4*>(row) = v;
    } else if (d0 < D) {
      row[0] = v.x;
      if (d0 + 1 < D) row[1] = v.y;
      if (d0 + 2 < D) row[2] = v.z;
      if (d0 + 3 < D) row[3] = v.w;
    }
    if (l == 0) a.b[h] = beta;
  }
}

template <int G, bool VEC>
static void launch_fold_in_items(int depth, const ItemFoldinArgs& a, unsigned blocks, hipStream_t s) {
  switch (depth) {
    case 1: hipLaunchKernelGGL((fold_in_items_kernel<G, 1, VEC>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
    case 2: hipLaunchKernelGGL((fold_in_items_kernel<G, 2, VEC>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
    case 4: hipLaunchKernelGGL((fold_in_items_kernel<G, 4, VEC>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
    default: hipLaunchKernelGGL((fold_in_items_kernel<G, 8, VEC>), dim3(blocks), dim3(TRS_BLOCK), 0, s, a); break;
  }
}
template <bool VEC>
static void launch_fold_in_items_g(int G, int depth, const ItemFoldinArgs& a, unsigned blocks, hipStream_t s) {
  switch (G) {
    case 4: launch_fold_in_items<4, VEC>(depth, a, blocks, s); break;
    case 8: launch_fold_in_items<8, VEC>(depth, a, blocks, s); break;
    case 16: launch_fold_in_items<16, VEC>(depth, a, blocks, s); break;
    case 32: launch_fold_in_items<32, VEC>(depth, a, blocks, s); break;
    default: launch_fold_in_items<64, VEC>(depth, a, blocks, s); break;
  }
}

}  // namespace

extern "C" int trs_fold_in_items(int net, const trs_tables* tables, const void* fold_dev, int64_t fold_bytes,
                                 int64_t n_items, const void* new_fold_dev, int64_t new_fold_bytes, const trs_csr* hist,
                                 const int32_t* stream_user_dev, const int32_t* stream_item_dev, int64_t n_stream,
                                 const trs_csr* seen, int32_t loss, int32_t epochs, float lr, float l2,
                                 int32_t negative_visits, uint64_t seed, int32_t shuffle, int32_t reject_seen,
                                 int32_t max_tries, float* item_out_dev, float* item_lin_out_dev, float* loss_out_dev,
                                 int32_t* err_flag_dev, void* stream) {
  const char* who = "trs_fold_in_items";
  TRS_REQUIRE(net == TRS_NET_LINEAR || net == TRS_NET_FM, "%s: net must be TRS_NET_LINEAR or TRS_NET_FM", who);
  TRS_REQUIRE(tables != nullptr, "%s: tables is NULL", who);
  const int32_t D = tables->D;
  TRS_REQUIRE(D >= 1 && D <= TRS_RETRIEVE_DMAX, "%s: D=%d outside 1..%d", who, D, TRS_RETRIEVE_DMAX);
  TRS_REQUIRE(tables->user && tables->user_lin, "%s: user table / 1-wide user table is NULL", who);
  TRS_REQUIRE(tables->n_users >= 1 && tables->n_users <= INT32_MAX, "%s: n_users=%lld outside 1..2^31-1", who,
              (long long)tables->n_users);
  TRS_REQUIRE(n_items >= 2 && n_items < INT32_MAX, "%s: n_items=%lld outside 2..2^31-2", who, (long long)n_items);
  const int64_t need = trs_item_fold_bytes(n_items, D);
  TRS_REQUIRE(fold_dev && fold_bytes >= need, "%s: fold buffer too small (%lld < %lld)", who, (long long)fold_bytes,
              (long long)need);
  TRS_REQUIRE(loss == TRS_LOSS_HINGE || loss == TRS_LOSS_BPR, "%s: loss=%d is not TRS_LOSS_HINGE or TRS_LOSS_BPR", who,
              loss);
  TRS_REQUIRE(epochs >= 1 && epochs <= 1024, "%s: epochs=%d outside 1..1024", who, epochs);
  TRS_REQUIRE(lr > 0.f && lr <= 3.402823466e+38f, "%s: lr must be finite and > 0", who);
  TRS_REQUIRE(l2 >= 0.f && l2 <= 3.402823466e+38f, "%s: l2 must be finite and >= 0", who);
  TRS_REQUIRE(max_tries >= 0 && max_tries <= 64, "%s: max_tries=%d outside 0..64", who, max_tries);
  TRS_REQUIRE(!reject_seen || max_tries >= 1, "%s: reject_seen needs max_tries >= 1", who);
  TRS_REQUIRE(negative_visits >= 0 && negative_visits <= 8, "%s: negative_visits=%d outside 0..8", who, negative_visits);
  TRS_REQUIRE(n_stream >= 0, "%s: n_stream=%lld is negative", who, (long long)n_stream);
  TRS_REQUIRE(negative_visits == 0 || (n_stream > 0 && stream_user_dev && stream_item_dev),
              "%s: negative_visits=%d needs train interactions (n_stream=%lld, stream NULL or empty)", who,
              negative_visits, (long long)n_stream);
  TRS_REQUIRE(!seen || (seen->off && seen->items && seen->n_rows >= 0), "%s: seen CSR has NULL arrays", who);
  TRS_REQUIRE(hist != nullptr && hist->n_rows >= 0, "%s: history CSR is NULL", who);
  const int depth = trs_tuning().foldin_depth;
  TRS_REQUIRE(depth == 1 || depth == 2 || depth == 4 || depth == 8, "%s: FOLDIN_DEPTH=%d is not 1, 2, 4 or 8", who,
              depth);
  if (hist->n_rows == 0) return TRS_OK;
  TRS_REQUIRE(hist->off && hist->items, "%s: history CSR has NULL arrays", who);
  const int64_t need_new = trs_item_fold_bytes(hist->n_rows, D);
  TRS_REQUIRE(new_fold_dev && new_fold_bytes >= need_new, "%s: new-item fold buffer too small (%lld < %lld)", who,
              (long long)new_fold_bytes, (long long)need_new);
  TRS_REQUIRE(item_out_dev && item_lin_out_dev, "%s: item_out/item_lin_out is NULL", who);

  const int Dp = fi_dp(D), G = Dp / 4;
  const int64_t n_pad = need / ((int64_t)(Dp + 1) * 4), n_pad_new = need_new / ((int64_t)(Dp + 1) * 4);
  const int64_t blocks = (hist->n_rows + TRS_BLOCK / G - 1) / (TRS_BLOCK / G);
  TRS_REQUIRE(blocks < ((int64_t)1 << 31), "%s: too many items in one call", who);
  ItemFoldinArgs a = {};
  a.U = (const float*)tables->user;
  a.ulin = (const float*)tables->user_lin;
  a.n_users = tables->n_users;
  a.S = (const float*)fold_dev;
  a.c = a.S + n_pad * Dp;
  a.n_items = n_items;
  a.T = (const float*)new_fold_dev;
  a.kappa = a.T + n_pad_new * Dp;
  a.off = hist->off;
  a.users = hist->items;
  a.n_new = hist->n_rows;
  a.su = stream_user_dev;
  a.si = stream_item_dev;
  a.n_stream = n_stream;
  a.net = net;
  a.loss = loss;
  a.epochs = epochs;
  a.shuffle = shuffle != 0;
  a.D = D;
  a.nu = negative_visits;
  a.reject = reject_seen != 0;
  a.max_tries = max_tries;
  a.lr = lr;
  a.l2 = l2;
  a.seed = seed;
  const bool rej = reject_seen && seen;
  a.sampler = TrsSampler{1, 0, max_tries, rej ? seen->off : nullptr, rej ? seen->items : nullptr, nullptr, 0,
                         rej ? seen->n_rows : 0};
  a.V = item_out_dev;
  a.b = item_lin_out_dev;
  a.loss_out = loss_out_dev;
  a.err = err_flag_dev;
  hipStream_t s = (hipStream_t)stream;
  const bool vec = (D & 3) == 0 && (reinterpret_cast<uintptr_t>(a.U) & 15) == 0 &&
                   (reinterpret_cast<uintptr_t>(a.V) & 15) == 0;
  if (vec)
    launch_fold_in_items_g<true>(G, depth, a, (unsigned)blocks, s);
  else
    launch_fold_in_items_g<false>(G, depth, a, (unsigned)blocks, s);
  TRS_CHECK_LAUNCH("fold_in_items_kernel");
  return TRS_OK;
}
