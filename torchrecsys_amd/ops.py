# -*- coding: utf-8 -*-
"""Thin torch-tensor front of the C-ABI (include/trs.h).  Every function enqueues HIP kernels of libtrs_hip.so on
torch's current stream; torch only owns the memory.  No CPU path: tensors must live on the GPU."""
import ctypes as C

import torch

from . import _lib
from ._lib import TRS_MAX_META, TRS_NET_FM, TRS_NET_LINEAR, TrsBatch, TrsTables, check, ptr

NET_ID = {"linear": TRS_NET_LINEAR, "fm": TRS_NET_FM}


_raw_stream = getattr(torch._C, "_cuda_getCurrentRawStream", None)
_cur_device = getattr(torch._C, "_cuda_getDevice", None)


def _stream():
    """hipStream_t of torch's current stream on the current device (the raw getters: this sits on every kernel launch,
    and torch.cuda.current_stream() costs ~9 us of Python per call)."""
    if _raw_stream is not None and _cur_device is not None:
        return _raw_stream(_cur_device())
    return torch.cuda.current_stream().cuda_stream


def _dev(t, name, dtype=None):
    if t is None:
        return None
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a GPU tensor: torchrecsys_amd computes on the MI355X only "
                           f"(no CPU fallback); got device {t.device}")
    if dtype is not None and t.dtype != dtype:
        raise TypeError(f"{name} must be {dtype}, got {t.dtype}")
    if not t.is_contiguous():
        raise ValueError(f"{name} must be contiguous")
    return t


def make_tables(user, item, user_lin=None, item_lin=None, metas=(), meta_lins=()):
    """Build a trs_tables struct from fp32 GPU tensors.  Returns (struct, keepalive list)."""
    T = TrsTables()
    keep = [user, item, user_lin, item_lin, list(metas), list(meta_lins)]
    _dev(user, "user table", torch.float32)
    _dev(item, "item table", torch.float32)
    if user.dim() != 2 or item.dim() != 2 or user.shape[1] != item.shape[1]:
        raise ValueError("user/item tables must be (n, D) with the same D")
    M = len(metas)
    if M > TRS_MAX_META:
        raise ValueError(f"at most {TRS_MAX_META} metadata columns are supported, got {M}")
    T.user, T.item = ptr(user), ptr(item)
    T.user_lin = ptr(_dev(user_lin, "user 1-wide table", torch.float32))
    T.item_lin = ptr(_dev(item_lin, "item 1-wide table", torch.float32))
    T.n_users, T.n_items = user.shape[0], item.shape[0]
    T.D, T.M = user.shape[1], M
    for m in range(M):
        _dev(metas[m], f"metadata table {m}", torch.float32)
        if metas[m].shape[1] != user.shape[1]:
            raise ValueError("metadata tables must have the same D as user/item")
        T.meta[m] = ptr(metas[m])
        T.n_meta[m] = metas[m].shape[0]
        if meta_lins:
            T.meta_lin[m] = ptr(_dev(meta_lins[m], f"metadata 1-wide table {m}", torch.float32))
    return T, keep


def make_batch(user, pos, neg=None, pos_meta=None, neg_meta=None, err_flag=None):
    """Build a trs_batch struct from int32/int64 GPU id tensors (all the same dtype)."""
    Bt = TrsBatch()
    ids = [t for t in (user, pos, neg, pos_meta, neg_meta) if t is not None]
    dt = user.dtype
    if dt not in (torch.int32, torch.int64):
        raise TypeError(f"ids must be int32 or int64, got {dt}")
    for t in ids:
        _dev(t, "id tensor", dt)
    B = user.shape[0]
    if pos.shape[0] != B or (neg is not None and neg.shape[0] != B):
        raise ValueError("user/pos/neg id tensors must have the same length")
    Bt.user, Bt.pos, Bt.neg = ptr(user), ptr(pos), ptr(neg)
    Bt.pos_meta, Bt.neg_meta = ptr(pos_meta), ptr(neg_meta)
    Bt.B = B
    Bt.idx_bytes = 4 if dt == torch.int32 else 8
    Bt.err_flag_dev = ptr(err_flag)
    return Bt, ids + [err_flag]


def score_forward(net, T, Bt, B, device, want_neg=True):
    lib = _lib.load()
    pos = torch.empty(B, dtype=torch.float32, device=device)
    neg = torch.empty(B, dtype=torch.float32, device=device) if want_neg else None
    check(lib.trs_score_forward(NET_ID[net], C.byref(T), C.byref(Bt), ptr(pos), ptr(neg), _stream()),
          "trs_score_forward")
    return pos, neg


def score_fwd_bwd(net, T, Bt, B, D, M, device, loss_sum, auc_count=None, want_scores=True, grad_rows=None,
                  grad_lin=None, loss=0):
    """Returns (pos, neg, grad_rows (R,B,D), grad_lin (R,B)); loss_sum/auc_count are accumulated in place."""
    lib = _lib.load()
    R = 3 + 2 * M
    pos = torch.empty(B, dtype=torch.float32, device=device) if want_scores else None
    neg = torch.empty(B, dtype=torch.float32, device=device) if want_scores else None
    if grad_rows is None:
        grad_rows = torch.empty((R, B, D), dtype=torch.float32, device=device)
    if grad_lin is None:
        grad_lin = torch.empty((R, B), dtype=torch.float32, device=device)
    inv_B = 1.0 / B if B > 0 else 0.0
    check(lib.trs_score_fwd_bwd(NET_ID[net], C.byref(T), C.byref(Bt), inv_B, ptr(pos), ptr(neg), ptr(loss_sum),
                                ptr(auc_count), ptr(grad_rows), ptr(grad_lin), int(loss), _stream()),
          "trs_score_fwd_bwd")
    return pos, neg, grad_rows, grad_lin


def score_backward(net, T, Bt, B, D, M, device, gpos, gneg):
    lib = _lib.load()
    R = 3 + 2 * M
    grad_rows = torch.empty((R, B, D), dtype=torch.float32, device=device)
    grad_lin = torch.empty((R, B), dtype=torch.float32, device=device)
    check(lib.trs_score_backward(NET_ID[net], C.byref(T), C.byref(Bt), ptr(gpos), ptr(gneg), ptr(grad_rows),
                                 ptr(grad_lin), _stream()), "trs_score_backward")
    return grad_rows, grad_lin


def score_sgd_update(net, T, Bt, grad_rows, grad_lin, lr):
    check(_lib.load().trs_score_sgd_update(NET_ID[net], C.byref(T), C.byref(Bt), ptr(grad_rows), ptr(grad_lin),
                                           float(lr), _stream()), "trs_score_sgd_update")


class TimingEvents:
    """n HIP events created by the library; elapsed(i, j) after the stream was synchronised."""

    def __init__(self, n):
        self.n = n
        self.handles = (C.c_void_p * n)()
        check(_lib.load().trs_events_create(n, self.handles), "trs_events_create")

    def elapsed_ms(self, i, j):
        out = C.c_float()
        check(_lib.load().trs_events_elapsed_ms(self.handles[i], self.handles[j], C.byref(out)), "trs_events_elapsed_ms")
        return out.value

    def __del__(self):
        try:
            _lib.load().trs_events_destroy(self.n, self.handles)
        except Exception:
            pass


def train_scratch(n_users, n_items, batch, D, device):
    """Zeroed scratch of trs_train_steps_sgd (ownership marks, duplicate stamps, item-bucket lists)."""
    nbytes = _lib.load().trs_train_scratch_bytes(int(n_users), int(n_items), int(batch), int(D))
    return torch.zeros(nbytes // 8 + 1, dtype=torch.int64, device=device)


def interleave_stream(stream_user, stream_item):
    """(N,2) int32 {user, item} pairs: the layout trs_train_steps_sgd reads the resident stream in."""
    return torch.stack([stream_user, stream_item], dim=1).contiguous()


class Sampler:
    """trs_sampler (include/trs.h): negative-sampler options beyond the reference's, for the device RNG mode.
      k            negatives per positive (the epoch then has k * N positions)
      popularity   draw candidates proportionally to the items' frequency in `stream_item`
      seen         (offsets (n_users+1,) int64, items int32 sorted per user): reject items the user has interacted with
      max_tries    candidates tried before the last one is kept
    Score-aware mining (batch_prepare_mined; not part of the C struct):
      mine         None, or 'hardest': train on a negative the current model ranks high
      candidates   K, negatives drawn and scored per triple (1..64)
      top          m: the negative is drawn uniformly among the m highest-scoring candidates (1..K; 1 = the arg-max)"""

    def __init__(self, k=1, popularity=False, seen=None, stream_item=None, max_tries=8, mine=None, candidates=8, top=1):
        if mine is not None and mine != 'hardest':
            raise ValueError(f"mine must be 'hardest' or None, got {mine!r}")
        self.mine = mine
        self.candidates, self.top = int(candidates), int(top)
        if mine is not None and not (1 <= self.candidates <= 64 and 1 <= self.top <= self.candidates):
            raise ValueError(f"mining needs 1 <= candidates <= 64 and 1 <= top <= candidates, got candidates="
                             f"{candidates!r}, top={top!r}")
        self.c = _lib.TrsSampler()
        self.c.k_neg, self.c.popularity, self.c.max_tries = int(k), int(bool(popularity)), int(max_tries)
        self.keep = [seen, stream_item]
        if seen is not None:
            off, items = seen
            _dev(off, "seen offsets", torch.int64)
            _dev(items, "seen items", torch.int32)
            self.c.seen_off, self.c.seen_items, self.c.seen_users = ptr(off), ptr(items), off.numel() - 1
        if popularity:
            _dev(stream_item, "stream items", torch.int32)
            self.c.pop_items, self.c.pop_n = ptr(stream_item), stream_item.numel()
        self.k = int(k)

    @staticmethod
    def seen_csr(user, item, n_users, n_items):
        """CSR of the distinct (user, item) pairs of a device-resident stream: (offsets int64 (n_users+1,), items int32)."""
        key = torch.unique(user.long() * int(n_items) + item.long())
        u = torch.div(key, int(n_items), rounding_mode="floor")
        off = torch.zeros(n_users + 1, dtype=torch.int64, device=user.device)
        off[1:] = torch.cumsum(torch.bincount(u, minlength=n_users), 0)
        return off, (key - u * int(n_items)).to(torch.int32).contiguous()


def _samp(sampler):
    return C.byref(sampler.c) if sampler is not None else None


class EpochPresort:
    """Buffers + result of trs_epoch_presort for n_batches whole batches: id arrays and the item references of every
    batch sorted by row (uint32 keys: key_bytes and, with the user sort, ukey_bytes are always 4).  `step_args(b)` gives
    what trs_train_steps_sgd needs to start at batch b of the slice."""

    def __init__(self, n_batches, batch, n_users, n_items, device, item_meta=None, n_meta=(), user_sort=True,
                 item_flags=True):
        """item_meta (n_items, M) int32 + n_meta (categories per column): also sort every metadata column's references.
        user_sort=False (plain SGD without metadata): user duplicates as FLAGS only (trs_epoch_user_flags: the LDS-bitmap
        kernel, no grouping of the users); the step then adds the flagged users' gradients with float atomics."""
        lib = _lib.load()
        self.user_sort = bool(user_sort) or batch > EpochFlags.MAX_BATCH
        self.item_flags = bool(item_flags)  # False: skip the item-duplicate flag pass (only K1's INL 2 mode reads them)
        kb, ktot, vtot, tmp = (C.c_int64() for _ in range(4))
        check(lib.trs_epoch_presort_sizes(n_batches, batch, n_items, C.byref(kb), C.byref(ktot), C.byref(vtot),
                                          C.byref(tmp)), "trs_epoch_presort_sizes")
        self.n_batches, self.batch, self.n_users, self.n_items = n_batches, batch, n_users, n_items
        self.key_bytes = kb.value
        n_pos = n_batches * batch
        self.ids = [torch.empty(n_pos, dtype=torch.int32, device=device) for _ in range(3)]
        self.keys = torch.empty(ktot.value, dtype=torch.uint8, device=device)
        self.vals = torch.empty(vtot.value, dtype=torch.uint8, device=device)
        uk, uv, ut = (C.c_int64() for _ in range(3))
        check(lib.trs_epoch_user_dups_sizes(n_batches, batch, n_users, C.byref(uk), C.byref(uv), C.byref(ut)),
              "trs_epoch_user_dups_sizes")
        self.ukeys = torch.empty(uk.value if self.user_sort else 8, dtype=torch.uint8, device=device)
        self.uvals = torch.empty(uv.value if self.user_sort else 8, dtype=torch.uint8, device=device)
        self.temp_bytes = max(tmp.value, ut.value)
        self.temp = torch.empty(self.temp_bytes, dtype=torch.uint8, device=device)
        self.user_dup = torch.empty(n_pos, dtype=torch.uint8, device=device)  # 1: user has another reference in its batch
        # {pos, neg} per position: 1 = the item row has another reference in the batch (K1 updates the others in place)
        self.item_dup = torch.empty((n_pos, 2), dtype=torch.uint8, device=device)
        self.sorted_keys = self.sorted_vals = None
        self.item_meta, self.n_meta = item_meta, [int(c) for c in n_meta]
        self.meta_keys = [torch.empty(ktot.value, dtype=torch.uint8, device=device) for _ in self.n_meta]
        self.meta_vals = [torch.empty(vtot.value, dtype=torch.uint8, device=device) for _ in self.n_meta]
        self.meta_sorted = []
        M = len(self.n_meta)
        self.pos_meta = torch.empty((n_pos, M), dtype=torch.int32, device=device) if M else None
        self.neg_meta = torch.empty((n_pos, M), dtype=torch.int32, device=device) if M else None

    @staticmethod
    def bytes_needed(n_batches, batch, n_items, n_meta_cols=0):
        lib = _lib.load()
        kb, ktot, vtot, tmp = (C.c_int64() for _ in range(4))
        check(lib.trs_epoch_presort_sizes(n_batches, batch, n_items, C.byref(kb), C.byref(ktot), C.byref(vtot),
                                          C.byref(tmp)), "trs_epoch_presort_sizes")
        return (12 * n_batches * batch + (1 + n_meta_cols) * (ktot.value + vtot.value) + tmp.value
                + 19 * n_batches * batch)

    def run(self, stream_ui, neg_static, shuffle_key, sample_seed, first_pos, err_flag, given_ids=None, sampler=None):
        """Generate (stream_ui given) or adopt (given_ids = (user, pos, neg) int32 tensors) the ids and sort the refs."""
        if given_ids is not None:
            n_pos = self.n_batches * self.batch  # may be a shorter tail slice in the same buffers
            for dst, src in zip(self.ids, given_ids):
                dst[:n_pos].copy_(src[:n_pos])
        sk, sv = C.c_void_p(), C.c_void_p()
        N = 0 if stream_ui is None else stream_ui.shape[0]
        check(_lib.load().trs_epoch_presort(ptr(stream_ui), ptr(neg_static), N, int(shuffle_key), int(sample_seed),
                                            int(first_pos), self.n_batches, self.batch, self.n_users, self.n_items,
                                            ptr(self.ids[0]), ptr(self.ids[1]), ptr(self.ids[2]), ptr(self.keys),
                                            ptr(self.vals), ptr(self.temp), self.temp_bytes, ptr(err_flag),
                                            C.byref(sk), C.byref(sv), ptr(self.item_dup) if self.item_flags else None,
                                            _samp(sampler), _stream()), "trs_epoch_presort")
        self.sorted_keys, self.sorted_vals = sk.value, sv.value
        if self.user_sort:
            uk, uv, ukb = C.c_void_p(), C.c_void_p(), C.c_int32()
            check(_lib.load().trs_epoch_user_dups(ptr(self.ids[0]), self.n_batches, self.batch, self.n_users,
                                                  ptr(self.ukeys), ptr(self.uvals), ptr(self.temp), self.temp_bytes,
                                                  ptr(self.user_dup), C.byref(uk), C.byref(uv), C.byref(ukb), _stream()),
                  "trs_epoch_user_dups")
            self.sorted_ukeys, self.sorted_uvals, self.ukey_bytes = uk.value, uv.value, ukb.value
        else:
            check(_lib.load().trs_epoch_user_flags(ptr(self.ids[0]), self.n_batches, self.batch, self.n_users,
                                                   ptr(self.user_dup), _stream()), "trs_epoch_user_flags")
            self.sorted_ukeys = self.sorted_uvals = None
            self.ukey_bytes = 0
        self.meta_sorted = []
        for m, n_cat in enumerate(self.n_meta):  # metadata columns: the same grouping by row, per column
            mk, mv = C.c_void_p(), C.c_void_p()
            check(_lib.load().trs_epoch_presort_meta(ptr(self.ids[1]), ptr(self.ids[2]), self.n_batches, self.batch,
                                                     ptr(self.item_meta), len(self.n_meta), m, n_cat,
                                                     ptr(self.meta_keys[m]), ptr(self.meta_vals[m]), ptr(self.temp),
                                                     self.temp_bytes, ptr(err_flag), C.byref(mk), C.byref(mv),
                                                     ptr(self.pos_meta), ptr(self.neg_meta), _stream()),
                  "trs_epoch_presort_meta")
            self.meta_sorted.append((mk.value, mv.value))

    def meta_step_args(self, b):
        """[(sorted keys address, sorted vals address)] of every metadata column for the steps starting at batch b."""
        o = b * self.batch
        return [(k + 2 * o * 4, v + 2 * o * 4) for k, v in self.meta_sorted]

    def meta_id_args(self, b):
        """(pos, neg) metadata id views (positions from batch b on, M) written by the presort, or (None, None)."""
        if not self.meta_sorted:
            return None, None
        o = b * self.batch
        return self.pos_meta[o:], self.neg_meta[o:]

    def step_args(self, b):
        """(user, pos, neg id views, sorted keys address, sorted vals address, user-duplicate flags view, sorted user
        runs, item-duplicate flags view) for the steps starting at batch b."""
        o = b * self.batch
        usorted = ((self.sorted_ukeys + o * self.ukey_bytes, self.sorted_uvals + o * 4, self.ukey_bytes, o)
                   if self.sorted_ukeys is not None else (None, None, 0, o))
        return ([t[o:] for t in self.ids], self.sorted_keys + 2 * o * self.key_bytes, self.sorted_vals + 2 * o * 4,
                self.user_dup[o:], usorted, self.item_dup[o:])


class EpochFlags:
    """The sparse regime's presort (trs_epoch_flags): ids of n_batches whole batches + conservative duplicate flags,
    one launch, no sort.  Same surface as EpochPresort where the step loop needs it."""

    MAX_BATCH = 262_144  # one workgroup per batch (csrc/presort.hip FLAG_THREADS * FLAG_U * FLAG_ROUNDS * FLAG_MAX_GROUPS)

    def __init__(self, n_batches, batch, n_users, n_items, device, ordered=True):
        self.n_batches, self.batch, self.n_users, self.n_items = n_batches, batch, n_users, n_items
        n_pos = n_batches * batch
        self.ids = [torch.empty(n_pos, dtype=torch.int32, device=device) for _ in range(3)]
        self.user_dup = torch.empty(n_pos, dtype=torch.uint8, device=device)
        self.item_dup = torch.empty((n_pos, 2), dtype=torch.uint8, device=device)
        # ordered: every batch comes out with its flagged triples first (trs_epoch_flags_ordered) and their count here —
        # what lets the one-launch step count a workgroup in early (trs_train_args.n_flagged_dev)
        self.n_flagged = torch.zeros(n_batches, dtype=torch.int32, device=device) if ordered else None
        self.key_bytes = self.ukey_bytes = 0

    @staticmethod
    def bytes_needed(n_batches, batch):
        return 15 * n_batches * batch

    def run(self, stream_ui, neg_static, shuffle_key, sample_seed, first_pos, err_flag, given_ids=None, sampler=None,
            n_batches=None):
        """n_batches: fewer batches than the buffers hold (an epoch's last, shorter slice)."""
        nb = self.n_batches if n_batches is None else int(n_batches)
        assert 0 < nb <= self.n_batches
        if given_ids is not None:
            n_pos = nb * self.batch
            for dst, src in zip(self.ids, given_ids):
                dst[:n_pos].copy_(src[:n_pos])
        N = 0 if stream_ui is None else stream_ui.shape[0]
        check(_lib.load().trs_epoch_flags_ordered(ptr(stream_ui), ptr(neg_static), N, int(shuffle_key), int(sample_seed),
                                                  int(first_pos), nb, self.batch, self.n_users,
                                                  self.n_items, ptr(self.ids[0]), ptr(self.ids[1]), ptr(self.ids[2]),
                                                  ptr(self.user_dup), ptr(self.item_dup), ptr(self.n_flagged),
                                                  ptr(err_flag), _samp(sampler), _stream()),
              "trs_epoch_flags_ordered")

    @property
    def base_ptrs(self):
        """Device addresses of (user, pos, neg ids; user / item duplicate flags) — FlagStepCall offsets them itself."""
        bp = getattr(self, "_base_ptrs", None)
        if bp is None:
            bp = self._base_ptrs = tuple(t.data_ptr() for t in self.ids) + (
                self.user_dup.data_ptr(), self.item_dup.data_ptr(),
                self.n_flagged.data_ptr() if self.n_flagged is not None else 0)
        return bp

    def step_args(self, b):
        """(id views, user-duplicate flags view, item-duplicate flags view) from batch b of the slice on."""
        o = b * self.batch
        return [t[o:] for t in self.ids], self.user_dup[o:], self.item_dup[o:]

    def n_flagged_from(self, b):
        """Flagged-triple counts from batch b on (None: the batches are in arbitrary order)."""
        return None if self.n_flagged is None else self.n_flagged[b:]


def train_steps_sgd(net, T, stream_ui, neg_static, shuffle_key, sample_seed, first_pos, batch, n_steps,
                    lr, user_buf, pos_buf, neg_buf, gz_buf, du_buf, loss_sums, err_flag, scratch=None, first_stamp=1,
                    events=None, sorted_keys=None, sorted_vals=None, key_bytes=0, user_dup=None, ustage=None,
                    user_sorted=None, opt=None, meta=None, item_dup=None, loss=0, sync=None, n_flagged=None):
    """n_steps fused steps driven from C (trs_train_steps_sgd).  stream_ui None: the steps' ids are already in
    user/pos/neg_buf.  events: optional flat list of 4*n_steps raw hipEvent_t handles.  sorted_keys / user_sorted: the
    sorted references of an EpochPresort; their keys are 4 bytes wide (key_bytes = 4, and 4 in user_sorted; 0 without
    the arrays; the library refuses 8).  opt: None (SGD with lr) or a
    _lib.TrsOpt (SparseAdam / Adagrad on the presorted path; keep the tensors it points to alive).  item_dup: the
    presort's item-duplicate flags (plain SGD without metadata): K1 also updates item rows referenced once.  Flag mode
    (sparse regime): user_dup + item_dup from an EpochFlags, ustage, and no sorted references; sync = (zeroed int32
    device tensor, ctypes c_uint32 host counter): the flagged references are applied by K1's own launch whenever its
    grid is resident at once."""
    a = _lib.TrsTrainArgs()
    if sync is not None:
        a.sync_dev, a.sync_count_host = ptr(sync[0]), C.pointer(sync[1])
    a.n_flagged_dev = ptr(n_flagged)  # (n_steps int32 of an ordered EpochFlags, or None)
    a.net, a.n_steps, a.tables, a.batch, a.lr = NET_ID[net], int(n_steps), C.pointer(T), int(batch), float(lr)
    a.first_stamp = int(first_stamp)
    a.loss = int(loss)
    a.stream_ui_dev, a.neg_static_dev = ptr(stream_ui), ptr(neg_static)
    a.N = 0 if stream_ui is None else stream_ui.shape[0]
    a.shuffle_key, a.sample_seed, a.first_pos = int(shuffle_key), int(sample_seed), int(first_pos)
    a.user_buf_dev, a.pos_buf_dev, a.neg_buf_dev = ptr(user_buf), ptr(pos_buf), ptr(neg_buf)
    a.gz_buf_dev, a.du_buf_dev, a.loss_sums_dev = ptr(gz_buf), ptr(du_buf), ptr(loss_sums)
    a.err_flag_dev, a.scratch_dev = ptr(err_flag), ptr(scratch)
    a.sorted_keys_dev, a.sorted_vals_dev, a.key_bytes = sorted_keys, sorted_vals, int(key_bytes)
    a.user_dup_flags_dev, a.item_dup_flags_dev, a.ustage_buf_dev = ptr(user_dup), ptr(item_dup), ptr(ustage)
    if user_sorted is not None:
        a.sorted_ukeys_dev, a.sorted_uvals_dev, a.ukey_bytes, a.slice_pos0 = user_sorted
    if opt is not None:
        a.opt = C.pointer(opt)
    if meta is not None:
        a.meta = C.pointer(meta)
    if events is not None:
        ev = (C.c_void_p * len(events))(*events)  # raw hipEvent_t handles (or None = step not timed)
        a.events = C.cast(ev, C.POINTER(C.c_void_p))
    check(_lib.load().trs_train_steps_sgd(C.byref(a), _stream()), "trs_train_steps_sgd")


TIMELINE = None  # diagnostic (bench.py TRS_BENCH_TIMELINE=1): a list that receives (label, time.perf_counter()) stamps


def stamp(label):
    if TIMELINE is not None:
        import time
        TIMELINE.append((label, time.perf_counter()))


class FlagStepCall:
    """trs_train_steps_sgd in flag mode (sparse regime) with the argument struct built ONCE: a call only writes the
    fields that change (step count, stamp, the slice offsets of ids / flags, the loss slot).  The generic wrapper above
    rebuilds ~40 ctypes fields per call — 50-80 us of host time that a short timed window sees as start-up latency."""

    def __init__(self, net, T, batch, lr, gz_buf, du_buf, err_flag, scratch, ustage, loss, sync=None):
        a = self.a = _lib.TrsTrainArgs()
        self.keep = (T, gz_buf, du_buf, err_flag, scratch, ustage, sync)
        if sync is not None:
            a.sync_dev, a.sync_count_host = ptr(sync[0]), C.pointer(sync[1])
        a.net, a.tables, a.batch, a.lr, a.loss = NET_ID[net], C.pointer(T), int(batch), float(lr), int(loss)
        a.gz_buf_dev, a.du_buf_dev = ptr(gz_buf), ptr(du_buf)
        a.err_flag_dev, a.scratch_dev, a.ustage_buf_dev = ptr(err_flag), ptr(scratch), ptr(ustage)
        self.batch = int(batch)
        self.ref = C.byref(a)
        self.fn = _lib.load().trs_train_steps_sgd
        self.sig = (C.addressof(T), float(lr), int(loss), ptr(gz_buf), ptr(du_buf), ptr(ustage), ptr(scratch))

    def __call__(self, ps, b_in_slice, n_steps, loss_sums, first_stamp):
        a, o = self.a, b_in_slice * self.batch
        base = ps.base_ptrs
        a.n_steps, a.first_stamp = int(n_steps), int(first_stamp)
        a.user_buf_dev, a.pos_buf_dev, a.neg_buf_dev = base[0] + 4 * o, base[1] + 4 * o, base[2] + 4 * o
        a.user_dup_flags_dev, a.item_dup_flags_dev = base[3] + o, base[4] + 2 * o
        a.n_flagged_dev = base[5] + 4 * b_in_slice if base[5] else None
        a.loss_sums_dev = loss_sums.data_ptr()
        check(self.fn(self.ref, _stream()), "trs_train_steps_sgd")


def rows_scatter_add(table, idx, vals, alpha, ld=None, err_flag=None):
    n_rows, D = table.shape
    n = idx.shape[0]
    ld = vals.stride(0) if ld is None else ld
    check(_lib.load().trs_rows_scatter_add(ptr(table), n_rows, D, ptr(idx), 4 if idx.dtype == torch.int32 else 8,
                                           ptr(vals), ld, n, float(alpha), ptr(err_flag), _stream()),
          "trs_rows_scatter_add")


def rows_apply_sparse_adam(table, acc, exp_avg, exp_avg_sq, stamp, idx, step_id, lr, beta1, beta2, eps, step_count):
    n_rows, D = table.shape
    check(_lib.load().trs_rows_apply_sparse_adam(ptr(table), ptr(acc), ptr(exp_avg), ptr(exp_avg_sq), ptr(stamp),
                                                 n_rows, D, ptr(idx), 4 if idx.dtype == torch.int32 else 8,
                                                 idx.shape[0], int(step_id), float(lr), float(beta1), float(beta2),
                                                 float(eps), int(step_count), _stream()),
          "trs_rows_apply_sparse_adam")


def rows_apply_adagrad(table, acc, state_sum, stamp, idx, step_id, clr, eps):
    n_rows, D = table.shape
    check(_lib.load().trs_rows_apply_adagrad(ptr(table), ptr(acc), ptr(state_sum), ptr(stamp), n_rows, D, ptr(idx),
                                             4 if idx.dtype == torch.int32 else 8, idx.shape[0], int(step_id),
                                             float(clr), float(eps), _stream()), "trs_rows_apply_adagrad")


def hinge_auc(pos, neg, loss_sum, auc_count, loss=0):
    """loss: 0 = hinge (the reference), 1 = BPR (_lib.LOSS_ID)."""
    check(_lib.load().trs_hinge_auc(ptr(pos), ptr(neg), pos.numel(), ptr(loss_sum), ptr(auc_count), int(loss),
                                    _stream()), "trs_hinge_auc")


def hinge_auc_batches(pos, neg, batch, loss_sums, auc_counts, loss=0):
    """Per-batch hinge sums / AUC counts of consecutive `batch`-row pieces of pos / neg into loss_sums[b], auc_counts[b]."""
    check(_lib.load().trs_hinge_auc_batches(ptr(pos), ptr(neg), pos.numel(), batch, ptr(loss_sums), ptr(auc_counts),
                                            int(loss), _stream()), "trs_hinge_auc_batches")


def hinge_backward(pos, neg, loss=0):
    """-> (gp, gn): the two halves of one (2B,) buffer (`gp._base` is the concatenated gradient the MLP backward reads)."""
    B = pos.numel()
    g = torch.empty(2 * B, dtype=pos.dtype, device=pos.device)
    gp, gn = g[:B], g[B:]
    check(_lib.load().trs_hinge_backward(ptr(pos), ptr(neg), B, 1.0 / B if B else 0.0, ptr(gp), ptr(gn), int(loss),
                                         _stream()), "trs_hinge_backward")
    return gp, gn


def hinge_auc_backward(pos, neg, loss_sum, auc_count, loss=0):
    """hinge_auc + hinge_backward in one launch -> (gp, gn), the halves of one (2B,) buffer."""
    B = pos.numel()
    g = torch.empty(2 * B, dtype=pos.dtype, device=pos.device)
    gp, gn = g[:B], g[B:]
    check(_lib.load().trs_hinge_auc_backward(ptr(pos), ptr(neg), B, 1.0 / B if B else 0.0, ptr(loss_sum),
                                             ptr(auc_count), ptr(gp), ptr(gn), int(loss), _stream()),
          "trs_hinge_auc_backward")
    return gp, gn


def sample_neg(pos, n_items, seed, offset):
    neg = torch.empty_like(pos)
    check(_lib.load().trs_sample_neg(ptr(pos), 4 if pos.dtype == torch.int32 else 8, pos.numel(), int(n_items),
                                     int(seed), int(offset), ptr(neg), _stream()), "trs_sample_neg")
    return neg


def _pair_out(B, M, dev):  # the int32 blocks batch_prepare / batch_prepare_mined fill
    out = {k: torch.empty(B, dtype=torch.int32, device=dev) for k in ("user", "pos", "neg")}
    if M:
        out["pos_meta"] = torch.empty((B, M), dtype=torch.int32, device=dev)
        out["neg_meta"] = torch.empty((B, M), dtype=torch.int32, device=dev)
    return out


def batch_prepare(stream_user, stream_item, neg_static, shuffle_key, t0, B, n_items, seed, offset, item_meta=None,
                  out=None, sampler=None):
    """Returns dict of int32 GPU tensors user/pos/neg[/pos_meta/neg_meta] for epoch positions [t0, t0+B)."""
    dev = stream_user.device
    M = 0 if item_meta is None else item_meta.shape[1]
    if out is None:
        out = _pair_out(B, M, dev)
    check(_lib.load().trs_batch_prepare(ptr(stream_user), ptr(stream_item), ptr(neg_static), stream_user.numel(),
                                        int(shuffle_key), int(t0), int(B), int(n_items), int(seed), int(offset),
                                        ptr(item_meta), M, ptr(out["user"]), ptr(out["pos"]), ptr(out["neg"]),
                                        ptr(out.get("pos_meta")), ptr(out.get("neg_meta")), _samp(sampler), _stream()),
          "trs_batch_prepare")
    return out


def batch_prepare_mined(stream_user, stream_item, shuffle_key, t0, B, n_items, seed, offset, net, T, sampler,
                        item_meta=None, out=None, return_chosen=False):
    """batch_prepare with score-aware hard-negative mining (trs_batch_prepare_mined, one launch): `sampler.candidates`
    negatives per triple are drawn by the sampler's rules, scored by scorer `net` ('linear' | 'fm') under the tables T as
    they are now, and one of the `sampler.top` best becomes out["neg"].  return_chosen: out["chosen"] = the index of
    the chosen candidate (int32).  No static negatives."""
    dev = stream_user.device
    if sampler is None or getattr(sampler, "mine", None) is None:
        raise ValueError("batch_prepare_mined needs an ops.Sampler with mine='hardest'")
    if net not in NET_ID:
        raise ValueError(f"hard-negative mining scores candidates with the Linear / FM kernels, not net={net!r}")
    M = 0 if item_meta is None else item_meta.shape[1]
    if out is None:
        out = _pair_out(B, M, dev)
    if return_chosen and "chosen" not in out:
        out["chosen"] = torch.empty(B, dtype=torch.int32, device=dev)
    check(_lib.load().trs_batch_prepare_mined(ptr(stream_user), ptr(stream_item), None, stream_user.numel(),
                                              int(shuffle_key), int(t0), int(B), int(n_items), int(seed), int(offset),
                                              ptr(item_meta), M, ptr(out["user"]), ptr(out["pos"]), ptr(out["neg"]),
                                              ptr(out.get("pos_meta")), ptr(out.get("neg_meta")), _samp(sampler),
                                              NET_ID[net], C.byref(T), sampler.candidates, sampler.top,
                                              ptr(out.get("chosen")) if return_chosen else None, _stream()),
          "trs_batch_prepare_mined")
    return out


def batch_prepare_multi(stream_user, stream_item, shuffle_key, t0, B, n_items, seed, offset, n_neg, item_meta=None,
                        out=None, sampler=None):
    """batch_prepare for n_neg sampled negatives per positive (trs_batch_prepare_multi, one launch).  Returns a dict of
    int32 GPU tensors: user (B,), items (1 + n_neg, B) slot-major — row 0 the positives, row 1 + j candidate j, drawn
    under seed + j * 0xD1B54A32D192ED03 (candidate 0 is batch_prepare's negative) — and, with item_meta (n_items, M),
    meta (1 + n_neg, B, M).  pos / neg are views of rows 0 / 1.  Candidates may repeat inside a row.  No static
    negatives."""
    dev = stream_user.device
    K = int(n_neg)
    M = 0 if item_meta is None else item_meta.shape[1]
    if out is None:
        out = {"user": torch.empty(B, dtype=torch.int32, device=dev),
               "items": torch.empty((1 + K, B), dtype=torch.int32, device=dev)}
        if M:
            out["meta"] = torch.empty((1 + K, B, M), dtype=torch.int32, device=dev)
        out["pos"], out["neg"] = out["items"][0], out["items"][1] if K >= 1 else None
    check(_lib.load().trs_batch_prepare_multi(ptr(stream_user), ptr(stream_item), None, stream_user.numel(),
                                              int(shuffle_key), int(t0), int(B), int(n_items), int(seed), int(offset),
                                              ptr(item_meta), M, ptr(out["user"]), ptr(out["items"]),
                                              ptr(out.get("meta")), _samp(sampler), K, _stream()),
          "trs_batch_prepare_multi")
    return out


def _check_blocks(user, items, meta, M, multi, also=()):
    """Checks the int32 id blocks user (B,), items (S, B), meta (S, B, M where M > 0) of a step; multi: they are
    batch_prepare_multi's, S = 1 + K >= 2.  also: (tensor, name, dtype) checked with them.  Returns (B, S)."""
    for t, name, dtype in (user, "user ids", torch.int32), (items, "item id block", torch.int32), \
            (meta, "metadata id block", torch.int32), *also:
        _dev(t, name, dtype)
    if items.dim() != 2 or items.shape[1] != user.shape[0] or items.shape[0] < 1 + multi:
        raise ValueError("items must be the (1 + K, B) block of batch_prepare_multi" if multi else
                         "items must be an (S, B) block of item ids, slot-major")
    B, S = user.shape[0], items.shape[0]
    if M and (meta is None or tuple(meta.shape) != (S, B, M)):
        raise ValueError(f"meta must be the (1 + K, B, M) = ({S}, {B}, {M}) block of batch_prepare_multi" if multi else
                         f"meta must be the (S, B, M) = ({S}, {B}, {M}) block of metadata ids")
    return B, S


def multineg_fields(K, M):
    """Staged gradient fields of score_multi_fwd_bwd: 1 user + (1 + K) item slots + M * (1 + K) metadata slots."""
    return 1 + (1 + K) * (1 + M)


def score_multi_fwd_bwd(net, T, user, items, meta, loss, tau, loss_sum, auc_count=None, grad_rows=None, grad_lin=None,
                        err_flag=None, forward_only=False, inv_B=None):
    """One pass over rows of one positive and K = items.shape[0] - 1 sampled negatives (trs_score_multi_fwd_bwd).
    user (B,), items (1 + K, B), meta (1 + K, B, M) or None: int32, the blocks of batch_prepare_multi.  loss:
    _lib.LOSS_ID (mean of K pairs) or _lib.LOSS_SAMPLED_SOFTMAX (with temperature tau).  loss_sum / auc_count are
    accumulated in place.  Returns (grad_rows (F, B, D), grad_lin (F, B)), F = multineg_fields(K, M), field-major: the
    user, the 1 + K item slots, then the 1 + K slots of every metadata column; (None, None) with forward_only."""
    B, S = _check_blocks(user, items, meta, T.M, True)
    K, D, M = S - 1, T.D, T.M
    if forward_only:
        grad_rows = grad_lin = None
    else:
        F = multineg_fields(K, M)
        if grad_rows is None:
            grad_rows = torch.empty((F, B, D), dtype=torch.float32, device=user.device)
        if grad_lin is None:
            grad_lin = torch.empty((F, B), dtype=torch.float32, device=user.device)
    if inv_B is None:
        inv_B = 1.0 / B if B > 0 else 0.0
    check(_lib.load().trs_score_multi_fwd_bwd(NET_ID[net], C.byref(T), ptr(user), ptr(items), ptr(meta) if M else None,
                                              B, M, K, int(loss), float(tau), float(inv_B), ptr(loss_sum),
                                              ptr(auc_count), ptr(grad_rows), ptr(grad_lin), ptr(err_flag), _stream()),
          "trs_score_multi_fwd_bwd")
    return grad_rows, grad_lin


_warp_weights = {}  # (n_items, K, kind, device) -> (K,) fp32 table of warp_rank_weights


def warp_rank_weight_values(n_items, K, kind="log"):
    """The K float64 rank weights of WARP, entry N - 1 for a row whose first violator came at draw N: with
    r_N = floor((n_items - 1) / N), 'log' gives log(max(1, r_N)) (LightFM's form), 'harmonic' sum_{i=1..r_N} 1 / i
    (Weston et al. 2011).  n_items - 1 < N gives 0.  n_items - 1 is used whatever the sampler's options are: popularity
    or seen rejection make the rank estimate approximate."""
    import numpy as np
    if kind not in ("log", "harmonic"):
        raise ValueError(f"rank_weight must be 'log' or 'harmonic', got {kind!r}")
    r = (int(n_items) - 1) // np.arange(1, int(K) + 1, dtype=np.int64)
    if kind == "log":
        return np.log(np.maximum(r, 1).astype(np.float64))
    H = np.concatenate([[0.0], np.cumsum(1.0 / np.arange(1, max(int(r.max()), 1) + 1, dtype=np.float64))])
    return H[np.maximum(r, 0)]


def warp_rank_weights(n_items, K, kind="log", device=None):
    """(K,) fp32 device table of warp_rank_weight_values (float64 on the host, rounded to fp32), cached per
    (n_items, K, kind) and device."""
    key = (int(n_items), int(K), kind, str(device))
    if key not in _warp_weights:
        w = warp_rank_weight_values(n_items, K, kind)
        _warp_weights[key] = torch.from_numpy(w.astype("float32")).to(device)
    return _warp_weights[key]


def score_warp_fwd_bwd(net, T, user, items, meta, margin, rank_weight, loss_sum, auc_count=None, neg_out=None,
                       neg_meta_out=None, trials_out=None, grad_rows=None, grad_lin=None, err_flag=None,
                       forward_only=False, inv_B=None, want_trials=True):
    """WARP over rows of one positive and K = items.shape[0] - 1 candidates (trs_score_warp_fwd_bwd): the first
    candidate j with (z_j - z_p) + margin > 0 is trained on, weighted by rank_weight[j] ((K,) fp32 on the device).
    user (B,), items (1 + K, B), meta (1 + K, B, M) or None: int32, the blocks of batch_prepare_multi.  loss_sum /
    auc_count are accumulated in place.  Returns (neg (B,), neg_meta (B, M) or None, trials (B,) or None, grad_rows
    (3 + 2M, B, D), grad_lin (3 + 2M, B)) — the staging order of score_fwd_bwd on (user, items[0], neg); the last two
    are None with forward_only."""
    B, S = _check_blocks(user, items, meta, T.M, True, [(rank_weight, "rank_weight", torch.float32)])
    K, D, M = S - 1, T.D, T.M
    if rank_weight is None or rank_weight.numel() != K:
        raise ValueError(f"rank_weight must hold K = {K} floats")
    dev = user.device
    if neg_out is None:
        neg_out = torch.empty(B, dtype=torch.int32, device=dev)
    if M and neg_meta_out is None:
        neg_meta_out = torch.empty((B, M), dtype=torch.int32, device=dev)
    if trials_out is None and want_trials:
        trials_out = torch.empty(B, dtype=torch.int32, device=dev)
    if forward_only:
        grad_rows = grad_lin = None
    else:
        R = 3 + 2 * M
        if grad_rows is None:
            grad_rows = torch.empty((R, B, D), dtype=torch.float32, device=dev)
        if grad_lin is None:
            grad_lin = torch.empty((R, B), dtype=torch.float32, device=dev)
    if inv_B is None:
        inv_B = 1.0 / B if B > 0 else 0.0
    check(_lib.load().trs_score_warp_fwd_bwd(NET_ID[net], C.byref(T), ptr(user), ptr(items), ptr(meta) if M else None,
                                             B, M, K, float(margin), ptr(rank_weight), float(inv_B), ptr(loss_sum),
                                             ptr(auc_count), ptr(neg_out), ptr(neg_meta_out) if M else None,
                                             ptr(trials_out), ptr(grad_rows), ptr(grad_lin), ptr(err_flag), _stream()),
          "trs_score_warp_fwd_bwd")
    return neg_out, (neg_meta_out if M else None), trials_out, grad_rows, grad_lin


def stage_add_l2(net, T, user, items, meta, coefs, grad_rows, grad_lin, err_flag=None):
    """Adds the per-sample L2 term to a step's staged gradients, in place (trs_stage_add_l2, one launch): for every
    staged reference, grad_rows[f, t] += c * W[id] and grad_lin[f, t] += c * w[id] from the tables as they are now.
    user (B,), items (S, B), meta (S, B, M) or None: int32, the blocks of batch_prepare_multi.  coefs = (c_user, c_item,
    c_meta), each already holding the 1/B of the batch mean; a group at 0 is skipped.  grad_rows (F, B, D) and grad_lin
    (F, B), F = 1 + S * (1 + M), field-major: the user, the S item slots, then the S slots of every metadata column."""
    c_user, c_item, c_meta = (float(c) for c in coefs)
    D, M = T.D, T.M
    B, S = _check_blocks(user, items, meta, M if c_meta > 0 else 0, False,  # (meta is read only with its coefficient)
                         [(grad_rows, "grad_rows", torch.float32), (grad_lin, "grad_lin", torch.float32)])
    F = 1 + S * (1 + M)
    if grad_rows is None or tuple(grad_rows.shape) != (F, B, D):
        raise ValueError(f"grad_rows must be the (F, B, D) = ({F}, {B}, {D}) staging buffer")
    if grad_lin is None or tuple(grad_lin.shape) != (F, B):
        raise ValueError(f"grad_lin must be the (F, B) = ({F}, {B}) staging buffer")
    if B == 0:  # (empty buffers have no storage to point at)
        return
    check(_lib.load().trs_stage_add_l2(NET_ID[net], C.byref(T), ptr(user), ptr(items), ptr(meta) if M else None, B, S,
                                       M, c_user, c_item, c_meta, ptr(grad_rows), ptr(grad_lin), ptr(err_flag),
                                       _stream()), "trs_stage_add_l2")


def score_all_items(net, T, user_id, n_items, device, item_meta=None, item0=0, n=None):
    n = n_items - item0 if n is None else n
    out = torch.empty(n, dtype=torch.float32, device=device)
    check(_lib.load().trs_score_all_items(NET_ID[net], C.byref(T), int(user_id), int(item0), int(n), ptr(item_meta),
                                          ptr(out), _stream()), "trs_score_all_items")
    return out


def topk(scores, k):
    lib = _lib.load()
    n = scores.numel()
    ws_bytes = lib.trs_topk_workspace_bytes(n, k)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=scores.device)
    out = torch.empty(k, dtype=torch.int64, device=scores.device)
    check(lib.trs_topk(ptr(scores), n, k, ptr(out), ptr(ws), ws_bytes, _stream()), "trs_topk")
    return out



# ------------------------------------------------------------------------------------------------- retrieval
def csr(off, items):
    """trs_csr of a sorted CSR (offsets int64 (n_rows+1,), items int32) on the GPU; None -> NULL."""
    if off is None:
        return None
    _dev(off, "CSR offsets", torch.int64)
    _dev(items, "CSR items", torch.int32)
    c = _lib.TrsCsr()
    c.off, c.items, c.n_rows = ptr(off), ptr(items), off.numel() - 1
    return c


def item_fold(net, T, n_items, D, device, item_meta=None):
    """Folded item matrix S and constants c of a Linear / FM scorer (trs_item_fold) as one uint8 buffer, or None when
    D is beyond the fused kernel."""
    lib = _lib.load()
    nb = lib.trs_item_fold_bytes(int(n_items), int(D))
    if nb <= 0:
        return None
    buf = torch.empty(nb, dtype=torch.uint8, device=device)
    check(lib.trs_item_fold(NET_ID[net], C.byref(T), ptr(item_meta), ptr(buf), nb, _stream()), "trs_item_fold")
    return buf


def fold_rows(fold, n_items):
    """The padded (n_pad, Dp) fp32 row block of a trs_item_fold buffer (layout: include/trs.h)."""
    n_pad = (n_items + 127) // 128 * 128
    Dp = fold.numel() // (4 * n_pad) - 1
    return fold.view(torch.float32)[:n_pad * Dp].view(n_pad, Dp)


def fold_views(fold, n_items, D):
    """(S (n_items, Dp) fp32, c (n_items,) fp32) views of a trs_item_fold buffer."""
    S = fold_rows(fold, n_items)
    return S[:n_items], fold.view(torch.float32)[S.numel():S.numel() + n_items]


def _topk_out(n, k, dev):
    """What a fused top-k call writes: (ids (n, k) int64, scores (n, k) fp32, workspace, workspace bytes)."""
    ws_bytes = _lib.load().trs_retrieve_workspace_bytes(n, k)
    return (torch.empty((n, k), dtype=torch.int64, device=dev), torch.empty((n, k), dtype=torch.float32, device=dev),
            torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev), ws_bytes)


def retrieve_topk(net, T, fold, users, k, seen=None, rel=None):
    """Fused top-k of dense users (int64 GPU tensor) over the catalogue: (ids (n,k) int64, scores (n,k) fp32,
    metrics (n,4) float64 or None).  seen / rel: (offsets, items) CSRs or None."""
    lib = _lib.load()
    _dev(users, "query users", torch.int64)
    n = users.numel()
    ids, scores, ws, ws_bytes = _topk_out(n, k, users.device)
    met = torch.empty((n, 4), dtype=torch.float64, device=users.device) if rel is not None else None
    cs, cr = csr(*seen) if seen is not None else None, csr(*rel) if rel is not None else None
    check(lib.trs_retrieve_topk(NET_ID[net], C.byref(T), ptr(fold), fold.numel(), ptr(users), n, int(k),
                                C.byref(cs) if cs is not None else None, C.byref(cr) if cr is not None else None,
                                ptr(ids), ptr(scores), ptr(met), ptr(ws), ws_bytes, _stream()), "trs_retrieve_topk")
    return ids, scores, met


def neighbour_fold(rows, n_rows, D, cosine):
    """Rows of a table as a padded, optionally unit-length buffer in trs_item_fold's layout (trs_neighbour_fold), one
    uint8 buffer.  rows: an (n, ld) fp32 GPU matrix whose first n_rows rows and D columns are the table."""
    lib = _lib.load()
    _dev(rows, "neighbour rows", torch.float32)
    if rows.dim() != 2 or rows.shape[0] < n_rows or rows.shape[1] < D:
        raise ValueError(f"rows must be an (n >= {n_rows}, ld >= {D}) matrix, got {tuple(rows.shape)}")
    nb = lib.trs_item_fold_bytes(int(n_rows), int(D))
    buf = torch.empty(max(nb, 8), dtype=torch.uint8, device=rows.device)
    check(lib.trs_neighbour_fold(ptr(rows), int(n_rows), int(D), rows.shape[1], int(bool(cosine)), ptr(buf), nb,
                                 _stream()), "trs_neighbour_fold")
    return buf


def neighbours_topk(fold, n_rows, D, queries, k):
    """Fused top-k neighbours of dense rows `queries` (int64 GPU tensor) in a neighbour_fold buffer, self excluded:
    (ids (n, k) int64 with -1 padding, similarities (n, k) fp32 with -inf padding)."""
    lib = _lib.load()
    _dev(queries, "query rows", torch.int64)
    n = queries.numel()
    ids, scores, ws, ws_bytes = _topk_out(n, k, queries.device)
    check(lib.trs_neighbours_topk(ptr(fold), fold.numel(), int(n_rows), int(D), ptr(queries), n, int(k), ptr(ids),
                                  ptr(scores), ptr(ws), ws_bytes, _stream()), "trs_neighbours_topk")
    return ids, scores


def fold_in_users(net, fold, n_items, D, hist, loss, epochs, lr, l2, seed, shuffle, reject_seen, max_tries,
                  want_loss=False, err_flag=None):
    """New user rows fitted to item histories against a frozen item fold (trs_fold_in_users; the update rule is in
    include/trs.h "fold-in").  fold: an item_fold buffer of (n_items, D); hist: (offsets int64 (n+1,), items int32) GPU
    CSR of sorted, distinct dense item rows.  Returns GPU tensors (U (n, D) fp32, b (n,) fp32, loss (epochs, n) fp32 or
    None).  err_flag: optional int32 GPU tensor whose bit 0 is set by an item id outside the catalogue."""
    lib = _lib.load()
    off, items = hist
    _dev(fold, "item fold", torch.uint8)
    dev = fold.device
    n = off.numel() - 1
    if items.numel() == 0:  # every history empty: the kernel reads no item, but the CSR may not carry a NULL array
        items = torch.zeros(1, dtype=torch.int32, device=dev)
    cs = csr(off, items)
    U = torch.empty((n, int(D)), dtype=torch.float32, device=dev)
    b = torch.empty((n,), dtype=torch.float32, device=dev)
    ls = torch.empty((int(epochs), n), dtype=torch.float32, device=dev) if want_loss else None
    check(lib.trs_fold_in_users(NET_ID[net], ptr(fold), fold.numel(), int(n_items), int(D), C.byref(cs),
                                _lib.LOSS_ID[loss], int(epochs), float(lr), float(l2),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(shuffle)), int(bool(reject_seen)),
                                int(max_tries), ptr(U), ptr(b), ptr(ls), ptr(_dev(err_flag, "err_flag", torch.int32)),
                                _stream()), "trs_fold_in_users")
    return U, b, ls


def fold_in_items(net, T, fold, n_items, new_fold, hist, stream_user, stream_item, seen, loss, epochs, lr, l2,
                  negative_visits, seed, shuffle, reject_seen, max_tries, want_loss=False, err_flag=None):
    """New item rows fitted to user histories against the frozen user table and item fold (trs_fold_in_items; the
    update rule is in include/trs.h "item fold-in").  T: the model's tables (the user side is read); fold: its item_fold
    buffer of (n_items, D); new_fold: an item_fold buffer of (n, D) holding the new items' metadata parts; hist:
    (offsets int64 (n+1,), users int32) GPU CSR of sorted, distinct dense user rows; stream_user / stream_item: the
    int32 train interactions (None with negative_visits == 0); seen: the model's seen CSR or None.  Returns GPU tensors
    (V (n, D) fp32, b (n,) fp32, loss (epochs, n) fp32 or None).  err_flag: optional int32 GPU tensor whose bit 0 is set
    by a user or stream id outside its table."""
    lib = _lib.load()
    off, users = hist
    _dev(fold, "item fold", torch.uint8)
    _dev(new_fold, "new-item fold", torch.uint8)
    _dev(stream_user, "train users", torch.int32)
    _dev(stream_item, "train items", torch.int32)
    if (stream_user is None) != (stream_item is None) or \
            (stream_user is not None and stream_user.numel() != stream_item.numel()):
        raise ValueError("stream_user and stream_item must be given together, with the same length")
    dev = fold.device
    n, D = off.numel() - 1, int(T.D)
    if users.numel() == 0:  # every history empty: the kernel reads no user, but the CSR may not carry a NULL array
        users = torch.zeros(1, dtype=torch.int32, device=dev)
    cs = csr(off, users)
    sn = csr(*seen) if seen is not None else None
    V = torch.empty((n, D), dtype=torch.float32, device=dev)
    b = torch.empty((n,), dtype=torch.float32, device=dev)
    ls = torch.empty((int(epochs), n), dtype=torch.float32, device=dev) if want_loss else None
    check(lib.trs_fold_in_items(NET_ID[net], C.byref(T), ptr(fold), fold.numel(), int(n_items), ptr(new_fold),
                                new_fold.numel(), C.byref(cs), ptr(stream_user), ptr(stream_item),
                                0 if stream_user is None else stream_user.numel(),
                                C.byref(sn) if sn is not None else None, _lib.LOSS_ID[loss], int(epochs), float(lr),
                                float(l2), int(negative_visits), int(seed) & 0xFFFFFFFFFFFFFFFF, int(bool(shuffle)),
                                int(bool(reject_seen)), int(max_tries), ptr(V), ptr(b), ptr(ls),
                                ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()), "trs_fold_in_items")
    return V, b, ls


def als_gram(rows, n=None, D=None):
    """G (D, D) fp32 = Y^T Y of the first n rows and D columns of the fp32 GPU matrix `rows` (trs_als_gram:
    deterministic, no atomics; include/trs.h "implicit ALS")."""
    lib = _lib.load()
    _dev(rows, "ALS rows", torch.float32)
    if rows.dim() != 2:
        raise ValueError(f"rows must be an (n, ld) matrix, got {tuple(rows.shape)}")
    n = rows.shape[0] if n is None else int(n)
    D = rows.shape[1] if D is None else int(D)
    if not 0 <= n <= rows.shape[0] or not 1 <= D <= rows.shape[1]:
        raise ValueError(f"n={n}, D={D} do not fit rows of shape {tuple(rows.shape)}")
    G = torch.empty((D, D), dtype=torch.float32, device=rows.device)
    ws = torch.empty(max(lib.trs_als_gram_workspace_bytes(n, D), 8), dtype=torch.uint8, device=rows.device)
    check(lib.trs_als_gram(ptr(rows), n, D, rows.shape[1], ptr(G), ptr(ws), _stream()), "trs_als_gram")
    return G


def als_solve(other, G, nbr, regularization, alpha, cg_steps, rows_inout, err_flag=None):
    """One ALS half-sweep in place (trs_als_solve; the rule is in include/trs.h "implicit ALS"): every row of rows_inout
    (n_rows, D) takes at most cg_steps conjugate-gradient steps from its current value towards its weighted
    least-squares solution against the frozen table `other` (n_other, D) with Gram matrix G (D, D) = als_gram(other).
    nbr: (offsets int64 (n_rows + 1,), ids int32) GPU CSR of sorted, distinct rows of `other`.  err_flag: optional int32
    GPU tensor whose bit 0 is set by an id outside [0, n_other).  Returns rows_inout."""
    lib = _lib.load()
    off, items = nbr
    _dev(other, "frozen table", torch.float32)
    _dev(G, "Gram matrix", torch.float32)
    _dev(rows_inout, "rows to solve", torch.float32)
    if other.dim() != 2 or rows_inout.dim() != 2 or other.shape[1] != rows_inout.shape[1]:
        raise ValueError("the frozen table and the rows to solve must be (n, D) with the same D")
    D = other.shape[1]
    if tuple(G.shape) != (D, D):
        raise ValueError(f"G must be ({D}, {D}), got {tuple(G.shape)}")
    n_rows = rows_inout.shape[0]
    if off.numel() != n_rows + 1:
        raise ValueError(f"neighbour CSR has {off.numel() - 1} rows for {n_rows} rows to solve")
    if items.numel() == 0:  # every list empty: the kernel reads no id, but the CSR may not carry a NULL array
        items = torch.zeros(1, dtype=torch.int32, device=other.device)
    cs = csr(off, items)
    check(lib.trs_als_solve(ptr(other), other.shape[0], D, ptr(G), C.byref(cs), float(regularization), float(alpha),
                            int(cg_steps), ptr(rows_inout), n_rows, ptr(_dev(err_flag, "err_flag", torch.int32)),
                            _stream()), "trs_als_solve")
    return rows_inout


def lgcn_dinv(off):
    """float32(1 / sqrt(float64(degree))) of every row of a CSR, 0 where the list is empty (include/trs.h "LightGCN")."""
    deg = (off[1:] - off[:-1]).to(torch.float64)
    return torch.where(deg > 0, 1.0 / deg.clamp(min=1).sqrt(), torch.zeros_like(deg)).to(torch.float32).contiguous()


def lgcn_propagate(in_rows, nbr, dinv_out, dinv_in, out, add=None, scale=1.0, accumulate=False, err_flag=None):
    """One launch of the LightGCN operator (trs_lgcn_propagate; the rule is in include/trs.h "LightGCN"):
        out[r] = [out[r] +] scale * ([add[r] +] dinv_out[r] * sum_{c in nbr[r]} dinv_in[c] * in_rows[c]).
    in_rows (n_in, D), out and add (n_out, D) fp32 GPU matrices; nbr = (offsets int64 (n_out + 1,), ids int32) GPU CSR of
    rows of in_rows; out may be add, never in_rows.  err_flag: optional int32 GPU tensor whose bit 0 is set by an id
    outside [0, n_in).  Returns out."""
    off, items = nbr
    _dev(in_rows, "input rows", torch.float32)
    _dev(out, "output rows", torch.float32)
    _dev(add, "rows to add", torch.float32)
    _dev(dinv_out, "dinv_out", torch.float32)
    _dev(dinv_in, "dinv_in", torch.float32)
    if in_rows.dim() != 2 or out.dim() != 2 or in_rows.shape[1] != out.shape[1]:
        raise ValueError("the input and the output rows must be (n, D) with the same D")
    n_out, D = out.shape
    if add is not None and tuple(add.shape) != (n_out, D):
        raise ValueError(f"add must be ({n_out}, {D}), got {tuple(add.shape)}")
    if off.numel() != n_out + 1 or dinv_out.numel() != n_out or dinv_in.numel() != in_rows.shape[0]:
        raise ValueError("the CSR and dinv_out must have one entry per output row, dinv_in one per input row")
    if items.numel() == 0:  # every list empty: the kernel reads no id, but the CSR may not carry a NULL array
        items = torch.zeros(1, dtype=torch.int32, device=out.device)
    cs = csr(off, items)
    check(_lib.load().trs_lgcn_propagate(ptr(in_rows), in_rows.shape[0], D, C.byref(cs), ptr(dinv_out), ptr(dinv_in),
                                         ptr(add), float(scale), ptr(out), n_out, int(bool(accumulate)),
                                         ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()),
          "trs_lgcn_propagate")
    return out


def lgcn_adam(param, grad, exp_avg, exp_avg_sq, lr, beta1, beta2, eps, step_count):
    """torch.optim.Adam's rule on every element of the dense fp32 GPU table `param`, in place (trs_lgcn_adam, one
    launch); exp_avg / exp_avg_sq are the moments, step_count the 1-based step."""
    for t, name in ((param, "param"), (grad, "grad"), (exp_avg, "exp_avg"), (exp_avg_sq, "exp_avg_sq")):
        _dev(t, name, torch.float32)
        if t.shape != param.shape:
            raise ValueError(f"{name} must have the parameter's shape {tuple(param.shape)}, got {tuple(t.shape)}")
    check(_lib.load().trs_lgcn_adam(ptr(param), ptr(grad), ptr(exp_avg), ptr(exp_avg_sq), param.numel(), float(lr),
                                    float(beta1), float(beta2), float(eps), int(step_count), _stream()),
          "trs_lgcn_adam")


def ease_padded(n):
    """Row count and row stride of the fp64 matrices of the EASE solver: n rounded up to a multiple of TRS_EASE_NB."""
    return -(-int(n) // _lib.EASE_NB) * _lib.EASE_NB


def _csr_nonnull(off, items):
    if items.numel() == 0:  # every list empty: the kernels read no id, but the CSR may not carry a NULL array
        items = torch.zeros(1, dtype=torch.int32, device=off.device)
    return csr(off, items), items


def ease_gram(seen_csr, n_items, lam, err_flag=None):
    """A = X^T X + lam I in fp64, (nbar, nbar) with nbar = ease_padded(n_items) and the padding an identity block
    (trs_ease_gram; include/trs.h "EASE").  seen_csr: (offsets int64 (n_users + 1,), items int32) GPU CSR of sorted,
    distinct item ids per user.  Exact: every entry is a count of users, plus lam on the diagonal."""
    off, items = seen_csr
    _dev(off, "CSR offsets", torch.int64)
    _dev(items, "CSR items", torch.int32)
    n, nbar = int(n_items), ease_padded(n_items)
    if not 1 <= n <= _lib.EASE_NMAX:
        raise ValueError(f"n_items={n} outside 1..{_lib.EASE_NMAX} (TRS_EASE_NMAX)")
    A = torch.empty((nbar, nbar), dtype=torch.float64, device=off.device)
    cs, keep = _csr_nonnull(off, items)
    check(_lib.load().trs_ease_gram(C.byref(cs), off.numel() - 1, n, float(lam), ptr(A),
                                    ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()), "trs_ease_gram")
    return A


def ease_invert(A, err, workspace=None):
    """P = A^-1 in place (trs_ease_invert: blocked Cholesky on the fp64 matrix cores) of the padded fp64 matrix
    ease_gram returned; err: int32 GPU tensor whose bit 0 a pivot that is not positive and finite sets.  workspace: a
    uint8 GPU tensor of trs_ease_invert_workspace_bytes to keep between calls (tools/ease_bench.py).  Returns A."""
    lib = _lib.load()
    _dev(A, "A", torch.float64)
    _dev(err, "err_flag", torch.int32)
    if err is None:
        raise ValueError("ease_invert needs an err_flag tensor")
    if A.dim() != 2 or A.shape[0] != A.shape[1] or A.shape[0] % _lib.EASE_NB or A.shape[0] == 0:
        raise ValueError(f"A must be square with a multiple of {_lib.EASE_NB} rows (ease_gram's output), got "
                         f"{tuple(A.shape)}")
    n = A.shape[0]
    ws_bytes = lib.trs_ease_invert_workspace_bytes(n)
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device=A.device) if workspace is None else \
        _dev(workspace, "workspace", torch.uint8)
    check(lib.trs_ease_invert(ptr(A), n, ptr(ws), ws.numel(), ptr(err), _stream()), "trs_ease_invert")
    return A


def ease_weights(P, n):
    """B (n, n) fp32 from the padded fp64 P = ease_invert(...): B[i][j] = -P[i][j] / P[j][j], B[i][i] = 0
    (trs_ease_weights)."""
    _dev(P, "P", torch.float64)
    n = int(n)
    if P.dim() != 2 or P.shape[0] != P.shape[1] or P.shape[0] != ease_padded(n) or n < 1:
        raise ValueError(f"P must be ({ease_padded(n)}, {ease_padded(n)}) for n={n}, got {tuple(P.shape)}")
    B = torch.empty((n, n), dtype=torch.float32, device=P.device)
    check(_lib.load().trs_ease_weights(ptr(P), n, ptr(B), _stream()), "trs_ease_weights")
    return B


def ease_scores(B, hist_csr, rows, err_flag=None):
    """Score rows (len(rows), n) fp32: row r = the sum of the rows of B that row rows[r] of hist_csr lists, in CSR order
    (trs_ease_scores).  B (n, n) fp32; hist_csr (offsets int64, items int32) GPU CSR; rows int64 GPU tensor."""
    _dev(B, "B", torch.float32)
    _dev(rows, "rows", torch.int64)
    off, items = hist_csr
    _dev(off, "CSR offsets", torch.int64)
    _dev(items, "CSR items", torch.int32)
    if B.dim() != 2 or B.shape[0] != B.shape[1]:
        raise ValueError(f"B must be square, got {tuple(B.shape)}")
    n = B.shape[0]
    out = torch.empty((rows.numel(), n), dtype=torch.float32, device=B.device)
    if rows.numel() == 0:
        return out
    cs, keep = _csr_nonnull(off, items)
    check(_lib.load().trs_ease_scores(ptr(B), n, C.byref(cs), ptr(rows), rows.numel(), ptr(out),
                                      ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()), "trs_ease_scores")
    return out


def _knn_kind(kind):
    if isinstance(kind, str):
        if kind not in _lib.KNN_KIND:
            raise ValueError(f"similarity must be one of {sorted(_lib.KNN_KIND)}, got {kind!r}")
        return _lib.KNN_KIND[kind]
    if isinstance(kind, bool) or not isinstance(kind, int) or kind not in _lib.KNN_KIND.values():
        raise ValueError(f"similarity must be one of {sorted(_lib.KNN_KIND)} (or its TRS_KNN_* id), got {kind!r}")
    return kind


def knn_build(seen_csr, inv_csr, n_items, kind, shrinkage, K, err_flag=None):
    """The K nearest items of every item (trs_knn_build; include/trs.h "item kNN"): (ids (n_items, K) int32 with -1
    beyond a row's candidates, w (n_items, K) fp32 with 0 there), rows in key order.  seen_csr: user -> sorted distinct
    items, inv_csr: item -> sorted distinct users, both (offsets int64, ids int32) GPU CSRs of the same pairs.  kind:
    'cosine' | 'jaccard' | 'conditional' | 'count'.  Exact and deterministic: the counts are integers, the similarity
    is formed in fp64 and rounded to fp32 once."""
    off, items = seen_csr
    ioff, iusers = inv_csr
    for t, name in ((off, "CSR offsets"), (ioff, "inverse CSR offsets")):
        _dev(t, name, torch.int64)
    for t, name in ((items, "CSR items"), (iusers, "inverse CSR users")):
        _dev(t, name, torch.int32)
    n, K = int(n_items), int(K)
    if n < 1 or ioff.numel() != n + 1:
        raise ValueError(f"the inverse CSR must have n_items={n} >= 1 rows, got {ioff.numel() - 1}")
    if not 1 <= K <= _lib.KNN_KMAX:
        raise ValueError(f"K={K} outside 1..{_lib.KNN_KMAX} (TRS_KNN_KMAX)")
    h = float(shrinkage)
    if not (h >= 0.0 and h != float("inf")):
        raise ValueError(f"shrinkage must be a finite number >= 0, got {shrinkage!r}")
    kind = _knn_kind(kind)
    lib = _lib.load()
    ids = torch.empty((n, K), dtype=torch.int32, device=off.device)
    w = torch.empty((n, K), dtype=torch.float32, device=off.device)
    ws = torch.empty(lib.trs_knn_build_workspace_bytes(n, K), dtype=torch.uint8, device=off.device)
    cs, keep = _csr_nonnull(off, items)
    ci, keep_i = _csr_nonnull(ioff, iusers)
    check(lib.trs_knn_build(C.byref(cs), C.byref(ci), off.numel() - 1, n, kind, h, K, ptr(ids), ptr(w), ptr(ws),
                            ws.numel(), ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()), "trs_knn_build")
    return ids, w


def knn_scores(ids, w, hist_csr, rows, err_flag=None):
    """Score rows (len(rows), n) fp32 of the rows `rows` of hist_csr under the neighbour lists ids / w (n, K): entry j =
    the sum of w[i][s] over the history's items i, in CSR order, whose list holds j at slot s (trs_knn_scores).
    hist_csr (offsets int64, items int32) GPU CSR; rows int64 GPU tensor."""
    _dev(ids, "nbr_ids", torch.int32)
    _dev(w, "nbr_w", torch.float32)
    _dev(rows, "rows", torch.int64)
    off, items = hist_csr
    _dev(off, "CSR offsets", torch.int64)
    _dev(items, "CSR items", torch.int32)
    if ids.dim() != 2 or ids.shape != w.shape or not 1 <= ids.shape[1] <= _lib.KNN_KMAX or ids.shape[0] < 1:
        raise ValueError(f"nbr_ids / nbr_w must both be (n, K) with n >= 1 and K in 1..{_lib.KNN_KMAX}, got "
                         f"{tuple(ids.shape)} / {tuple(w.shape)}")
    n, K = ids.shape
    out = torch.empty((rows.numel(), n), dtype=torch.float32, device=ids.device)
    if rows.numel() == 0:
        return out
    cs, keep = _csr_nonnull(off, items)
    check(_lib.load().trs_knn_scores(ptr(ids), ptr(w), n, K, C.byref(cs), ptr(rows), rows.numel(), ptr(out),
                                     ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()), "trs_knn_scores")
    return out


def seq_weights(context, decay, device=None):
    """The fixed slot weights of the sequence model, w_l = decay^l / sum_{j < L} decay^j (float64 arithmetic, rounded to
    fp32 once): an (L,) fp32 tensor, slot 0 the most recent item."""
    w = [float(decay) ** l for l in range(int(context))]
    return torch.tensor([x / sum(w) for x in w], dtype=torch.float32, device=device)


def _seq_csr(seq):
    """(trs_csr, keepalive) of an ordered sequence CSR (offsets int64 (n + 1,), item ids int32 in order; rows are not
    sorted).  An empty id tensor (every row empty: nothing is ever read) is replaced by a one-element buffer: the entry
    points refuse NULL item ids, since they cannot see from the host that every row is empty."""
    off, items = seq
    _dev(off, "sequence offsets", torch.int64)
    _dev(items, "sequence item ids", torch.int32)
    if items.numel() == 0:
        items = torch.zeros(1, dtype=torch.int32, device=off.device)
    c = _lib.TrsCsr()
    c.off, c.items, c.n_rows = ptr(off), ptr(items), off.numel() - 1
    return c, items


def seq_fwd_bwd(T, ctx, seq, user, entry, neg, weights, loss, loss_sum, auc_count=None, grad_rows=None, grad_lin=None,
                ctx_ids=None, err_flag=None, forward_only=False, inv_B=None):
    """One pass of the sequence model over B triples (trs_seq_fwd_bwd; the model is in include/trs.h "sequence model").
    T: the Linear tables (no metadata); ctx (n_items, D) fp32; seq = (offsets int64 (n_users + 1,), item ids int32 in
    order); user (B,) int32, entry (B,) int64 positions in the id array, neg (B,) int32; weights (L,) fp32; loss a
    _lib.LOSS_ID.  loss_sum / auc_count are accumulated in place.  Returns (grad_rows (3 + L, B, D), grad_lin (3, B),
    ctx_ids (L, B) int32), field-major: user, positive, negative, then the context slots; (None, None, None) with
    forward_only."""
    for t, name, dtype in ((ctx, "context table", torch.float32), (user, "user ids", torch.int32),
                           (entry, "entries", torch.int64), (neg, "negative ids", torch.int32),
                           (weights, "context weights", torch.float32), (loss_sum, "loss_sum", torch.float32),
                           (auc_count, "auc_count", torch.int32), (grad_rows, "grad_rows", torch.float32),
                           (grad_lin, "grad_lin", torch.float32), (ctx_ids, "ctx_ids", torch.int32),
                           (err_flag, "err_flag", torch.int32)):
        _dev(t, name, dtype)
    B, D, L = user.shape[0], T.D, int(weights.numel())
    if entry.shape[0] != B or neg.shape[0] != B:
        raise ValueError("user / entry / neg must have the same length")
    if ctx.dim() != 2 or ctx.shape[0] != T.n_items or ctx.shape[1] != D:
        raise ValueError(f"the context table must be (n_items, D) = ({T.n_items}, {D}), got {tuple(ctx.shape)}")
    if forward_only:
        grad_rows = grad_lin = ctx_ids = None
    else:
        dev = user.device
        if grad_rows is None:
            grad_rows = torch.empty((3 + L, B, D), dtype=torch.float32, device=dev)
        if grad_lin is None:
            grad_lin = torch.empty((3, B), dtype=torch.float32, device=dev)
        if ctx_ids is None:
            ctx_ids = torch.empty((L, B), dtype=torch.int32, device=dev)
        if grad_rows.numel() < (3 + L) * B * D or grad_lin.numel() < 3 * B or ctx_ids.numel() < L * B:
            raise ValueError("staging buffers are smaller than (3 + L, B, D) / (3, B) / (L, B)")
    if inv_B is None:
        inv_B = 1.0 / B if B > 0 else 0.0
    cs, keep = _seq_csr(seq)
    check(_lib.load().trs_seq_fwd_bwd(C.byref(T), ptr(ctx), C.byref(cs), ptr(user), ptr(entry), ptr(neg), B, L,
                                      ptr(weights) if L else None, int(loss), float(inv_B), ptr(loss_sum),
                                      ptr(auc_count), ptr(grad_rows), ptr(grad_lin), ptr(ctx_ids) if L else None,
                                      ptr(err_flag), _stream()), "trs_seq_fwd_bwd")
    return grad_rows, grad_lin, ctx_ids


def seq_user_rows(T, ctx, seq, users, weights, ld=None, out=None, err_flag=None):
    """Query rows of the sequence model (trs_seq_user_rows): out[r, :D] = (U[users[r]], or 0 for users[r] < 0 or users
    None) + sum_l w_l C[row r's item len-1-l].  seq = (offsets int64 (n + 1,), item ids int32, oldest first), one row
    per output row; users (n,) int64 or None.  Returns the (n, ld) fp32 rows (ld defaults to D; columns beyond D are 0
    in a buffer made here)."""
    for t, name, dtype in ((ctx, "context table", torch.float32), (users, "users", torch.int64),
                           (weights, "context weights", torch.float32), (out, "out", torch.float32),
                           (err_flag, "err_flag", torch.int32)):
        _dev(t, name, dtype)
    n, D, L = seq[0].numel() - 1, T.D, int(weights.numel())
    if users is not None and users.numel() != n:
        raise ValueError(f"{users.numel()} users for {n} sequences")
    if ctx.dim() != 2 or ctx.shape[0] != T.n_items or ctx.shape[1] != D:
        raise ValueError(f"the context table must be (n_items, D) = ({T.n_items}, {D}), got {tuple(ctx.shape)}")
    ld = D if ld is None else int(ld)
    if out is None:
        out = torch.zeros((n, ld), dtype=torch.float32, device=ctx.device)
    elif out.dim() != 2 or out.shape[0] != n or out.stride(0) != ld:
        raise ValueError(f"out must be (n, ld) = ({n}, {ld})")
    cs, keep = _seq_csr(seq)
    check(_lib.load().trs_seq_user_rows(C.byref(T), ptr(ctx), C.byref(cs), ptr(users), n, L,
                                        ptr(weights) if L else None, ptr(out), ld, ptr(err_flag), _stream()),
          "trs_seq_user_rows")
    return out


def item_ranks(net, T, fold, users, targets_csr, seen=None, want_values=False):
    """Exact ranks of each query's target items over the catalogue (trs_item_ranks; the definition is in
    include/trs.h "exact ranks").  users: dense int64 GPU tensor; targets_csr: (offsets int64 (n + 1,), items int32) GPU
    CSR, row q = the sorted, distinct dense targets of users[q]; seen: (offsets, items) CSR or None.  Returns (ranks int64
    (n_targets,), values fp32 (n_targets,) in the scorer's output units or None), in CSR order."""
    lib = _lib.load()
    _dev(users, "query users", torch.int64)
    off, items = targets_csr
    n, dev = users.numel(), users.device
    if off.numel() != n + 1:
        raise ValueError(f"targets CSR has {off.numel() - 1} rows for {n} query users")
    n_t = items.numel()
    ranks = torch.empty(n_t, dtype=torch.int64, device=dev)
    values = torch.empty(n_t, dtype=torch.float32, device=dev) if want_values else None
    if n == 0 or n_t == 0:
        return ranks, values
    ws_bytes = lib.trs_item_ranks_workspace_bytes(n, n_t)
    ws = torch.empty(max(ws_bytes, 8), dtype=torch.uint8, device=dev)
    ct, cs = csr(off, items), csr(*seen) if seen is not None else None
    check(lib.trs_item_ranks(NET_ID[net], C.byref(T), ptr(fold), fold.numel(), ptr(users), n, C.byref(ct),
                             C.byref(cs) if cs is not None else None, ptr(ranks), ptr(values), ptr(ws), ws_bytes,
                             _stream()), "trs_item_ranks")
    return ranks, values


def mmr_rerank(nfold, n_items, D, pool_ids, pool_scores, k, lam, want_pos=False, err_flag=None):
    """Greedy MMR selection of k entries out of each row's candidate pool (trs_mmr_rerank; the rule is in include/trs.h
    "diversified re-ranking").  nfold: a neighbour_fold buffer of the item side of (n_items, D); pool_ids (n, N) int64
    dense ids with -1 padding and pool_scores (n, N) fp32, as retrieve_topk returns them; lam = lambda in [0, 1].
    Returns GPU tensors (ids (n, k) int64, scores (n, k) fp32, pool positions (n, k) int32 or None)."""
    lib = _lib.load()
    _dev(nfold, "neighbour fold", torch.uint8)
    _dev(pool_ids, "pool ids", torch.int64)
    _dev(pool_scores, "pool scores", torch.float32)
    if pool_ids.dim() != 2 or pool_scores.shape != pool_ids.shape:
        raise ValueError(f"pool ids / scores must be two (n, N) matrices, got {tuple(pool_ids.shape)} and "
                         f"{tuple(pool_scores.shape)}")
    n, N = pool_ids.shape
    dev = pool_ids.device
    ids = torch.empty((n, int(k)), dtype=torch.int64, device=dev)
    scores = torch.empty((n, int(k)), dtype=torch.float32, device=dev)
    pos = torch.empty((n, int(k)), dtype=torch.int32, device=dev) if want_pos else None
    check(lib.trs_mmr_rerank(ptr(nfold), nfold.numel(), int(n_items), int(D), ptr(pool_ids), ptr(pool_scores), n, N,
                             int(k), float(lam), ptr(ids), ptr(scores), ptr(pos),
                             ptr(_dev(err_flag, "err_flag", torch.int32)), _stream()), "trs_mmr_rerank")
    return ids, scores, pos


def list_ild(nfold, n_items, D, ids):
    """Intra-list diversity of the lists ids (n, k) int64 (-1 = none) over a neighbour_fold buffer of (n_items, D): the
    mean of 1 - similarity over each list's pairs of valid entries (trs_list_ild), float64 (n,) on the GPU."""
    _dev(nfold, "neighbour fold", torch.uint8)
    _dev(ids, "list ids", torch.int64)
    if ids.dim() != 2:
        raise ValueError(f"ids must be an (n, k) matrix, got {tuple(ids.shape)}")
    out = torch.empty((ids.shape[0],), dtype=torch.float64, device=ids.device)
    check(_lib.load().trs_list_ild(ptr(nfold), nfold.numel(), int(n_items), int(D), ptr(ids), ids.shape[0],
                                   ids.shape[1], ptr(out), _stream()), "trs_list_ild")
    return out


def mask_seen(scores, users, seen):
    """Seen entries of score rows (n, n_items) fp32 -> -inf (trs_mask_seen), in place."""
    _dev(scores, "score rows", torch.float32)
    _dev(users, "users", torch.int64)
    cs = csr(*seen)
    check(_lib.load().trs_mask_seen(ptr(scores), scores.shape[0], scores.shape[1], ptr(users), C.byref(cs), _stream()),
          "trs_mask_seen")
    return scores


def rank_metrics(ids, users, rel):
    """(hits, dcg, idcg, n_rel) float64 (n, 4) of top-k ids (n, k) int64 (-1 = none) against rel (trs_rank_metrics)."""
    _dev(ids, "top-k ids", torch.int64)
    _dev(users, "users", torch.int64)
    out = torch.empty((ids.shape[0], 4), dtype=torch.float64, device=ids.device)
    cr = csr(*rel)
    check(_lib.load().trs_rank_metrics(ptr(ids), ids.shape[0], ids.shape[1], ptr(users), C.byref(cr), ptr(out),
                                       _stream()), "trs_rank_metrics")
    return out

# ------------------------------------------------------------------------------------------------- in-batch softmax
class InBatchSoftmax:
    """Workspace and logit chunk of the in-batch softmax loss (csrc/softmax.hip, include/trs.h "in-batch softmax") for
    batches of up to `capacity` rows of a D-factor scorer.  One call = stage, then per chunk of R rows Z = Q K^T, the
    rows kernel, dQ = G K and dK += G^T Q on trs_gemm_f32, then the gradient rows and the loss sum."""

    CHUNK_BYTES = 256 << 20  # largest logit chunk R * B * 4 bytes (R a multiple of 128)

    def __init__(self, capacity, D, device):
        self.cap, self.D, self.dev = int(capacity), int(D), device
        self.Dp = 16
        while self.Dp < self.D:
            self.Dp *= 2
        self.Dq = self.Dp + 4
        self.ws_bytes = _lib.load().trs_softmax_workspace_bytes(self.cap, self.D)
        self.ws = torch.empty(self.ws_bytes // 4, dtype=torch.float32, device=device)
        self.z = None

    def chunk_rows(self, B, chunk_rows=None):
        """Rows per logit chunk: `chunk_rows` if given, else the most multiple-of-128 rows within CHUNK_BYTES."""
        R = chunk_rows or max(128, self.CHUNK_BYTES // (4 * B) // 128 * 128)
        return min(int(R), B)

    def _mats(self, B):
        """Q, K, dQ, dK (B, Dq) views of the workspace for a batch of B rows (layout of include/trs.h)."""
        mat = (B * self.Dq + 63) // 64 * 64
        return [self.ws[k * mat:k * mat + B * self.Dq].view(B, self.Dq) for k in range(4)]

    def __call__(self, net, T, Bt, tau, logq, loss_sum, grad_rows=None, grad_lin=None, chunk_rows=None):
        """loss_sum (1-element fp32) += sum of the batch's row losses; grad_rows (2+M, B, D) / grad_lin (2+M, B) receive
        the gradient rows of the batch mean (both None: the loss only)."""
        lib = _lib.load()
        B = int(Bt.B)
        if B < 1 or B > self.cap:
            raise ValueError(f"in-batch softmax: batch of {B} rows outside 1..{self.cap}")
        s = _stream()
        check(lib.trs_softmax_stage(NET_ID[net], C.byref(T), C.byref(Bt), float(tau), ptr(logq), ptr(self.ws),
                                    self.ws_bytes, s), "trs_softmax_stage")
        Q, K, dQ, dK = self._mats(B)
        Dp = self.Dp
        R = self.chunk_rows(B, chunk_rows)
        if self.z is None or self.z.numel() < R * B:
            self.z = torch.empty(R * B, dtype=torch.float32, device=self.dev)
        want = grad_rows is not None
        for r0 in range(0, B, R):
            n = min(R, B - r0)
            Z = self.z[:n * B].view(n, B)
            gemm(0, 1, Q[r0:r0 + n, :Dp], K[:, :Dp], out=Z)
            check(lib.trs_softmax_rows(ptr(Z), Z.numel() * 4, r0, n, B, self.D, float(tau), ptr(self.ws), self.ws_bytes,
                                       s), "trs_softmax_rows")
            if want:
                gemm(0, 0, Z, K[:, :Dp], out=dQ[r0:r0 + n, :Dp])
                gemm(1, 0, Z, Q[r0:r0 + n], out=dK, beta=0.0 if r0 == 0 else 1.0)
        check(lib.trs_softmax_grads(NET_ID[net], C.byref(T), C.byref(Bt), float(tau), ptr(self.ws), self.ws_bytes,
                                    ptr(grad_rows), ptr(grad_lin), ptr(loss_sum), s), "trs_softmax_grads")


# ------------------------------------------------------------------------------------------------- MLP kernels
def mlp_gather_concat(T, Bt, passes, x=None, x16=None):
    """x: fp32 (rows, (2+M)D) and/or x16: the same image in bfloat16 (same row stride in elements)."""
    ld = (x if x is not None else x16).stride(0)
    if x is not None and x16 is not None and x16.stride(0) != ld:
        raise ValueError("mlp_gather_concat: x and x16 must share the row stride")
    check(_lib.load().trs_mlp_gather_concat(C.byref(T), C.byref(Bt), passes, ptr(x), ptr(x16), ld, _stream()),
          "trs_mlp_gather_concat")


def mlp_gather_gemm1(T, Bt, passes, W, bias, y, bn_part=None, x_image=None):
    """MLP layer 0 with the gather inside the GEMM (trs_mlp_gather_gemm1_fwd).  W: the fp32 weight (N, K) or its bfloat16
    image; y: preallocated (rows, N) fp32 or bfloat16 output; x_image: optional (rows, K) buffer for the x0 image the
    weight-gradient GEMM reads (fp32 with an fp32 W, bfloat16 with a bfloat16 W).  Returns False when the shape is not
    one the fused kernels take (nothing launched: run mlp_gather_concat + gemm)."""
    bf16 = W.dtype == torch.bfloat16
    y32 = y if y.dtype == torch.float32 else None
    y16 = y if y.dtype == torch.bfloat16 else None
    x32 = x_image if (x_image is not None and x_image.dtype == torch.float32) else None
    x16 = x_image if (x_image is not None and x_image.dtype == torch.bfloat16) else None
    rc = _lib.load().trs_mlp_gather_gemm1_fwd(C.byref(T), C.byref(Bt), passes, int(bf16), ptr(W), W.stride(0), ptr(bias),
                                              W.shape[0], ptr(y32), ptr(y16), y.stride(0), ptr(bn_part), ptr(x32),
                                              ptr(x16), x_image.stride(0) if x_image is not None else 0, _stream())
    if rc == 1:
        return False
    check(rc, "trs_mlp_gather_gemm1_fwd")
    return True


def mlp_embed_sgd_supported(T):
    return bool(_lib.load().trs_mlp_embed_sgd_update_supported(C.byref(T)))


def mlp_embed_sgd_update(T, Bt, dx0, lr, user_dup=None, item_dup=None):
    """Embedding-row SGD of an MLP step from d x0 ((2B, ld) fp32 or bfloat16): user / item rows (+ optional duplicate
    flags: unflagged references are plain read-modify-writes) and the owner-computes metadata update."""
    f32 = dx0 if dx0.dtype == torch.float32 else None
    b16 = dx0 if dx0.dtype == torch.bfloat16 else None
    if f32 is None and b16 is None:
        raise TypeError(f"mlp_embed_sgd_update: d x0 must be float32 or bfloat16, got {dx0.dtype}")
    check(_lib.load().trs_mlp_embed_sgd_update(C.byref(T), C.byref(Bt), ptr(f32), ptr(b16), dx0.stride(0), float(lr),
                                               ptr(user_dup), ptr(item_dup), _stream()), "trs_mlp_embed_sgd_update")


_gemm_ws = {}


def _workspace(dev, nbytes):
    """One grow-only scratch buffer per device for split-K slabs / reduction partials."""
    buf = _gemm_ws.get(dev)
    if buf is None or buf.numel() < nbytes:
        buf = torch.empty(max(int(nbytes), 1 << 20), dtype=torch.uint8, device=dev)
        _gemm_ws[dev] = buf
    return buf


GEMM_TILE_ROWS = 128  # rows per output tile = rows per fused-BN-statistics chunk


def gemm(transA, transB, A, B, out=None, bias=None, alpha=1.0, beta=0.0, bf16=False, bn_part=None):
    """out(M,N) = alpha * op(A) op(B) + beta * out (+ bias); fp32 MFMA, or bf16-rounded operands with fp32
    accumulation when bf16=True.  A, B, out: 2-D fp32 GPU tensors whose last
    dimension is contiguous (row stride = leading dimension)."""
    lib = _lib.load()
    M, K = (A.shape[1], A.shape[0]) if transA else (A.shape[0], A.shape[1])
    Kb, N = (B.shape[1], B.shape[0]) if transB else (B.shape[0], B.shape[1])
    if K != Kb:
        raise ValueError(f"gemm: inner dimensions differ ({K} vs {Kb})")
    for t in (A, B):
        if t.dtype != torch.float32 or t.stride(-1) != 1 or not t.is_cuda:
            raise ValueError("gemm operands must be fp32 GPU tensors with a contiguous last dimension")
    if out is None:
        out = torch.empty((M, N), dtype=torch.float32, device=A.device)
    wsb = 0 if bn_part is not None else lib.trs_gemm_f32_workspace_bytes(M, N, K)
    ws = _workspace(A.device, wsb) if wsb else None
    fn = lib.trs_gemm_bf16 if bf16 else lib.trs_gemm_f32
    check(fn(int(transA), int(transB), M, N, K, float(alpha), ptr(A), A.stride(0), ptr(B), B.stride(0),
             float(beta), ptr(out), out.stride(0), ptr(bias), ptr(bn_part), ptr(ws), wsb, _stream()), "trs_gemm")
    return out


def gemm_bf16in(tn, A, B, out=None, bias=None, bn_part=None, out_bf16=False, alpha=1.0, beta=0.0):
    """bf16-resident GEMM: tn False: out(M,N) = A(M,K) B(N,K)^T; tn True: out(M,N) = A(K,M)^T B(K,N).  A, B bfloat16 GPU
    tensors with a contiguous last dimension; fp32 accumulation; fp32 output, or bfloat16 when out_bf16 (or `out` is a
    bfloat16 tensor).  alpha, beta: out = alpha * (product) + beta * out (fp32 `out` given; beta != 0 reads it)."""
    lib = _lib.load()
    for t in (A, B):
        if t.dtype != torch.bfloat16 or t.stride(-1) != 1 or not t.is_cuda:
            raise ValueError("gemm_bf16in operands must be bfloat16 GPU tensors with a contiguous last dimension")
    if tn:
        K, M = A.shape
        Kb, N = B.shape
    else:
        M, K = A.shape
        N, Kb = B.shape
    if K != Kb:
        raise ValueError(f"gemm_bf16in: inner dimensions differ ({K} vs {Kb})")
    if out is None:
        out = torch.empty((M, N), dtype=torch.bfloat16 if out_bf16 else torch.float32, device=A.device)
    o16 = out.dtype == torch.bfloat16
    wsb = 0 if (bn_part is not None or o16) else lib.trs_gemm_bf16in_workspace_bytes(M, N, K)
    ws = _workspace(A.device, wsb) if wsb else None
    if beta != 0.0 and (o16 or bn_part is not None):
        raise ValueError("gemm_bf16in: beta != 0 needs an fp32 `out` and no fused statistics")
    check(lib.trs_gemm_bf16in(int(tn), M, N, K, float(alpha), ptr(A), A.stride(0), ptr(B), B.stride(0), float(beta),
                              None if o16 else ptr(out), ptr(out) if o16 else None, out.stride(0), ptr(bias),
                              ptr(bn_part), ptr(ws), wsb, _stream()), "trs_gemm_bf16in")
    return out


def bn_relu_forward_forms_dot(y):
    """trs_bn_relu_forward forms the output-layer dot inside its launch for this pre-activation tensor (a row's columns in
    one wave: H a power of two in 4..256, 4-element-aligned rows) — the activations then need not be stored."""
    H = y.shape[1]
    return 4 <= H <= 256 and (H & (H - 1)) == 0 and y.stride(0) % 4 == 0 and y.data_ptr() % 16 == 0


def gemm_bf16in_ok(M, N, K):
    """Shapes the bf16-resident kernels take (all tiles interior)."""
    return M % GEMM_TILE_ROWS == 0 and N % 128 == 0 and K % 64 == 0


def f32_to_bf16(src, dst=None, dst_t=None):
    """bf16 copy (dst, same shape) and/or transposed bf16 copy (dst_t) of a 2-D fp32 GPU tensor."""
    rows, cols = src.shape
    check(_lib.load().trs_f32_to_bf16(ptr(src), rows, cols, src.stride(0), ptr(dst), ptr(dst_t), _stream()),
          "trs_f32_to_bf16")


class WeightImages:
    """trs_f32_to_bf16_multi with its argument arrays kept: the bf16 (and transposed bf16) images of up to 8 fp32 matrices
    refreshed by one launch (srcs[k] (rows, cols) -> dsts[k] (rows, cols), dsts_t[k] (cols, rows))."""

    MAX = 8

    def __init__(self, srcs, dsts, dsts_t):
        n = len(srcs)
        if not 1 <= n <= self.MAX:
            raise ValueError(f"WeightImages: 1..{self.MAX} matrices")
        self.keep = (list(srcs), list(dsts), list(dsts_t))
        self.key = tuple(t.data_ptr() for t in srcs)
        self.n = n
        self.src = (C.c_void_p * n)(*[t.data_ptr() for t in srcs])
        self.dst = (C.c_void_p * n)(*[ptr(t) for t in dsts])
        self.dst_t = (C.c_void_p * n)(*[ptr(t) for t in dsts_t])
        self.rows = (C.c_int64 * n)(*[t.shape[0] for t in srcs])
        self.cols = (C.c_int64 * n)(*[t.shape[1] for t in srcs])
        self.ld = (C.c_int64 * n)(*[t.stride(0) for t in srcs])

    def refresh(self):
        check(_lib.load().trs_f32_to_bf16_multi(self.n, self.src, self.rows, self.cols, self.ld, self.dst, self.dst_t,
                                                _stream()), "trs_f32_to_bf16_multi")


def bn_batch_stats(y, rows_per_pass, passes, momentum, mean_out, var_out, running_mean, running_var):
    lib = _lib.load()
    H = y.shape[1]
    ws = _workspace(y.device, 4 * lib.trs_bn_workspace_floats(rows_per_pass, H, passes))
    check(lib.trs_bn_batch_stats(ptr(y), rows_per_pass, H, y.stride(0), passes, float(momentum), ptr(mean_out),
                                 ptr(var_out), ptr(running_mean), ptr(running_var), ptr(ws), _stream()),
          "trs_bn_batch_stats")


def bn_stats_finalize(part, rows_per_pass, chunk_rows, H, passes, momentum, mean_out, var_out, running_mean,
                      running_var):
    check(_lib.load().trs_bn_stats_finalize(ptr(part), rows_per_pass, chunk_rows, H, passes, float(momentum),
                                            ptr(mean_out), ptr(var_out), ptr(running_mean), ptr(running_var), _stream()),
          "trs_bn_stats_finalize")


def bn_relu_forward(y, rows_per_pass, passes, use_bn, stat_passes, mean, var, gamma, beta, eps, out=None, out16=None,
                    momentum=0.0, running_mean=None, running_var=None, dot=None, tracked=None):
    """out: fp32 and/or out16: bfloat16 image of relu(bn(y)) (same row stride in elements).  running_mean/var: the
    momentum update of the running statistics rides in this launch (instead of bn_stats_finalize's), and with it
    tracked (BatchNorm1d.num_batches_tracked, int64 scalar tensor) += passes.  dot=(w, bias,
    scores): the H -> 1 output layer scores[r] = out[r] . w + bias from the same launch where the layer is narrow enough
    (rowdot on `out` otherwise)."""
    H = y.shape[1]
    ldo = (out if out is not None else out16).stride(0) if (out is not None or out16 is not None) else H
    check(_lib.load().trs_bn_relu_forward(ptr(y), int(y.dtype == torch.bfloat16), rows_per_pass, passes, H, y.stride(0),
                                          int(use_bn), stat_passes,
                                          ptr(mean), ptr(var), ptr(gamma), ptr(beta), float(eps), ptr(out), ptr(out16),
                                          ldo, float(momentum), ptr(running_mean), ptr(running_var), ptr(tracked),
                                          *((ptr(t) for t in dot) if dot is not None else (None, None, None)), _stream()),
          "trs_bn_relu_forward")


def bn_relu_backward(y, dx, rows_per_pass, passes, use_bn, mean, var, gamma, beta, eps, dy, dgamma, dbeta,
                     dy_colsum=None, dy16=None, phase=0, sums=None, stat_rows=0, outer=None, outer_xw=None):
    """phase 0: whole backward on the local batch.  Synchronised BatchNorm: phase 1 (reduce: `sums` (passes,2,H) fp32
    receives sum(d), sum(d*xhat)), all-reduce `sums`, phase 2 (apply with stat_rows = world * rows_per_pass).
    outer=(g, w) with dx=None: dx[r][c] = g[r] * w[c] formed inside the kernels (the output layer's input gradient);
    outer_xw (H): receives sum_r g[r] * relu(bn(y))[r] — the output layer's weight gradient without stored activations."""
    lib = _lib.load()
    H = y.shape[1]
    ws = _workspace(y.device, 4 * lib.trs_bn_backward_workspace_floats(rows_per_pass, H, passes))
    ldd = dx.stride(0) if dx is not None else (dy16 if dy16 is not None else dy).stride(0)
    og, ow = outer if outer is not None else (None, None)
    check(lib.trs_bn_relu_backward(ptr(y), int(y.dtype == torch.bfloat16), ptr(dx),
                                   int(dx is not None and dx.dtype == torch.bfloat16),
                                   rows_per_pass, passes, H, y.stride(0), ldd, int(use_bn),
                                   ptr(mean), ptr(var), ptr(gamma), ptr(beta), float(eps), ptr(dy), ptr(dy16),
                                   ptr(dgamma), ptr(dbeta), ptr(dy_colsum), ptr(ws), int(phase), ptr(sums),
                                   int(stat_rows), ptr(og), ptr(ow), ptr(outer_xw), _stream()), "trs_bn_relu_backward")


def colsum(x, out, row_weight=None, passes=1):
    lib = _lib.load()
    rows, H = x.shape
    rpp = rows // passes
    ws = _workspace(x.device, 4 * lib.trs_colsum_workspace_floats(rpp, passes, H))
    check(lib.trs_colsum(ptr(x), rpp, passes, H, x.stride(0), ptr(row_weight), ptr(out), ptr(ws), _stream()),
          "trs_colsum")


def rowdot(x, w, bias, out):
    rows, H = x.shape
    check(_lib.load().trs_rowdot(ptr(x), rows, H, x.stride(0), ptr(w), ptr(bias), ptr(out), _stream()), "trs_rowdot")


def outer(g, w, dx):
    rows, H = dx.shape
    check(_lib.load().trs_outer(ptr(g), ptr(w), rows, H, ptr(dx), dx.stride(0), _stream()), "trs_outer")
