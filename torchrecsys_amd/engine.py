# -*- coding: utf-8 -*-
"""Training-step engine behind TorchRecSys.fit(): drives the fused HIP kernels for one optimiser step and honours the
user-supplied torch optimiser object (reference model.py:188-200 only ever calls zero_grad() and step() on it).

Optimiser dispatch:
  torch.optim.SGD (momentum=0, weight_decay=0)  -> fused row scatter  W[r] += -lr * g        (trs_score_sgd_update)
  torch.optim.SparseAdam                        -> accumulate + elected-owner lazy Adam rows  (trs_rows_apply_sparse_adam)
  torch.optim.Adagrad (weight_decay=0)          -> accumulate + elected-owner Adagrad rows    (trs_rows_apply_adagrad)
  anything else                                 -> the staged rows are handed to the optimiser as the sparse COO
                                                   gradients autograd would have produced, then optimizer.step().
Moments live in optimizer.state[p] under torch's own key names, so optimizer.state_dict() stays truthful.

Every per-step loss (step, warp_step, softmax_step, multineg_step) stages its gradients with its own kernel into one
field-major layout (staged_layout) and ends in one tail, SparseScorerTrainer._apply_staged, which hands every table its
block through the rule above; single-lr SGD on pairs (step, warp_step) keeps its one-launch fused scatter in front of it.
"""
import os

import torch
from ctypes import addressof as C_addressof

from . import ops


def _group_of(optimizer, p):
    for g in optimizer.param_groups:
        for q in g["params"]:
            if q is p:
                return g
    return None


def classify_optimizer(optimizer, params):
    """'sgd' | 'sparse_adam' | 'adagrad' | 'generic' for the given embedding parameters."""
    groups = [_group_of(optimizer, p) for p in params]
    if any(g is None for g in groups):
        return "generic"
    t = type(optimizer)
    if t is torch.optim.SGD:
        ok = all(g["momentum"] == 0 and g["dampening"] == 0 and g["weight_decay"] == 0 and not g["nesterov"]
                 and not g.get("maximize", False) for g in groups)
        return "sgd" if ok else "generic"
    if t is torch.optim.SparseAdam:
        return "sparse_adam" if all(not g.get("maximize", False) for g in groups) else "generic"
    if t is torch.optim.Adam:
        # torch.optim.Adam raises on sparse gradients, so the reference cannot run it on these tables at all (SURVEY
        # §0.3, README quick-start).  Here it gets SparseAdam's lazy semantics (touched rows only) with Adam's own
        # hyper-parameters; moments live in optimizer.state[p] under Adam's key names.
        ok = all(g["weight_decay"] == 0 and not g.get("amsgrad", False) and not g.get("maximize", False) for g in groups)
        return "sparse_adam" if ok else "generic"
    if t is torch.optim.Adagrad:
        ok = all(g["weight_decay"] == 0 and not g.get("maximize", False) for g in groups)
        return "adagrad" if ok else "generic"
    return "generic"


class RowState:
    """Per-table scratch of the coalescing optimisers: gradient accumulator + owner-election stamps."""

    def __init__(self, p):
        self.acc = torch.zeros_like(p.data)
        self.stamp = torch.zeros(p.shape[0], dtype=torch.int32, device=p.device)
        self.step_id = 0

    def next_id(self):
        self.step_id += 1
        if self.step_id >= 2 ** 31 - 1:
            self.stamp.zero_()
            self.step_id = 1
        return self.step_id


def optimizer_state(kind, optimizer, p, g):
    """optimizer.state[p] of a coalescing rule, created on first use under torch's own key names like torch does (g:
    the parameter's group).  torch.optim.Adam counts its steps in a tensor, SparseAdam in an int; torch.optim.Adagrad
    creates its state in __init__, a foreign object's is made here."""
    st = optimizer.state[p]
    if kind == "sparse_adam" and "exp_avg" not in st:
        st["step"] = torch.tensor(0.0) if type(optimizer) is torch.optim.Adam else 0
        st["exp_avg"] = torch.zeros_like(p.data)
        st["exp_avg_sq"] = torch.zeros_like(p.data)
    if kind == "adagrad" and "sum" not in st:
        st["step"] = torch.tensor(0.0)
        st["sum"] = torch.full_like(p.data, g.get("initial_accumulator_value", 0.0))
    return st


def staged_layout(S, M, has_meta_lin):
    """The one layout of every step's staging buffers (ops.stage_add_l2 documents the same): F =
    1 + S (1 + M) fields, the user, the S item slots, then the S slots of every metadata column.  Returns one (index into
    table_params(), id source 'user' | 'item' | column m, field slice, wide) per table in update order; wide tables take
    their block of grad_rows, 1-wide ones that of grad_lin (has_meta_lin: FM's 1-wide metadata tables)."""
    items = slice(1, 1 + S)
    out = [(0, "user", slice(0, 1), True), (1, "item", items, True), (2, "user", slice(0, 1), False),
           (3, "item", items, False)]
    for m in range(M):
        fields = slice(1 + S + m * S, 1 + S + (m + 1) * S)
        out.append((4 + m, m, fields, True))
        if has_meta_lin:
            out.append((4 + M + m, m, fields, False))
    return out


def apply_rows(kind, optimizer, p, rs, idx, vals, ld=None):
    """One coalescing-optimiser update of table `p` from uncoalesced (idx, vals) entries."""
    g = _group_of(optimizer, p)
    st = optimizer_state(kind, optimizer, p, g)
    ops.rows_scatter_add(rs.acc, idx, vals, 1.0, ld=ld)
    if kind == "sparse_adam":
        st["step"] += 1
        b1, b2 = g["betas"]
        ops.rows_apply_sparse_adam(p.data, rs.acc, st["exp_avg"], st["exp_avg_sq"], rs.stamp, idx, rs.next_id(),
                                   g["lr"], b1, b2, g["eps"], int(st["step"]))
    elif kind == "adagrad":
        st["step"] += 1
        step = float(st["step"])
        clr = g["lr"] / (1 + (step - 1) * g["lr_decay"])
        ops.rows_apply_adagrad(p.data, rs.acc, st["sum"], rs.stamp, idx, rs.next_id(), clr, g["eps"])
    else:
        raise ValueError(kind)


class SparseScorerTrainer:
    """One training step of a Linear / FM scorer on a device-resident batch."""

    def __init__(self, net, optimizer, batch_capacity):
        self.net, self.opt = net, optimizer
        self.params = net.table_params()
        self.kind = classify_optimizer(optimizer, self.params)
        dev = self.params[0].device
        self.dev = dev
        self.D = self.params[0].shape[1]
        self.M = net.n_meta_tables()
        self.R = 3 + 2 * self.M
        self.cap = batch_capacity
        self.grad_rows = torch.empty((self.R, batch_capacity, self.D), dtype=torch.float32, device=dev)
        self.grad_lin = torch.empty((self.R, batch_capacity), dtype=torch.float32, device=dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=dev)
        self.kernel_events = None  # bench.py: {"kernel name": [(start_event, end_event), ...]} on the launch stream
        self.loss_id = 0  # _lib.LOSS_ID: hinge (the reference) | bpr; set by fit(loss=...)
        # specialised exact 3-kernel SGD step (csrc/fast_step.hip): no metadata, plain SGD with one learning rate
        self.fast_lr = None
        self.fast_kind = None  # "sgd": C step loop on every path; "sparse_adam" / "adagrad": on the presorted path only
        hyper = {"sgd": ("lr",), "sparse_adam": ("lr", "betas", "eps"),
                 "adagrad": ("lr", "lr_decay", "eps", "initial_accumulator_value")}.get(self.kind)
        # metadata scorers: plain SGD on any shape; the adaptive rules where the staging kernel with the rule exists
        # (csrc/fast_step.hip meta_stage_kernel: up to 3 sorted columns, whole-row D)
        meta_adaptive_ok = (self.M <= 3 and self.D in (32, 64, 128, 256) and os.environ.get("TRS_META_SORTED", "1") != "0")
        if hyper is not None and (self.M == 0 or self.kind == "sgd" or meta_adaptive_ok):
            lrs = {tuple(_group_of(optimizer, p).get(k) for k in hyper) for p in self.params}
            if len(lrs) == 1:  # one rule for all tables
                self.fast_kind = self.kind
                self.fast_lr = _group_of(optimizer, self.params[0])["lr"]
                self.gz = torch.empty((2, batch_capacity), dtype=torch.float32, device=dev)
                self.du = torch.empty((batch_capacity, self.D), dtype=torch.float32, device=dev)
                self.id_bufs = [torch.empty(batch_capacity, dtype=torch.int32, device=dev) for _ in range(3)]
                self.scratch = ops.train_scratch(self.params[0].shape[0], self.params[1].shape[0], batch_capacity, self.D, dev)
                self.stamp = 1
        self.row_state = {}
        if self.kind in ("sparse_adam", "adagrad"):
            self.row_state = {id(p): RowState(p) for p in self.params}
        if self.fast_kind in ("sparse_adam", "adagrad"):
            # item runs cut at a chunk boundary: at most one per 64-reference chunk (+ slack)
            # (one list + counter pair for the item table and one per metadata column)
            self.cut_rows = torch.empty((1 + self.M, 2 * batch_capacity // 64 + 64), dtype=torch.int32, device=dev)
            self.cut_count = torch.zeros((1 + self.M, 2), dtype=torch.int32, device=dev)
            self.meta_lin_state = None  # Linear scorer: scratch in place of the 1-wide metadata tables' state
        # presorted epoch slices (csrc/presort.hip): two buffer sets, the one being built on the side stream and the one
        # the step kernels read
        self.ustage = None            # (capacity, D) pre-update user rows staged by K1 for the item update
        self._ps_fits = {}            # batch size -> do the two buffer sets fit
        self._ps_sets = [None, None]  # ops.EpochPresort per set
        self._ps_tags = [None, None]  # what each set holds (epoch, first batch, batches, batch size)
        self._ps_done = [None, None]  # (slice view, completion event) of a prefetched set
        self._ps_cur = 1              # set the step kernels currently read
        self._ps_stream = None        # side HIP stream of the prefetch
        self.xstage = self.meta_ids = None  # metadata scorers: staged field sums / user rows, metadata ids of a batch
        self.item_meta = None               # (n_items, M) int32 item -> metadata table (set by the runner)

    def _views(self, B):
        """Staging views for a batch of B <= capacity rows (contiguous (R,B,D) / (R,B) prefixes)."""
        if B == self.cap:
            return self.grad_rows, self.grad_lin
        gr = self.grad_rows.view(-1)[: self.R * B * self.D].view(self.R, B, self.D)
        gl = self.grad_lin.view(-1)[: self.R * B].view(self.R, B)
        return gr, gl

    def _sync(self):
        """(device arrival counter, host count of scheduled arrivals) of the one-launch flag-mode step
        (trs_train_args.sync_dev / sync_count_host), or None: TRS_FLAG_ONE_LAUNCH=0."""
        if os.environ.get("TRS_FLAG_ONE_LAUNCH", "1") == "0" or getattr(self, "_one_launch_off", False):
            return None
        if getattr(self, "sync", None) is None:
            import ctypes
            self.sync = (torch.zeros(288, dtype=torch.int32, device=self.dev), ctypes.c_uint32(0))
        return self.sync

    def _stamps(self, n):
        """First of n consecutive step stamps of the duplicate-detection scratch (never 0, re-zeroed before wrapping)."""
        if self.stamp + n >= 0xFFFFFFF0:
            self.scratch.zero_()
            self.stamp = 1
            if self.fast_kind in ("sparse_adam", "adagrad"):
                self.cut_count.zero_()  # the cut-run counters alternate by stamp parity
        first = self.stamp
        self.stamp += n
        return first

    # bench timing samples one step in 29: a sampled step carries four event records and runs ~20 us longer (rocprofv3
    # trace: 9 us between K1 and K2, 4-6 us before / after the step, against back-to-back launches otherwise).  A prime
    # stride: a power of two would pin the samples to the same positions of the 512-batch presort slices (the first
    # steps of a slice overlap the next slice's sort) and of the 64-step C calls
    EVENT_EVERY = 29

    def _make_events(self, n_steps):
        """Raw hipEvent_t handles, 4 per sampled step (None for the others), owned by an ops.TimingEvents."""
        self._ev_count = getattr(self, "_ev_count", 0)
        sampled = [s for s in range(n_steps) if (self._ev_count + s) % self.EVENT_EVERY == 0]
        self._ev_count += n_steps
        te = ops.TimingEvents(4 * len(sampled))
        evs = [None] * (4 * n_steps)
        for j, s in enumerate(sampled):
            evs[4 * s:4 * s + 4] = [te.handles[4 * j + q] for q in range(4)]
        return te, evs, len(sampled)

    def _collect_events(self, te, n_sampled, names=("fwd_stage_kernel", "item_update_kernel", "user_update_kernel")):
        """names: what ran between the four events of a step (item_update_kernel = phases a + b when not presorted)."""
        ke = self.kernel_events
        for j in range(n_sampled):
            for q, name in enumerate(names):
                ke.setdefault(name, []).append((te, 4 * j + q, 4 * j + q + 1))

    def fast_stream_steps(self, st, shuffle_key, sample_seed, first_pos, batch, n_steps, loss_sums):
        """n_steps fused steps straight from the resident stream `st` (dict user/pos/neg int32); loss_sums: (n_steps,)
        view.  Only valid when self.fast_lr is not None and batch == capacity."""
        te, evs, ns = self._make_events(n_steps) if self.kernel_events is not None else (None, None, 0)
        if "ui" not in st:
            st["ui"] = ops.interleave_stream(st["user"], st["pos"])
        ops.train_steps_sgd(self.net.NET, self.net.tables(), st["ui"], st["neg"], shuffle_key,
                            sample_seed, first_pos, batch, n_steps, self.fast_lr, *self.id_bufs, self.gz, self.du,
                            loss_sums, self.err, self.scratch, self._stamps(n_steps), evs, loss=self.loss_id)
        if te is not None:
            self._collect_events(te, ns)

    # ---- presorted item references (csrc/presort.hip) ---------------------------------------------------------------
    SLICE_BATCHES = int(os.environ.get("TRS_SLICE_BATCHES", "512"))  # batches grouped per presort call (bounds the buffers: 2 x 512 x B references per set)

    def wants_presort(self, batch):
        """Group the item references by row once per epoch slice (removes the float atomics from the item update and
        lets the step run as two launches).  Measured faster in both regimes — dense (c2: 131 072 references over 100 K
        items per step, 67 -> 49 us) and sparse (c4 shard: 65 536 over 1 M items, 68 -> 51 us) — so it is on whenever
        its buffers fit; TRS_PRESORT_MIN_DENSITY (references per step / n_items) is a tuning knob."""
        n_items = self.params[1].shape[0]
        dense = float(os.environ.get("TRS_PRESORT_MIN_DENSITY", "0"))
        if self.fast_lr is None or 2 * batch < dense * n_items:
            return False
        memo = self._ps_fits
        if batch not in memo:  # decided once: two buffer sets (one being sorted while the other is read)
            need = 2 * (ops.EpochFlags.bytes_needed(self.SLICE_BATCHES, batch) if self.sparse_regime(batch) else
                        ops.EpochPresort.bytes_needed(self.SLICE_BATCHES, batch, n_items, self.M))
            free, _ = torch.cuda.mem_get_info(self.dev)
            memo[batch] = need < 0.3 * free
        return memo[batch]

    def sparse_regime(self, batch):
        """Most item references of a batch are ALONE on their row (uniform ids: probability exp(-2B / n_items) — 0.94 at
        c4's per-GPU batch, 65 536 references over 1M items; 0.27 at c2, 131 072 over 100K).  Then K1 updates the lone
        rows in place, the few flagged references follow in a small launch of float atomics, and the epoch needs duplicate
        FLAGS only (trs_epoch_flags: one launch, no sort) — c4: 48.5 us per step with sorted runs for every reference ->
        38.6 with K1 taking the lone references -> see DESIGN.md for the flag mode.  In the dense regime the sorted runs
        stay (K1's flag loads and conditional stores cost more than they save: 45.7 -> 47.1 us at c2).
        TRS_SPARSE_REGIME=0/1 forces the choice; plain SGD without metadata only."""
        if self.fast_kind != "sgd" or self.M > 0:
            return False
        env = os.environ.get("TRS_SPARSE_REGIME")
        if env is not None:
            return env != "0"
        return 2 * batch <= 0.7 * self.params[1].shape[0] and batch <= ops.EpochFlags.MAX_BATCH  # lone share >= 1/2

    def _presort_run(self, i, n_batches, batch, st, shuffle_key, sample_seed, first_pos, given_ids):
        sets = self._ps_sets
        ps = sets[i]
        if (ps is None or ps.batch != batch or ps.n_batches < n_batches) and self.sparse_regime(batch):
            ps = sets[i] = ops.EpochFlags(max(n_batches, min(self.SLICE_BATCHES, n_batches)), batch,
                                          self.params[0].shape[0], self.params[1].shape[0], self.dev,
                                          ordered=os.environ.get("TRS_FLAG_ORDERED", "1") != "0")  # knob: A/B
        elif ps is None or ps.batch != batch or ps.n_batches < n_batches:
            meta_kw = {}
            if self.M > 0 and os.environ.get("TRS_META_SORTED", "1") != "0":  # knob: 0 = atomic scatter of staged fields
                meta_kw = dict(item_meta=self.item_meta, n_meta=[p.shape[0] for p in self.params[4:4 + self.M]])
            # plain SGD without metadata needs the users' duplicate FLAGS only (flagged users add their gradient with float
            # atomics) as long as few users repeat inside a batch — share ~ 1 - exp(-batch / n_users): c2 6 % (flags 43.5 us
            # per step, sorted runs 45.9), c1 29 % (flags 17.0, sorted runs 13.8); the adaptive rules and the metadata
            # scorers coalesce duplicated users through sorted runs
            few_dups = batch <= 0.15 * self.params[0].shape[0]
            user_sort = not (self.fast_kind == "sgd" and self.M == 0 and few_dups)
            if os.environ.get("TRS_USER_SORT") in ("0", "1"):  # tuning knob
                user_sort = os.environ["TRS_USER_SORT"] == "1" or not (self.fast_kind == "sgd" and self.M == 0)
            ps = sets[i] = ops.EpochPresort(max(n_batches, min(self.SLICE_BATCHES, n_batches)), batch,
                                            self.params[0].shape[0], self.params[1].shape[0], self.dev,
                                            user_sort=user_sort,
                                            item_flags=os.environ.get("TRS_ITEM_INLINE", "0") == "1", **meta_kw)
        if ps.n_batches != n_batches:  # a shorter tail slice: same buffers, fewer batches
            full = ps
            ps = type(full).__new__(type(full))
            ps.__dict__.update(full.__dict__)
            ps.n_batches = n_batches
        if st is not None:
            ps.run(st["ui"], st["neg"], shuffle_key, sample_seed, first_pos, self.err, sampler=getattr(self, "sampler", None))
        else:
            ps.run(None, None, 0, 0, 0, self.err, given_ids=given_ids)
        return ps

    def presort_slice(self, n_batches, batch, st=None, shuffle_key=0, sample_seed=0, first_pos=0, given_ids=None,
                      tag=None, prefetch=False):
        """Group the item references of `n_batches` whole batches (device stream `st`, or host-prepared ids).

        Two buffer sets: with prefetch=True the work is queued on a side HIP stream into the set the step kernels are
        not reading (the sort is bandwidth work, the step kernels are latency-bound, so the two overlap) and is picked
        up later by a call with the same `tag`."""
        if st is not None and "ui" not in st:
            st["ui"] = ops.interleave_stream(st["user"], st["pos"])
        tags, done, cur = self._ps_tags, self._ps_done, self._ps_cur
        main = torch.cuda.current_stream(self.dev)
        if prefetch:
            i = 1 - cur
            if tag is not None and tags[i] == tag:
                return None
            if self._ps_stream is None:
                self._ps_stream = torch.cuda.Stream(self.dev)
            side = self._ps_stream
            side.wait_stream(main)  # the steps that read set i were queued before this point
            with torch.cuda.stream(side):
                ps = self._presort_run(i, n_batches, batch, st, shuffle_key, sample_seed, first_pos, given_ids)
                ev = torch.cuda.Event()
                ev.record(side)
            tags[i], done[i] = tag, (ps, ev)
            return None
        for i in (0, 1):
            if tag is not None and tags[i] == tag and done[i] is not None:
                ps, ev = done[i]
                main.wait_event(ev)
                self._ps_cur = i
                return ps
        i = 1 - cur
        if self._ps_stream is not None:
            main.wait_stream(self._ps_stream)  # a prefetch may still be writing set i
        ps = self._presort_run(i, n_batches, batch, st, shuffle_key, sample_seed, first_pos, given_ids)
        tags[i], done[i] = tag, None
        self._ps_cur = i
        return ps

    def _meta_stage(self, batch, item_meta, meta_sorted=(), meta_ids=(None, None)):
        """_lib.TrsMetaStage of a metadata scorer: K1 looks the ids up in `item_meta` (n_items, M) int32."""
        from . import _lib
        if item_meta is None or item_meta.dtype != torch.int32:
            raise ValueError("metadata scorers need the (n_items, M) int32 item -> metadata table on the device")
        if self.xstage is None:
            passes = 2 if self.net.NET == "fm" else 1
            self.xstage = torch.empty((passes, self.cap, self.D), dtype=torch.float32, device=self.dev)
            self.meta_ids = torch.empty((2, self.cap, self.M), dtype=torch.int32, device=self.dev)
        if batch != self.cap:
            raise ValueError("the C step loop runs whole batches of the trainer's capacity")
        ms = _lib.TrsMetaStage()
        ms.item_meta_tab, ms.xstage, ms.meta_ids = ops.ptr(item_meta), ops.ptr(self.xstage), ops.ptr(self.meta_ids)
        ms.grad_rows, ms.grad_lin = ops.ptr(self.grad_rows), ops.ptr(self.grad_lin)
        for m, (k, v) in enumerate(meta_sorted):  # sorted references per column: runs instead of the atomic scatter
            ms.sorted_keys[m], ms.sorted_vals[m] = k, v
        if meta_sorted:
            if getattr(self, "lin_scratch", None) is None:
                self.lin_scratch = torch.zeros(max(p.shape[0] for p in self.params[4:4 + self.M]), dtype=torch.float32,
                                               device=self.dev)
            ms.lin_scratch = ops.ptr(self.lin_scratch)
            ms.pos_meta_ids, ms.neg_meta_ids = ops.ptr(meta_ids[0]), ops.ptr(meta_ids[1])
        return ms

    def fast_sorted_steps(self, ps, b_in_slice, batch, n_steps, loss_sums, item_meta=None):
        te, evs, ns = self._make_events(n_steps) if self.kernel_events is not None else (None, None, 0)
        if self.ustage is None:
            self.ustage = torch.empty_like(self.du)  # pre-update user rows staged by K1 for the item update
        if isinstance(ps, ops.EpochFlags) and te is None:  # the same call with its argument struct kept between calls
            T = self.net.tables()
            sig = (C_addressof(T), float(self.fast_lr), int(self.loss_id), ops.ptr(self.gz), ops.ptr(self.du),
                   ops.ptr(self.ustage), ops.ptr(self.scratch))
            fc = getattr(self, "_flag_call", None)
            if fc is None or fc.batch != batch or fc.sig != sig:
                fc = self._flag_call = ops.FlagStepCall(self.net.NET, T, batch, self.fast_lr, self.gz, self.du, self.err,
                                                        self.scratch, self.ustage, self.loss_id, self._sync())
            ops.stamp("fast_sorted_steps:before_call")
            fc(ps, b_in_slice, n_steps, loss_sums, self._stamps(n_steps))
            return
        if isinstance(ps, ops.EpochFlags):  # sparse regime: flags only, the flagged references follow K1 with atomics
            ids, udup, idup = ps.step_args(b_in_slice)
            sy = self._sync()
            arrivals = sy[1].value if sy else 0
            ops.train_steps_sgd(self.net.NET, self.net.tables(), None, None, 0, 0, 0, batch, n_steps, self.fast_lr, *ids,
                                self.gz, self.du, loss_sums, self.err, self.scratch, self._stamps(n_steps), evs,
                                user_dup=udup, item_dup=idup, ustage=self.ustage, loss=self.loss_id, sync=self._sync(),
                                n_flagged=ps.n_flagged_from(b_in_slice))
            if te is not None:
                # one launch per step (K1's own workgroups applied the flagged references: the library scheduled arrivals
                # on the counter): the second interval holds no kernel either
                one = sy is not None and sy[1].value != arrivals
                self.one_launch = one
                self._collect_events(te, ns, ("fwd_stage_kernel", "event_overhead_2" if one else "flagged_update_kernel",
                                              "event_overhead"))
            return
        ids, sk, sv, udup, usorted, idup = ps.step_args(b_in_slice)
        idup = None  # dense regime / adaptive rules / metadata scorers: every item reference goes through the runs
        if os.environ.get("TRS_ITEM_INLINE", "0") == "1" and self.fast_kind == "sgd" and self.M == 0:
            idup = ps.step_args(b_in_slice)[5]  # knob: sorted runs + K1 taking the lone item references (INL 2)
        opt = self._adaptive_rule(n_steps) if self.fast_kind != "sgd" else None
        meta = (self._meta_stage(batch, item_meta, ps.meta_step_args(b_in_slice), ps.meta_id_args(b_in_slice))
                if self.M > 0 else None)
        ops.train_steps_sgd(self.net.NET, self.net.tables(), None, None, 0, 0, 0, batch, n_steps, self.fast_lr, *ids,
                            self.gz, self.du, loss_sums, self.err, self.scratch, self._stamps(n_steps), evs, sk, sv,
                            ps.key_bytes, udup, self.ustage, usorted, opt, meta, idup, loss=self.loss_id)
        if te is not None:
            # item and duplicated-user updates are ONE launch, and the last two events are recorded back to back — that
            # interval is the cost of an event record itself
            self._collect_events(te, ns, ("fwd_stage_kernel", "sorted_updates_fused_kernel", "event_overhead"))

    def _adaptive_rule(self, n_steps):
        """_lib.TrsOpt of the next n_steps SparseAdam / Adagrad steps; moments live in optimizer.state[p] under torch's
        own key names (created on first use like torch does) and the step counters are advanced here."""
        from . import _lib
        g = _group_of(self.opt, self.params[0])
        sts = [optimizer_state(self.kind, self.opt, p, g) for p in self.params]  # (one rule for all tables: one g)
        step0 = int(sts[0]["step"])
        assert all(int(st["step"]) == step0 for st in sts), "embedding tables were stepped a different number of times"
        o = _lib.TrsOpt()
        o.lr, o.step0 = float(g["lr"]), step0
        if self.kind == "sparse_adam":
            o.kind, (o.beta1, o.beta2), o.eps = 1, g["betas"], float(g["eps"])
            s1, s2 = [st["exp_avg"] for st in sts], [st["exp_avg_sq"] for st in sts]
        else:
            o.kind, o.eps, o.lr_decay = 2, float(g["eps"]), float(g["lr_decay"])
            s1, s2 = [st["sum"] for st in sts], [None] * len(sts)
        o.user_s1, o.item_s1, o.user_lin_s1, o.item_lin_s1 = (ops.ptr(t) for t in s1[:4])
        o.user_s2, o.item_s2, o.user_lin_s2, o.item_lin_s2 = (ops.ptr(t) for t in s2[:4])
        # the generic path's (all-zero between steps) gradient accumulators double as the meeting point of cut runs
        o.gacc, o.gacc_lin = ops.ptr(self.row_state[id(self.params[1])].acc), ops.ptr(self.row_state[id(self.params[3])].acc)
        o.cut_rows, o.cut_count, o.cut_capacity = ops.ptr(self.cut_rows[0]), ops.ptr(self.cut_count[0]), self.cut_rows.shape[1]
        M = self.M
        has_lin = len(self.params) == 4 + 2 * M  # FM: 1-wide metadata tables follow the metadata tables
        if M > 0 and not has_lin and self.meta_lin_state is None:
            self.meta_lin_state = [torch.zeros((3, self.params[4 + m].shape[0]), dtype=torch.float32, device=self.dev)
                                   for m in range(M)]
        for m in range(M):
            o.meta_s1[m], o.meta_s2[m] = ops.ptr(s1[4 + m]), ops.ptr(s2[4 + m])
            o.meta_gacc[m] = ops.ptr(self.row_state[id(self.params[4 + m])].acc)
            if has_lin:
                o.meta_lin_s1[m], o.meta_lin_s2[m] = ops.ptr(s1[4 + M + m]), ops.ptr(s2[4 + M + m])
                o.meta_gacc_lin[m] = ops.ptr(self.row_state[id(self.params[4 + M + m])].acc)
            else:
                sc = self.meta_lin_state[m]
                o.meta_lin_s1[m], o.meta_lin_s2[m], o.meta_gacc_lin[m] = ops.ptr(sc[0]), ops.ptr(sc[1]), ops.ptr(sc[2])
            o.meta_cut_rows[m], o.meta_cut_count[m] = ops.ptr(self.cut_rows[1 + m]), ops.ptr(self.cut_count[1 + m])
        for st in sts:
            st["step"] += n_steps
        return o

    def fast_array_steps(self, ep, first, batch, n_steps, loss_sums):
        """n_steps fused steps over consecutive batches of host-prepared epoch id arrays `ep` (dict user/pos/neg int32,
        epoch order) starting at row `first`."""
        te, evs, ns = self._make_events(n_steps) if self.kernel_events is not None else (None, None, 0)
        e = first + n_steps * batch
        ops.train_steps_sgd(self.net.NET, self.net.tables(), None, None, 0, 0, 0, batch, n_steps, self.fast_lr,
                            ep["user"][first:e], ep["pos"][first:e], ep["neg"][first:e], self.gz, self.du, loss_sums,
                            self.err, self.scratch, self._stamps(n_steps), evs, loss=self.loss_id)
        if te is not None:
            self._collect_events(te, ns)

    def step(self, ids, loss_slot, auc_slot=None):
        """ids: dict user/pos/neg[/pos_meta/neg_meta] of GPU id tensors.  loss_slot: 1-element fp32 view that receives
        the SUM of the batch's hinge terms (caller divides by B)."""
        B = ids["user"].shape[0]
        net = self.net
        if (self.fast_kind == "sgd" and self.M == 0 and auc_slot is None and ids["user"].dtype == torch.int32
                and self.l2 is None):  # (the one-launch step stages nothing a penalty could be added to)
            te, evs, ns = self._make_events(1) if self.kernel_events is not None else (None, None, 0)
            ops.train_steps_sgd(net.NET, net.tables(), None, None, 0, 0, 0, B, 1, self.fast_lr, ids["user"],
                                ids["pos"], ids["neg"], self.gz, self.du, loss_slot, self.err, self.scratch,
                                self._stamps(1), evs, loss=self.loss_id)
            if te is not None:
                self._collect_events(te, ns)
            return
        T = net.tables()
        Bt, keep = ops.make_batch(ids["user"], ids["pos"], ids["neg"], ids.get("pos_meta"), ids.get("neg_meta"),
                                  self.err)
        gr, gl = self._views(B)
        ev = self.kernel_events
        if ev is not None:
            e0, e1, e2 = (torch.cuda.Event(enable_timing=True) for _ in range(3))
            e0.record()
        ops.score_fwd_bwd(net.NET, T, Bt, B, self.D, self.M, self.dev, loss_slot, auc_slot, want_scores=False,
                          grad_rows=gr, grad_lin=gl, loss=self.loss_id)
        self._add_l2_pair(ids, gr, gl)
        if ev is not None:
            e1.record()
        self._apply_pair_rows(ids, T, Bt, gr, gl, (e0, e1, e2) if ev is not None else None)

    # per-sample L2 regularisation (fit(l2=...)): None | (lambda_user, lambda_item, lambda_metadata), set by fit()
    l2 = None

    def _add_l2(self, user, items, meta, gr, gl):
        """fit(l2=...): adds lambda_group / B times the pre-update row of every staged reference to its staged gradient
        (ops.stage_add_l2, one launch) — between a step's staging kernel and its first row update, so the penalised
        gradient goes through the optimiser's rule like any other.  items (S, B), meta (S, B, M): int32 blocks in the
        staging buffer's slot order."""
        if self.l2 is None:
            return
        inv_B = 1.0 / user.shape[0]
        ops.stage_add_l2(self.net.NET, self.net.tables(), user, items, meta, [lam * inv_B for lam in self.l2], gr, gl,
                         self.err)

    def _add_l2_pair(self, ids, gr, gl):
        """_add_l2 for triples (user, pos, neg) staged in trs_score_fwd_bwd's order: S = 2, one stack per id block (the
        reference-RNG path carries int64 ids)."""
        if self.l2 is None:
            return
        i32 = torch.int32
        items = torch.stack([ids["pos"], ids["neg"]]).to(i32)
        meta = torch.stack([ids["pos_meta"], ids["neg_meta"]]).to(i32) if self.M else None
        self._add_l2(ids["user"].to(i32), items, meta, gr, gl)

    def _apply_pair_rows(self, ids, T, Bt, gr, gl, events=None):
        """The row updates of one step from gradients staged in trs_score_fwd_bwd's order (S = 2 item slots) for the
        triples `ids` / `Bt`: the fused scatter (one launch) for single-lr SGD, the staged tail otherwise.  events:
        step()'s three timing events (bench.py)."""
        lrs = {_group_of(self.opt, p)["lr"] for p in self.params} if self.kind == "sgd" else ()
        if len(lrs) == 1:
            ops.score_sgd_update(self.net.NET, T, Bt, gr, gl, lrs.pop())
            if events is not None:
                e0, e1, e2 = events
                e2.record()
                ev = self.kernel_events
                ev.setdefault("score_kernel<fwd_bwd>", []).append((e0, e1))
                ev.setdefault("score_sgd_update_kernel", []).append((e1, e2))
            return
        self._apply_staged(ids["user"], torch.cat([ids["pos"], ids["neg"]]),
                           lambda m: torch.cat([ids["pos_meta"][:, m], ids["neg_meta"][:, m]]), 2, gr, gl)

    def _apply_staged(self, user, item_idx, meta_idx, S, gr, gl, skip_user_lin=False):
        """The tail of every step: each embedding table takes its block of the staged gradients (staged_layout) through
        the optimiser's rule (module docstring).  user (B,), item_idx (S * B,) and meta_idx(m) -> (S * B,) are the flat
        ids, slot-major as the fields; a column's ids are built once for its two tables.  skip_user_lin: the user's
        1-wide block is known to be exactly zero."""
        if self.kind == "sgd":
            fn = lambda p, idx, vals, ld: ops.rows_scatter_add(p.data, idx, vals, -_group_of(self.opt, p)["lr"], ld=ld)
        elif self.kind in ("sparse_adam", "adagrad"):
            fn = lambda p, idx, vals, ld: apply_rows(self.kind, self.opt, p, self.row_state[id(p)], idx, vals, ld)
        else:
            self.opt.zero_grad()
            fn = self._set_sparse_grad
        B, ids = user.shape[0], {"user": user, "item": item_idx}
        for table, source, fields, wide in staged_layout(S, self.M, net_has_meta_lin(self.net)):
            if skip_user_lin and table == 2:
                continue
            if source not in ids:
                ids[source] = meta_idx(source)
            ld = self.D if wide else 1
            n = fields.stop - fields.start
            fn(self.params[table], ids[source], (gr if wide else gl)[fields].reshape(n * B, ld), ld)
        if self.kind not in ("sgd", "sparse_adam", "adagrad"):
            self.opt.step()

    # in-batch softmax (fit(loss='softmax')): (temperature, (n_items,) fp32 log q or None), set by fit()
    softmax = None
    SOFTMAX_CHUNK_ROWS = None  # logit rows per chunk (a multiple of 128); None: ops.InBatchSoftmax.CHUNK_BYTES decides

    def softmax_step(self, ids, loss_slot):
        """One step of the in-batch softmax loss on the batch's (user, positive, metadata) rows: every other positive of
        the batch is a negative (ids["neg"] is ignored).  loss_slot receives the SUM of the row losses (caller divides
        by B).  S = 1 item slot; the staged rows go through the one tail (_apply_staged)."""
        tau, logq = self.softmax
        B, D, M = ids["user"].shape[0], self.D, self.M
        net = self.net
        if getattr(self, "_sm", None) is None:
            self._sm = ops.InBatchSoftmax(self.cap, D, self.dev)
            self._sm_rows = torch.empty((2 + M) * self.cap * D, dtype=torch.float32, device=self.dev)
            self._sm_lin = torch.empty((2 + M) * self.cap, dtype=torch.float32, device=self.dev)
        gr = self._sm_rows[:(2 + M) * B * D].view(2 + M, B, D)
        gl = self._sm_lin[:(2 + M) * B].view(2 + M, B)
        T = net.tables()
        Bt, keep = ops.make_batch(ids["user"], ids["pos"], None, ids.get("pos_meta"), None, self.err)
        self._sm(net.NET, T, Bt, tau, logq, loss_slot, gr, gl, chunk_rows=self.SOFTMAX_CHUNK_ROWS)
        if self.l2 is not None:  # S = 1: the positives and their metadata, viewed as one-slot blocks
            i32 = torch.int32
            self._add_l2(ids["user"].to(i32), ids["pos"].to(i32).view(1, B),
                         ids["pos_meta"].to(i32).view(1, B, M) if M else None, gr, gl)
        self._apply_staged(ids["user"], ids["pos"], lambda m: ids["pos_meta"][:, m].contiguous(), 1, gr, gl)

    # K sampled negatives per positive (fit(n_negatives=K) / fit(loss='sampled_softmax')): (K, loss id of
    # trs_score_multi_fwd_bwd, temperature), set by fit()
    multineg = None

    def multineg_step(self, ids, loss_slot):
        """One step on rows of one positive and K sampled negatives: ids = ops.batch_prepare_multi's blocks (user (B,),
        items (1 + K, B), meta (1 + K, B, M)).  loss_slot receives the SUM of the row losses (caller divides by B).  One
        kernel stages every gradient from the pre-update tables (S = 1 + K item slots); the rows then go through the
        one tail (_apply_staged), each table's entries being one contiguous block of the staging buffer.  No host sync."""
        K, loss_id, tau = self.multineg
        B, D, M = ids["user"].shape[0], self.D, self.M
        F = ops.multineg_fields(K, M)
        if getattr(self, "_mn_rows", None) is None or self._mn_rows.numel() < F * self.cap * D:
            self._mn_rows = torch.empty(F * self.cap * D, dtype=torch.float32, device=self.dev)
            self._mn_lin = torch.empty(F * self.cap, dtype=torch.float32, device=self.dev)
        gr = self._mn_rows[:F * B * D].view(F, B, D)
        gl = self._mn_lin[:F * B].view(F, B)
        net = self.net
        ops.score_multi_fwd_bwd(net.NET, net.tables(), ids["user"], ids["items"], ids.get("meta"), loss_id, tau,
                                loss_slot, None, gr, gl, self.err)
        self._add_l2(ids["user"], ids["items"], ids.get("meta"), gr, gl)
        # under the softmax the user's 1-wide block is exactly 0: nothing to apply — unless the user group's penalty was
        # added to it.  The ids are (slot, row, column): item ids flat as they lie, one copy per metadata column
        zero_user_lin = loss_id == ops._lib.LOSS_SAMPLED_SOFTMAX and not (self.l2 is not None and self.l2[0] > 0)
        self._apply_staged(ids["user"], ids["items"].view(-1), lambda m: ids["meta"][:, :, m].contiguous().view(-1),
                           1 + K, gr, gl, skip_user_lin=zero_user_lin)

    # WARP (fit(loss='warp')): (K, margin, (K,) fp32 device table of rank weights), set by fit()
    warp = None

    def warp_step(self, ids, loss_slot):
        """One WARP step on rows of one positive and K candidates: ids = ops.batch_prepare_multi's blocks.  One kernel
        finds every row's first margin violator and stages the gradients of (user, positive, that candidate) into the
        (R, B, D) views step() owns, weighted by the rank estimate; the row updates are then exactly step()'s, on the
        triples (user, slot 0, chosen candidate).  loss_slot receives the SUM of the row losses.  No host sync."""
        K, margin, weights = self.warp
        B, M = ids["user"].shape[0], self.M
        if getattr(self, "_warp_neg", None) is None:
            self._warp_neg = torch.empty(self.cap, dtype=torch.int32, device=self.dev)
            self._warp_neg_meta = torch.empty((self.cap, M), dtype=torch.int32, device=self.dev) if M else None
        neg = self._warp_neg[:B]
        neg_meta = self._warp_neg_meta.view(-1)[:B * M].view(B, M) if M else None
        gr, gl = self._views(B)
        T = self.net.tables()
        ops.score_warp_fwd_bwd(self.net.NET, T, ids["user"], ids["items"], ids.get("meta"), margin, weights, loss_slot,
                               None, neg, neg_meta, None, gr, gl, self.err, want_trials=False)
        triple = {"user": ids["user"], "pos": ids["items"][0], "neg": neg}
        if M:
            triple["pos_meta"], triple["neg_meta"] = ids["meta"][0], neg_meta
        Bt, keep = ops.make_batch(triple["user"], triple["pos"], neg, triple.get("pos_meta"), triple.get("neg_meta"),
                                  self.err)
        self._add_l2_pair(triple, gr, gl)  # (user, positive, chosen candidate) of every row, violator or not
        self._apply_pair_rows(triple, T, Bt, gr, gl)

    @staticmethod
    def _set_sparse_grad(p, idx, vals, ld):
        g = torch.sparse_coo_tensor(idx.reshape(1, -1).long(), vals, size=p.shape)
        p.grad = g if p.grad is None else p.grad + g

    def per_step_only(self):
        """Does this configuration need FitRunner's per-step loop?  The in-batch softmax, K sampled negatives and WARP
        have their own staging kernels, and the L2 penalty is added to staged gradients, which neither the C step loop
        nor the presorted path has.  (Mining is the sampler's property: FitRunner asks it.)"""
        return (self.softmax is not None or self.multineg is not None or self.warp is not None
                or self.l2 is not None)

    def n_candidates(self):
        """K when the step takes ops.batch_prepare_multi's blocks of K candidates per row, else None."""
        multi = self.multineg or self.warp
        return multi[0] if multi else None

    def loss_step(self, ids, loss_slot):
        """One step of the loss fit() configured."""
        step = (self.softmax_step if self.softmax is not None else self.multineg_step if self.multineg is not None
                else self.warp_step if self.warp is not None else self.step)
        step(ids, loss_slot)

    def check_errors(self):
        from .collaborative._scorer import check_err_flag
        try:
            check_err_flag(self.err, "fit")
        except RuntimeError:
            self._one_launch_off = True  # (the grid was not resident at once: two launches per step from now on)
            self._flag_call = None
            raise


def net_has_meta_lin(net):
    return bool(getattr(net, "META_LIN_NAME", None))


class SequenceTrainer:
    """Plain-SGD steps of the sequence model (include/trs.h "sequence model") on a Linear net without
    metadata: U, V and b are the net's tables, ctx the context table C (n_items, D), weights the (L,) fixed slot weights,
    seq = (offsets, item ids) the ordered CSR on the device.  One step = trs_sample_neg, trs_seq_fwd_bwd, then each
    table's block of the staging buffer through ops.rows_scatter_add at -lr (U: B rows, V and b: 2B, C: L * B).  No
    optimiser object and no host sync: the loss is accumulated where the caller says."""

    def __init__(self, net, ctx, weights, seq, batch_capacity, lr, loss_id):
        ps = net.table_params()
        self.net, self.ctx, self.weights, self.seq = net, ctx, weights, seq
        self.user, self.item, self.item_lin = ps[0].data, ps[1].data, ps[3].data
        self.dev, self.D, self.L = self.user.device, self.user.shape[1], int(weights.numel())
        self.cap, self.lr, self.loss_id = int(batch_capacity), float(lr), int(loss_id)
        self.n_items = self.item.shape[0]
        F = 3 + self.L
        self.grad_rows = torch.empty(F * self.cap * self.D, dtype=torch.float32, device=self.dev)
        self.grad_lin = torch.empty(3 * self.cap, dtype=torch.float32, device=self.dev)
        self.ctx_ids = torch.empty(max(self.L, 1) * self.cap, dtype=torch.int32, device=self.dev)
        self.items2 = torch.empty(2 * self.cap, dtype=torch.int32, device=self.dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.dev)

    def seq_step(self, user, entry, loss_slot, seed, offset, neg=None):
        """One step on the triples (user[t], entry[t], a sampled negative): user (B,) int32, entry (B,) int64 positions
        in the CSR's id array.  The negative is trs_sample_neg's draw (uniform, never the row's positive) under (seed,
        offset + t) unless `neg` (B,) int32 is given.  loss_slot: 1-element fp32 view that receives the SUM of the row
        losses (the caller divides by B)."""
        B, D, L = user.shape[0], self.D, self.L
        if B > self.cap:
            raise ValueError(f"batch of {B} rows above the trainer's capacity {self.cap}")
        pos = self.seq[1][entry]
        if neg is None:
            neg = ops.sample_neg(pos, self.n_items, seed, offset)
        gr = self.grad_rows[:(3 + L) * B * D].view(3 + L, B, D)
        gl = self.grad_lin[:3 * B].view(3, B)
        cid = self.ctx_ids[:L * B].view(L, B)
        ops.seq_fwd_bwd(self.net.tables(), self.ctx, self.seq, user, entry, neg, self.weights, self.loss_id, loss_slot,
                        None, gr, gl, cid, self.err)
        items = self.items2[:2 * B]
        items[:B], items[B:] = pos, neg
        ops.rows_scatter_add(self.user, user, gr[0], -self.lr, ld=D)
        ops.rows_scatter_add(self.item, items, gr[1:3].view(2 * B, D), -self.lr, ld=D)
        ops.rows_scatter_add(self.item_lin, items, gl[1:3].view(2 * B, 1), -self.lr, ld=1)
        if L:
            ops.rows_scatter_add(self.ctx, cid.view(-1), gr[3:].view(L * B, D), -self.lr, ld=D)

    def check_errors(self):
        from .collaborative._scorer import check_err_flag
        check_err_flag(self.err, "fit_sequence")


class LightGCNTrainer:
    """Training steps of LightGCN (include/trs.h "LightGCN") on a Linear / FM net without metadata.
    base = (U0, V0) are the trained tables; the net's own user / item tables always hold Final = the Horner forward of
    the base tables, and its 1-wide tables stay zero.  graph = (by_user CSR, by_item CSR) of the distinct train pairs on
    the device.  One step = forward (2 * layers launches of trs_lgcn_propagate), trs_score_fwd_bwd as the Linear scorer
    on the propagated tables, the row gradients scatter-added into a zeroed dense G, the backward (the same recurrence
    on G), and the update: plain SGD leaves the last backward launches to add -lr * alpha * H_0 straight into the base
    tables, Adam lets them write the gradient and runs trs_lgcn_adam on each table.  No optimiser object and no host
    sync: the loss is accumulated where the caller says.

    Besides the base tables the trainer holds G (both sides), an item-side and two user-side work tables — 4 buffers of
    the size of both tables together at most (BUFFERS['sgd']) — and for Adam the two moments of each table on top
    (BUFFERS['adam'] = 6)."""

    BUFFERS = {'sgd': 4, 'adam': 6}  # table-pair-sized buffers a fit needs, the base tables included
    BETAS, EPS = (0.9, 0.999), 1e-8  # torch.optim.Adam's defaults

    def __init__(self, net, base, graph, layers, batch_capacity, lr, loss_id, optimizer='adam', l2=0.0):
        ps = net.table_params()
        self.net = net
        self.user, self.item, self.user_lin, self.item_lin = (p.data for p in ps[:4])
        self.base_user, self.base_item = base
        self.by_user, self.by_item = graph
        self.dev, self.D = self.user.device, self.user.shape[1]
        self.K, self.cap, self.lr, self.loss_id = int(layers), int(batch_capacity), float(lr), int(loss_id)
        self.optimizer, self.l2 = optimizer, float(l2)
        self.alpha = float(torch.tensor(1.0 / (self.K + 1), dtype=torch.float32))  # float32(1 / (K + 1))
        self.dinv_user, self.dinv_item = ops.lgcn_dinv(self.by_user[0]), ops.lgcn_dinv(self.by_item[0])
        # the propagated tables scored as the Linear scorer: <Final_u, Final_i> + 0 + 0
        self.tables, self._keep = ops.make_tables(self.user, self.item, self.user_lin, self.item_lin)
        f32 = dict(dtype=torch.float32, device=self.dev)
        self.g_user, self.g_item = torch.zeros_like(self.user), torch.zeros_like(self.item)
        self.w_user = [torch.empty_like(self.user) for _ in range(min(self.K, 2))]  # the user side ping-pongs
        self.w_item = torch.empty_like(self.item) if self.K >= 2 else None
        self.grad_rows = torch.empty(3 * self.cap * self.D, **f32)
        self.grad_lin = torch.empty(3 * self.cap, **f32)
        self.l2_rows = torch.empty(3 * self.cap * self.D, **f32) if self.l2 else None
        self.l2_lin = torch.empty(3 * self.cap, **f32) if self.l2 else None
        self.items2 = torch.empty(2 * self.cap, dtype=torch.int32, device=self.dev)
        self.err = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self.steps = 0
        if optimizer == 'adam':
            self.moments = [torch.zeros_like(t) for t in (self.user, self.user, self.item, self.item)]
        if self.l2:  # the base tables as a scorer's tables: trs_stage_add_l2 reads the rows it penalises from them
            self.base_tables, self._keep_base = ops.make_tables(self.base_user, self.base_item, self.user_lin,
                                                                self.item_lin)

    def _horner(self, e_user, e_item, out_user, out_item, scale, accumulate=False):
        """scale * F_0 of F_K = E, F_k = E + A^ F_{k+1} for E = (e_user, e_item), written (or with accumulate: added)
        to (out_user, out_item); K >= 1.  The user side of step j goes to a work table, the item side is formed in
        place from the user side of the step before; only the last step writes the outputs.  out may be E."""
        K = self.K
        fu, fv = e_user, e_item
        for j in range(K):
            last = j == K - 1
            nu = out_user if last else self.w_user[j % 2]
            nv = out_item if last else self.w_item
            if last and nu is e_user and fu is e_user:  # K == 1 written over E: the item launch still reads e_user
                nu = self.w_user[0]
            sc, acc = (scale, accumulate) if last else (1.0, False)
            ops.lgcn_propagate(fv, self.by_user, self.dinv_user, self.dinv_item, nu, add=e_user, scale=sc,
                               accumulate=acc, err_flag=self.err)
            ops.lgcn_propagate(fu, self.by_item, self.dinv_item, self.dinv_user, nv, add=e_item, scale=sc,
                               accumulate=acc, err_flag=self.err)
            fu, fv = nu, nv
        return fu, fv

    def forward(self):
        """The net's user / item tables = Final of the base tables."""
        if self.K == 0:
            self.user.copy_(self.base_user)
            self.item.copy_(self.base_item)
        else:
            self._horner(self.base_user, self.base_item, self.user, self.item, self.alpha)

    def lgcn_step(self, user, pos, neg, loss_slot):
        """One step on the triples (user, pos, neg), (B,) int32 on the device.  loss_slot: 1-element fp32 view that
        receives the SUM of the row losses (the caller divides by B).  The net's tables hold Final of the base tables
        on entry (forward()) and again on return."""
        B, D, K = user.shape[0], self.D, self.K
        if B > self.cap:
            raise ValueError(f"batch of {B} rows above the trainer's capacity {self.cap}")
        gr = self.grad_rows[:3 * B * D].view(3, B, D)
        gl = self.grad_lin[:3 * B].view(3, B)
        Bt, keep = ops.make_batch(user, pos, neg, None, None, self.err)
        ops.score_fwd_bwd('linear', self.tables, Bt, B, D, 0, self.dev, loss_slot, None, want_scores=False, grad_rows=gr,
                          grad_lin=gl, loss=self.loss_id)
        items = self.items2[:2 * B]
        items[:B], items[B:] = pos, neg
        lr, sgd = self.lr, self.optimizer == 'sgd'
        if self.l2:  # lambda / B times the PRE-update base row of every reference, staged before any update
            lrw = self.l2_rows[:3 * B * D].view(3, B, D)
            llin = self.l2_lin[:3 * B].view(3, B)
            lrw.zero_()
            llin.zero_()
            c = self.l2 / B
            ops.stage_add_l2('linear', self.base_tables, user, items.view(2, B), None, (c, c, 0.0), lrw, llin, self.err)
        if K == 0 and sgd:  # plain matrix factorisation: the row gradients go straight into the base tables
            ops.rows_scatter_add(self.base_user, user, gr[0], -lr, ld=D)
            ops.rows_scatter_add(self.base_item, items, gr[1:3].view(2 * B, D), -lr, ld=D)
        else:
            self.g_user.zero_()
            self.g_item.zero_()
            ops.rows_scatter_add(self.g_user, user, gr[0], 1.0, ld=D)
            ops.rows_scatter_add(self.g_item, items, gr[1:3].view(2 * B, D), 1.0, ld=D)
        if sgd:
            if K:
                self._horner(self.g_user, self.g_item, self.base_user, self.base_item, -lr * self.alpha, accumulate=True)
            if self.l2:
                ops.rows_scatter_add(self.base_user, user, lrw[0], -lr, ld=D)
                ops.rows_scatter_add(self.base_item, items, lrw[1:3].view(2 * B, D), -lr, ld=D)
        else:
            gu, gv = (self.g_user, self.g_item) if K == 0 else \
                self._horner(self.g_user, self.g_item, self.g_user, self.g_item, self.alpha)
            if self.l2:
                ops.rows_scatter_add(gu, user, lrw[0], 1.0, ld=D)
                ops.rows_scatter_add(gv, items, lrw[1:3].view(2 * B, D), 1.0, ld=D)
            self.steps += 1
            b1, b2 = self.BETAS
            ops.lgcn_adam(self.base_user, gu, self.moments[0], self.moments[1], lr, b1, b2, self.EPS, self.steps)
            ops.lgcn_adam(self.base_item, gv, self.moments[2], self.moments[3], lr, b1, b2, self.EPS, self.steps)
        self.forward()

    def check_errors(self):
        from .collaborative._scorer import check_err_flag
        check_err_flag(self.err, "fit_lightgcn")
