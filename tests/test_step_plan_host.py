# -*- coding: utf-8 -*-
"""What trs_train_steps_sgd accepts and refuses, host side (no GPU): its arguments are resolved once per call into one
of four forms (csrc/fast_step.hip, resolve_step_plan), and every check runs before anything touches the device.  With
n_steps = 0 a call validates and returns, so dummy non-NULL pointers are enough (as in tests/test_long_run_host.py).
Every row below is one of the four forms in a valid shape, changed in ONE place; it states accept or refuse and, for a
refusal, a fragment of the message.  The kernels each form launches: tests/test_gpu_row_shapes.py."""
import ctypes as C

import pytest

from torchrecsys_amd import _lib, ops

P = 0x1000  # a non-NULL "device pointer": validation never dereferences it
SGD, SPARSE_ADAM, ADAGRAD = 0, 1, 2


class Case:
    """A trs_train_args with everything it points to kept alive."""

    def __init__(self, form, D=8, M=0):
        T = self.T = _lib.TrsTables()
        T.user = T.item = T.user_lin = T.item_lin = P
        T.n_users, T.n_items, T.D, T.M = 10, 10, D, 0
        a = self.a = _lib.TrsTrainArgs()
        a.net, a.n_steps, a.tables, a.batch, a.lr = ops.NET_ID["fm"], 0, C.pointer(T), 16, 0.05
        a.first_stamp = 1
        a.user_buf_dev = a.pos_buf_dev = a.neg_buf_dev = a.gz_buf_dev = a.du_buf_dev = a.loss_sums_dev = P
        a.scratch_dev = P
        self.count = C.c_uint32(0)
        if form == "stream":  # marks, ids derived from the resident stream
            a.stream_ui_dev, a.N = P, 64
        elif form in ("sorted_marks", "sorted"):
            a.sorted_keys_dev = a.sorted_vals_dev = P
            a.key_bytes = 4
            if form == "sorted":
                a.user_dup_flags_dev = a.ustage_buf_dev = a.sorted_ukeys_dev = a.sorted_uvals_dev = P
                a.ukey_bytes = 4
        elif form == "flags":
            a.user_dup_flags_dev = a.item_dup_flags_dev = a.ustage_buf_dev = P
        else:
            assert form == "marks", form
        if M:
            self.metadata(M)

    def no_pairs(self):
        self.a.sorted_ukeys_dev = self.a.sorted_uvals_dev = None
        self.a.ukey_bytes = 0

    def opt(self, kind, s2=True):
        o = self.o = _lib.TrsOpt()
        o.kind, o.lr, o.beta1, o.beta2, o.eps, o.cut_capacity = kind, 0.01, 0.9, 0.999, 1e-8, 32
        o.user_s1 = o.item_s1 = o.user_lin_s1 = o.item_lin_s1 = o.gacc = o.gacc_lin = o.cut_rows = o.cut_count = P
        if s2:
            o.user_s2 = o.item_s2 = o.user_lin_s2 = o.item_lin_s2 = P
        for m in range(self.T.M):
            o.meta_s1[m] = o.meta_s2[m] = o.meta_lin_s1[m] = o.meta_lin_s2[m] = P
            o.meta_gacc[m] = o.meta_gacc_lin[m] = o.meta_cut_rows[m] = o.meta_cut_count[m] = P
        self.a.opt = C.pointer(o)

    def metadata(self, M, staging=True):
        """M metadata columns with sorted references and their id arrays."""
        self.T.M = M
        for m in range(M):
            self.T.meta[m] = self.T.meta_lin[m] = P
            self.T.n_meta[m] = 5
        if staging:
            ms = self.ms = _lib.TrsMetaStage()
            ms.item_meta_tab = ms.xstage = ms.lin_scratch = ms.pos_meta_ids = ms.neg_meta_ids = P
            for m in range(M):
                ms.sorted_keys[m] = ms.sorted_vals[m] = P
            self.a.meta = C.pointer(ms)

    def sync(self):
        self.a.sync_dev, self.a.sync_count_host = P, C.pointer(self.count)


def _set(**fields):
    def change(c):
        for k, v in fields.items():
            setattr(c.a, k, v)
    return change


def _tables(**fields):
    def change(c):
        for k, v in fields.items():
            setattr(c.T, k, v)
    return change


def _seq(*changes):
    def change(c):
        for ch in changes:
            ch(c)
    return change


OK = None
# (id, form, keyword arguments of Case, the one change, OK or a fragment of the refusal)
ROWS = [
    # ---- the four forms, each in its minimal valid shape
    ("marks", "marks", {}, None, OK),
    ("marks_without_scratch", "marks", {}, _set(scratch_dev=None), OK),
    ("marks_from_stream_dynamic", "stream", {}, None, OK),
    ("marks_from_stream_static_negatives", "stream", {}, _set(neg_static_dev=P), OK),
    ("sorted_marks", "sorted_marks", {}, None, OK),
    ("sorted_with_user_pairs", "sorted", {}, None, OK),
    ("sorted_pairs_omitted_plain_sgd", "sorted", {}, Case.no_pairs, OK),
    ("sorted_item_flags", "sorted", {}, _set(item_dup_flags_dev=P), OK),
    ("sorted_item_flags_pairs_omitted", "sorted", {}, _seq(Case.no_pairs, _set(item_dup_flags_dev=P)), OK),
    ("sorted_sparse_adam", "sorted", {}, lambda c: c.opt(SPARSE_ADAM), OK),
    ("sorted_adagrad", "sorted", {}, lambda c: c.opt(ADAGRAD, s2=False), OK),
    ("sorted_opt_struct_naming_sgd", "sorted", {}, lambda c: c.opt(SGD, s2=False), OK),
    ("sorted_meta", "sorted", {"M": 2}, None, OK),
    ("sorted_meta_adaptive", "sorted", {"M": 2, "D": 64}, lambda c: c.opt(SPARSE_ADAM), OK),
    ("flags_two_launches", "flags", {}, None, OK),
    ("flags_with_sync", "flags", {}, Case.sync, OK),
    ("flags_with_sync_and_n_flagged", "flags", {}, _seq(Case.sync, _set(n_flagged_dev=P)), OK),
    ("flags_n_flagged_without_sync", "flags", {}, _set(n_flagged_dev=P), OK),
    # ---- refusals on the sorted side
    ("sorted_with_a_stream", "sorted", {}, _set(stream_ui_dev=P, N=64), "presorted mode needs the epoch's id arrays"),
    ("sorted_marks_with_a_stream", "sorted_marks", {}, _set(stream_ui_dev=P, N=64), "presorted mode needs"),
    ("sorted_without_scratch", "sorted", {}, _set(scratch_dev=None), "presorted mode needs the epoch's id arrays, scratch"),
    ("sorted_without_vals", "sorted", {}, _set(sorted_vals_dev=None), "presorted mode needs"),
    ("sorted_key_bytes_0", "sorted", {}, _set(key_bytes=0), "presorted mode needs"),
    ("user_flags_without_ustage", "sorted", {}, _set(ustage_buf_dev=None), "user-duplicate flags need the staging buffer"),
    ("user_pairs_without_uvals", "sorted", {}, _set(sorted_uvals_dev=None), "user-duplicate flags need the staging buffer"),
    ("user_pairs_ukey_bytes_0", "sorted", {}, _set(ukey_bytes=0), "user-duplicate flags need the staging buffer"),
    ("pairs_omitted_with_adaptive_rule", "sorted", {}, _seq(Case.no_pairs, lambda c: c.opt(SPARSE_ADAM)),
     "plain SGD without metadata may omit the pairs"),
    ("pairs_omitted_with_metadata", "sorted", {"M": 1}, Case.no_pairs, "plain SGD without metadata may omit the pairs"),
    # ---- item flags, adaptive rules, SparseAdam
    ("item_flags_with_adaptive_rule", "sorted", {}, _seq(_set(item_dup_flags_dev=P), lambda c: c.opt(ADAGRAD)),
     "item-duplicate flags need the presorted plain-SGD step"),
    ("item_flags_with_metadata", "sorted", {"M": 1}, _set(item_dup_flags_dev=P), "item-duplicate flags need"),
    ("item_flags_alone", "marks", {}, _set(item_dup_flags_dev=P), "item-duplicate flags need"),
    ("item_flags_on_sorted_marks", "sorted_marks", {}, _set(item_dup_flags_dev=P), "item-duplicate flags need"),
    ("adaptive_without_user_flags", "sorted_marks", {}, lambda c: c.opt(SPARSE_ADAM),
     "adaptive rules need the presorted mode with user-duplicate flags"),
    ("adaptive_on_marks", "marks", {}, lambda c: c.opt(ADAGRAD), "adaptive rules need the presorted mode"),
    ("bad_opt_kind", "sorted", {}, lambda c: c.opt(7), "bad opt->kind"),
    ("sparse_adam_without_s2", "sorted", {}, lambda c: c.opt(SPARSE_ADAM, s2=False), "SparseAdam needs exp_avg_sq tables"),
    ("adaptive_without_cut_scratch", "sorted", {}, _seq(lambda c: c.opt(ADAGRAD), lambda c: setattr(c.o, "cut_rows", None)),
     "optimiser state / cut-run scratch is NULL"),
    # ---- the flags form
    ("flags_with_a_stream", "flags", {}, _set(stream_ui_dev=P, N=64), "the flag mode takes given ids"),
    ("flags_with_adaptive_rule", "flags", {}, lambda c: c.opt(SPARSE_ADAM), "the flag mode takes given ids"),
    ("flags_without_ustage", "flags", {}, _set(ustage_buf_dev=None), "the flag mode takes given ids"),
    # ---- metadata
    ("meta_tables_without_staging", "sorted", {}, lambda c: c.metadata(1, staging=False),
     "metadata tables need the metadata staging"),
    ("staging_without_meta_tables", "sorted", {"M": 1}, _tables(M=0), "metadata tables need the metadata staging"),
    ("meta_without_sorted_references", "marks", {"M": 1}, None, "metadata scorers run on the presorted step"),
    ("meta_on_sorted_marks", "sorted_marks", {"M": 1}, None, "metadata scorers run on the presorted step"),
    ("meta_in_flag_mode", "flags", {"M": 1}, None, "the flag mode takes given ids"),
    ("adaptive_meta_at_D_48", "sorted", {"M": 2, "D": 48}, lambda c: c.opt(SPARSE_ADAM), "D in {32, 64, 128, 256}"),
    ("adaptive_meta_column_state_missing", "sorted", {"M": 2, "D": 64},
     _seq(lambda c: c.opt(ADAGRAD), lambda c: c.o.meta_gacc.__setitem__(1, None)),
     "optimiser state of metadata column 1 is NULL"),
    ("meta_without_xstage", "sorted", {"M": 1}, lambda c: setattr(c.ms, "xstage", None), "metadata staging buffer is NULL"),
    ("meta_unsorted_without_gradient_staging", "sorted", {"M": 1}, lambda c: c.ms.sorted_keys.__setitem__(0, None),
     "metadata gradient staging is NULL"),
    ("meta_sorted_column_missing", "sorted", {"M": 2}, lambda c: c.ms.sorted_vals.__setitem__(1, None),
     "sorted references of metadata column 1 are NULL"),
    ("meta_table_missing", "sorted", {"M": 2}, lambda c: c.T.meta.__setitem__(1, None), "metadata table 1 is NULL"),
    # ---- the stream
    ("stream_window_past_N", "stream", {}, _set(first_pos=60, n_steps=1), "outside the stream of 64 rows"),
    ("stream_negative_first_pos", "stream", {}, _set(first_pos=-1), "outside the stream"),
    ("dynamic_sampling_with_one_item", "stream", {}, _tables(n_items=1), "dynamic sampling needs n_items >= 2"),
    ("static_negatives_with_one_item", "stream", {}, _seq(_tables(n_items=1), _set(neg_static_dev=P)), OK),
    # ---- the rest
    ("batch_0", "marks", {}, _set(batch=0), "bad batch / n_steps"),
    ("batch_2_to_the_30", "marks", {}, _set(batch=1 << 30), "bad batch / n_steps"),
    ("negative_n_steps", "marks", {}, _set(n_steps=-1), "bad batch / n_steps"),
    ("bad_loss", "marks", {}, _set(loss=5), "bad loss kind"),
    ("bad_loss_in_flag_mode", "flags", {}, _set(loss=-1), "bad loss kind"),
    ("bad_net", "marks", {}, _set(net=99), "net must be TRS_NET_LINEAR or TRS_NET_FM"),
    ("null_tables", "marks", {}, lambda c: setattr(c.a, "tables", None), "tables is NULL"),
    ("null_table", "marks", {}, _tables(item_lin=None), "NULL table"),
    ("null_buffer", "sorted", {}, _set(du_buf_dev=None), "NULL buffer"),
    ("stamp_0_with_scratch", "marks", {}, _set(first_stamp=0), "stamps must be non-zero and must not wrap"),
    ("stamp_0_without_scratch", "marks", {}, _set(first_stamp=0, scratch_dev=None), OK),
    # ---- the sorted references carry 32-bit keys: nothing ever produced 8-byte ones, and they are refused
    ("key_bytes_8", "sorted", {}, _set(key_bytes=8), "32-bit keys"),
    ("key_bytes_8_on_sorted_marks", "sorted_marks", {}, _set(key_bytes=8), "32-bit keys"),
    ("ukey_bytes_8", "sorted", {}, _set(ukey_bytes=8), "32-bit keys"),
]
WIDE_KEYS = {"key_bytes_8", "key_bytes_8_on_sorted_marks", "ukey_bytes_8"}  # accepted before keys became 32-bit only


def outcome(lib, row):
    """(return code, message) of the row's call."""
    _, form, kw, change, _ = row
    c = Case(form, **kw)
    if change is not None:
        change(c)
    rc = lib.trs_train_steps_sgd(C.byref(c.a), None)
    return rc, (lib.trs_last_error().decode() if rc else "")


def test_the_table_names_every_row_once():
    ids = [r[0] for r in ROWS]
    assert len(ids) == len(set(ids)) and WIDE_KEYS <= set(ids)


@pytest.mark.parametrize("row", ROWS, ids=[r[0] for r in ROWS])
def test_arguments_are_accepted_or_refused_before_the_device_is_touched(row):
    lib = _lib.load()
    rc, msg = outcome(lib, row)
    want = row[4]
    if want is OK:
        assert rc == 0, msg
    else:
        assert rc == -1 and msg.startswith("trs_train_steps_sgd: ") and want in msg, (rc, msg)
        with pytest.raises(_lib.TrsError):
            _lib.check(rc, "trs_train_steps_sgd")
