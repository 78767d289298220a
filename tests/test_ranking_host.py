# -*- coding: utf-8 -*-
"""Retrieval C-ABI (include/trs.h "retrieval") without a GPU: symbols are bound, arguments are validated on the host
before any launch, the workspace helper is monotone."""
import ctypes

from torchrecsys_amd import _lib

NEW = ("trs_item_fold_bytes", "trs_item_fold", "trs_retrieve_workspace_bytes", "trs_retrieve_topk", "trs_mask_seen",
       "trs_rank_metrics")


def _err():
    return _lib.load().trs_last_error().decode()


def _tables(n_users=10, n_items=20, D=8):
    """A trs_tables struct with non-NULL (never dereferenced) pointers: validation only."""
    T = _lib.TrsTables()
    T.user = T.item = T.user_lin = T.item_lin = 0x1000
    T.n_users, T.n_items, T.D, T.M = n_users, n_items, D, 0
    return T


def _topk(lib, T, k, ws_bytes, fold_bytes=None, ws=0x1000):
    fb = (lib.trs_item_fold_bytes(T.n_items, T.D) if T is not None else 1 << 20) if fold_bytes is None else fold_bytes
    return lib.trs_retrieve_topk(_lib.TRS_NET_FM, ctypes.byref(T) if T is not None else None, 0x1000, fb, 0x1000, 5,
                                 k, None, None, 0x1000, 0x1000, None, ws, ws_bytes, None)


def test_new_symbols_exported_and_bound():
    lib = _lib.load()
    assert lib.trs_abi_version() == _lib.ABI_VERSION == 6
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in _lib.PROTOTYPES, name
        assert hasattr(raw, name), name
    assert ctypes.sizeof(_lib.TrsCsr) == 24


def test_retrieve_topk_rejects_bad_arguments():
    lib = _lib.load()
    T = _tables()
    ws = lib.trs_retrieve_workspace_bytes(5, 10)
    assert ws > 0
    assert _topk(lib, None, 10, ws) == -1 and "NULL" in _err()
    T0 = _tables()
    T0.user = None
    assert _topk(lib, T0, 10, ws) == -1 and "user table" in _err()
    assert _topk(lib, T, 0, ws) == -1 and "k=0" in _err()
    K1 = _lib.RETRIEVE_KMAX + 1
    big = _tables(n_items=1000)
    assert _topk(lib, big, K1, lib.trs_retrieve_workspace_bytes(5, K1)) == -1 and f"k={K1}" in _err()
    assert _topk(lib, T, 10, ws - 8) == -1 and "workspace too small" in _err()
    assert _topk(lib, T, 10, ws, fold_bytes=16) == -1 and "fold buffer too small" in _err()
    assert _topk(lib, _tables(D=_lib.RETRIEVE_DMAX + 1), 10, ws) == -1 and "D=" in _err()


def test_rank_metrics_and_mask_seen_reject_bad_arguments():
    lib = _lib.load()
    rel = _lib.TrsCsr(0x1000, 0x1000, 4)
    assert lib.trs_rank_metrics(0x1000, 3, 0, 0x1000, ctypes.byref(rel), 0x1000, None) == -1 and "k=0" in _err()
    assert lib.trs_rank_metrics(0x1000, 3, 5, 0x1000, None, 0x1000, None) == -1 and "NULL" in _err()
    assert lib.trs_rank_metrics(None, 3, 5, 0x1000, ctypes.byref(rel), 0x1000, None) == -1 and "NULL" in _err()
    bad = _lib.TrsCsr(None, 0x1000, 4)
    assert lib.trs_rank_metrics(0x1000, 3, 5, 0x1000, ctypes.byref(bad), 0x1000, None) == -1 and "CSR" in _err()
    assert lib.trs_mask_seen(0x1000, 3, 10, 0x1000, None, None) == -1 and "NULL" in _err()
    assert lib.trs_item_fold(_lib.TRS_NET_FM, None, None, 0x1000, 1 << 20, None) == -1 and "NULL" in _err()


def test_workspace_bytes_monotone():
    lib = _lib.load()
    prev = 0
    for n_q in [1, 2, 31, 32, 33, 100, 1000, 16384, 16385, 100_000, 1 << 20]:
        b = lib.trs_retrieve_workspace_bytes(n_q, 10)
        assert b >= prev and b >= n_q * 10 * 8
        prev = b
    for n_q in [1, 33, 5000, 1 << 20]:
        prev = 0
        for k in range(1, _lib.RETRIEVE_KMAX + 1):
            b = lib.trs_retrieve_workspace_bytes(n_q, k)
            assert b >= prev
            prev = b
    assert lib.trs_item_fold_bytes(1000, 64) > 1000 * 64 * 4
    assert lib.trs_item_fold_bytes(1000, _lib.RETRIEVE_DMAX + 1) == 0
