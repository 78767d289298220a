# -*- coding: utf-8 -*-
"""What tests/test_gpu_large_offsets.py can see, shown without a GPU.  A table is modelled as a counter-based hash of
the element offset (nothing large is allocated), a gather is written with its offset computed in 64 bits and three
narrowed ways, and the ids band_rows yields must make every narrowing visible on exactly the bands it breaks:

    int32 bytes     breaks b1, b2, b3   (row * D * 4 >= 2^31)
    uint32 bytes    breaks b2, b3       (row * D * 4 >= 2^32)
    int32 elements  breaks b3           (row * D >= 2^31)

(The narrowed gathers are numpy on the hash; no narrowed kernel is ever run: a signed wrap addresses memory outside
the allocation.)"""
import numpy as np
import pytest
import torch

import large_tables as lt

WIDTHS = [64, 32, 10]  # the widths tests/test_gpu_large_offsets.py uses (16-byte lanes, Linear's, the scalar tail)
PER_BAND = [73, 3998]  # flag_mode_case's 300 and 16 000 occurring users: 4 * per_band + 8


def value(off):
    """The table: a 32-bit hash (splitmix64 finaliser) of the int64 ELEMENT offset, defined for any offset, also one
    outside the table."""
    z = np.asarray(off, dtype=np.int64).astype(np.uint64)
    with np.errstate(over="ignore"):
        z = (z + np.uint64(0x9E3779B97F4A7C15))
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
    return ((z ^ (z >> np.uint64(31))) & np.uint64(0xFFFFFFFF)).astype(np.uint32)


def _wrap(x, bits, signed):
    x = np.asarray(x, dtype=np.int64) & ((1 << bits) - 1)
    return np.where(x >= 1 << (bits - 1), x - (1 << bits), x) if signed else x


def gather(rows, D, n_rows, how):
    """value at row * D + d for d < D, with the row's base offset computed as `how` says."""
    rows = np.asarray(rows, dtype=np.int64)
    if how == "right":
        base = rows * D
    elif how == "int32 bytes":
        base = _wrap(rows * D * 4, 32, True) // 4        # (a multiple of 4 either way: the division is exact)
    elif how == "uint32 bytes":
        base = _wrap(rows * D * 4, 32, False) // 4
    elif how == "int32 elements":
        base = _wrap(rows * D, 32, True) % (n_rows * D)  # wrap, then reduce modulo the table size
    else:
        raise ValueError(how)
    return value(base[:, None] + np.arange(D, dtype=np.int64)[None, :])


BREAKS = {"int32 bytes": {1, 2, 3}, "uint32 bytes": {2, 3}, "int32 elements": {3}}


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("per_band", PER_BAND)
def test_band_rows_properties(D, per_band):
    n = lt.n_rows_for(D)
    assert n == 2 ** 31 // D + 4099 and (n - 1) * D >= 2 ** 31 and n * D < 2 ** 32
    rows = lt.band_rows(n, D, per_band, seed=D)
    assert rows.dtype == np.int64 and rows.size == 4 * per_band + 8
    assert (np.diff(rows) > 0).all() and rows[0] == 0 and rows[-1] == n - 1  # sorted, distinct, in range
    band = lt.band_of(rows, D)
    counts = np.bincount(band, minlength=4)
    assert (counts >= per_band).all() and counts.sum() == rows.size
    for b in lt.BOUNDARIES:  # the last row below and the first row at every boundary
        r = -(-b // D)
        assert r * D >= b > (r - 1) * D and r in rows and r - 1 in rows
        assert lt.band_of([r - 1], D)[0] + 1 == lt.band_of([r], D)[0]
    lt.assert_covers(rows, n, D)
    for drop in (rows[band != 2], rows[rows != -(-(1 << 30) // D)], rows[1:], rows[:-1]):
        with pytest.raises(AssertionError):  # a band, a boundary row, row 0, the last row
            lt.assert_covers(drop, n, D)
    assert np.array_equal(rows, lt.band_rows(n, D, per_band, seed=D))       # the seed decides
    assert not np.array_equal(rows, lt.band_rows(n, D, per_band, seed=D + 1))


@pytest.mark.parametrize("D", WIDTHS)
@pytest.mark.parametrize("per_band", PER_BAND)
@pytest.mark.parametrize("how", sorted(BREAKS))
def test_each_narrowed_offset_is_seen_on_exactly_its_bands(D, per_band, how):
    n = lt.n_rows_for(D)
    rows = lt.band_rows(n, D, per_band, seed=D)
    band = lt.band_of(rows, D)
    right, wrong = gather(rows, D, n, "right"), gather(rows, D, n, how)
    differs = (right != wrong).any(axis=1)
    broken = np.isin(band, sorted(BREAKS[how]))
    assert broken.any() and (~broken).any()
    assert differs[broken].all(), f"{how}: a row of a band it breaks reads the right values"
    assert not differs[~broken].any(), f"{how}: a row below its bands reads wrong values"
    # the same through the checker the GPU tests use: the compacted rows of the gathers, compared row by row
    small_rows, (remap,) = lt.compact([rows[::-1]])
    assert np.array_equal(small_rows, rows) and np.array_equal(small_rows[remap], rows[::-1])
    per_band_seen = {b: bool(differs[band == b].all()) for b in range(4)}
    assert per_band_seen == {b: b in BREAKS[how] for b in range(4)}


@pytest.mark.parametrize("D", WIDTHS)
def test_band_places_put_the_ids_that_occur_on_the_boundaries(D):
    n, n_small = lt.n_rows_for(D), 300
    ids = np.random.RandomState(D).randint(0, n_small, 400)  # about 80 of the 300 never occur
    place = lt.band_places(ids, n_small, n, D, seed=D)
    assert np.array_equal(np.sort(place), lt.band_rows(n, D, (n_small - 8) // 4, seed=D))
    assert np.unique(ids).size < n_small
    lt.assert_covers(place[ids], n, D)
    per_band = np.bincount(lt.band_of(np.unique(place[ids]), D), minlength=4)
    assert per_band.min() >= (np.unique(ids).size - 8) // 4  # the ids that occur are dealt evenly over the bands
    with pytest.raises(AssertionError):
        lt.assert_covers(lt.band_rows(n, D, (n_small - 8) // 4, seed=D)[ids[:40]], n, D)


def test_compact_and_gather_small():
    a, b = np.array([7, 3, 7, 100]), np.array([[3, 5], [100, 0]])
    rows, (ma, mb) = lt.compact([a, b])
    assert rows.tolist() == [0, 3, 5, 7, 100] and np.array_equal(rows[ma], a) and np.array_equal(rows[mb], b)
    t = torch.arange(101 * 3, dtype=torch.float32).reshape(101, 3)
    assert np.array_equal(lt.gather_small(t, rows), t.numpy()[rows])


def test_fill_and_checksums_see_one_changed_bit(monkeypatch):
    monkeypatch.setattr(lt, "CHUNK_ELEMS", 50)  # several chunks, the last one short
    t = lt.fill(torch.empty((37, 10)), seed=4)
    assert bool((t != 0).all()) and np.unique(t.numpy()).size == t.numel() and abs(float(t.std()) - 0.3) < 0.05
    assert torch.equal(t, lt.fill(torch.empty((37, 10)), seed=4)) and not torch.equal(t, lt.fill(torch.empty((37, 10)), seed=5))
    cs = lt.row_checksums(t)
    assert cs.dtype == torch.int64 and torch.equal(cs, t.view(torch.int32).sum(dim=1, dtype=torch.int64))
    after = t.clone()
    after[5] += 1.0
    after[11, 3] = float(np.nextafter(np.float32(after[11, 3]), np.float32(9)))  # one ulp
    cs2 = lt.row_checksums(after)
    lt.assert_untouched(cs, cs2, [5, 11])
    lt.assert_untouched(cs, cs, [])
    for touched in ([5], [11], []):
        with pytest.raises(AssertionError, match="rows outside the call's ids changed"):
            lt.assert_untouched(cs, cs2, touched)
