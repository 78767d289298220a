# -*- coding: utf-8 -*-
"""Tables whose row offsets pass 32 bits: where to put the ids, how to fill the table, and how to see what a call did
to it.  Imports without a GPU (numpy + torch; nothing here touches a device until it is handed a device tensor).

Every kernel addresses a row as table + row * D.  With fp32 rows that product passes three thresholds at which a
narrowed offset goes wrong, and the bands between them name what a row in them can expose:

    b0  row * D in [0, 2^29)        nothing (control)
    b1  row * D in [2^29, 2^30)     a signed 32-bit BYTE offset
    b2  row * D in [2^30, 2^31)     an unsigned 32-bit BYTE offset
    b3  row * D in [2^31, n * D)    a signed 32-bit ELEMENT offset

tests/test_large_tables_host.py shows (on a hashed table, no allocation) that ids drawn by band_rows make each of the
three narrowings visible on exactly its bands; tests/test_gpu_large_offsets.py runs the kernels on such ids.

Out of scope: the unsigned 32-bit ELEMENT band (2^32 elements and more: 17 GB per table, beyond any shape the project
documents) and 1-wide tables (they reach b1 only from 2^29 rows on)."""
import numpy as np
import torch

BOUNDARIES = (1 << 29, 1 << 30, 1 << 31)  # element offsets at which b1, b2, b3 begin
N_BANDS = 4
CHUNK_ELEMS = 1 << 27  # elements per device-side pass of fill / row_checksums (a 1 GB int64 temporary at most)


def n_rows_for(D):
    """Rows of a "large" table of width D: just past the start of b3, and no multiple of any tile size."""
    return 2 ** 31 // D + 4099


def first_row_at(offset, D):
    """The first row whose element offset row * D is >= offset."""
    return -(-offset // D)


def band_bounds(n_rows, D):
    """[(first row, one past the last row)] of b0 .. b3."""
    edges = [0] + [first_row_at(b, D) for b in BOUNDARIES] + [n_rows]
    assert all(a < b for a, b in zip(edges, edges[1:])), (n_rows, D, "the table does not reach every band")
    return list(zip(edges[:-1], edges[1:]))


def band_of(rows, D):
    """Band index 0 .. 3 of every row, by its element offset row * D."""
    off = np.asarray(rows, dtype=np.int64) * D
    return np.searchsorted(np.asarray(BOUNDARIES, dtype=np.int64), off, side="right")


def boundary_rows(n_rows, D):
    """Row 0, row n_rows - 1, and the last row below and the first row at each of the three boundaries (8 rows)."""
    out = [0, n_rows - 1]
    for b in BOUNDARIES:
        r = first_row_at(b, D)
        out += [r - 1, r]
    return np.unique(np.asarray(out, dtype=np.int64))


def band_rows(n_rows, D, per_band, seed):
    """Sorted distinct row ids: per_band from each of b0 .. b3 and the boundary_rows (4 * per_band + 8 ids).  Drawn
    inside each band; no permutation of n_rows is ever built."""
    rs = np.random.RandomState(seed)
    special = boundary_rows(n_rows, D)
    assert special.size == 8, (n_rows, D)
    picked = [special]
    for lo, hi in band_bounds(n_rows, D):
        taken = special[(special >= lo) & (special < hi)]
        assert hi - lo - taken.size >= per_band, (lo, hi, per_band, "the band has too few rows")
        if hi - lo <= 1 << 20:  # a narrow band (b3 of n_rows_for: 4099 rows): shuffle the band itself
            cand = lo + rs.permutation(hi - lo)
            cand = cand[~np.isin(cand, taken)][:per_band]
        else:                   # a wide band: draw, drop repeats, until there are enough
            cand = np.empty(0, dtype=np.int64)
            while cand.size < per_band:
                more = rs.randint(lo, hi, size=2 * per_band + 16).astype(np.int64)
                more = more[~np.isin(more, taken)]
                cand = np.concatenate([cand, more])
                _, first = np.unique(cand, return_index=True)
                cand = cand[np.sort(first)]
            cand = cand[:per_band]
        picked.append(cand.astype(np.int64))
    rows = np.unique(np.concatenate(picked))
    assert rows.size == 4 * per_band + special.size
    return rows


def band_places(ids_small, n_small, n_rows, D, seed):
    """place (n_small,) int64: small id j sits at row place[j] of a table of n_rows rows, the rows being band_rows(n_rows,
    D, (n_small - 8) // 4, seed).  The ids that occur in ids_small take the eight boundary rows first (an id nothing
    names would leave its row unnamed), then the rows drawn inside the bands, dealt one band after the other (so that
    the ids that occur name as many rows of b3 as of b0)."""
    assert n_small >= 8 and (n_small - 8) % 4 == 0, n_small
    special = boundary_rows(n_rows, D)
    drawn = np.setdiff1d(band_rows(n_rows, D, (n_small - 8) // 4, seed), special)
    drawn = drawn.reshape(N_BANDS, -1).T.reshape(-1)  # (sorted: per_band rows of b0, then of b1, ...)
    occurring = np.unique(np.asarray(ids_small, dtype=np.int64))
    assert occurring.size >= special.size and occurring.min() >= 0 and occurring.max() < n_small
    place = np.empty(n_small, dtype=np.int64)
    place[np.concatenate([occurring, np.setdiff1d(np.arange(n_small), occurring)])] = np.concatenate([special, drawn])
    return place


def assert_covers(rows, n_rows, D):
    """The id set reaches all four bands and holds all three boundaries (both sides), row 0 and the last row."""
    rows = np.unique(np.asarray(rows, dtype=np.int64))
    assert rows.min() >= 0 and rows.max() < n_rows
    assert set(band_of(rows, D).tolist()) == set(range(N_BANDS)), "a band without an id"
    assert np.isin(boundary_rows(n_rows, D), rows).all(), "a boundary row is missing"


def _row_chunks(table):
    step = max(1, CHUNK_ELEMS // max(1, table.shape[1]))
    for lo in range(0, table.shape[0], step):
        yield lo, min(lo + step, table.shape[0])


def fill(table, seed, scale=0.3):
    """N(0, scale) over the WHOLE table, generated on the table's device (scale: what the family's small-shape tests
    use; 0.3 is make_case's).  Never zeros: a read that wraps must land on a row with different contents."""
    g = torch.Generator(device=table.device)
    g.manual_seed(int(seed))
    for lo, hi in _row_chunks(table):
        table[lo:hi].normal_(0.0, float(scale), generator=g)
    return table


def row_checksums(table):
    """table.view(torch.int32).sum(dim=1, dtype=torch.int64): an exact, order-free fingerprint per row (one int64 per
    row, no fp64 copy of the table).  Computed in row chunks: the widening sum keeps an int64 image of its input."""
    bits = table.view(torch.int32)
    out = torch.empty(table.shape[0], dtype=torch.int64, device=table.device)
    for lo, hi in _row_chunks(table):
        out[lo:hi] = bits[lo:hi].sum(dim=1, dtype=torch.int64)
    return out


def assert_untouched(before, after, touched_rows, what="table"):
    """before, after: row_checksums of the table around the call.  Every row NOT in touched_rows is bit-identical."""
    assert before.shape == after.shape
    changed = before != after
    changed[torch.as_tensor(np.asarray(touched_rows, dtype=np.int64), device=changed.device)] = False
    n = int(changed.sum().item())
    if n:
        rows = torch.nonzero(changed).reshape(-1)[:8].tolist()
        raise AssertionError(f"{what}: {n} rows outside the call's ids changed, first {rows}")


def compact(ids_list):
    """Rows referenced by any id array -> (sorted unique rows, the arrays remapped to positions in them)."""
    rows = np.unique(np.concatenate([np.asarray(a).reshape(-1) for a in ids_list]))
    return rows, [np.searchsorted(rows, a) for a in ids_list]


def gather_small(table, rows):
    """The referenced rows of a (device) table as a small dense numpy table."""
    idx = torch.as_tensor(np.asarray(rows, dtype=np.int64), device=table.device)
    return table[idx].cpu().numpy()
