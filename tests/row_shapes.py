# -*- coding: utf-8 -*-
"""The row shapes (VEC, G, K) of csrc/score_kernels.h restated for the tests: pick_row_cfg in Python and, for every
entry of TRS_ROW_SHAPES, the smallest and the largest width that selects it.  tests/test_row_shapes.py keeps this table
in step with the header; tests/test_gpu_row_shapes.py runs every launcher that dispatches on a row shape at every
width listed here."""


def pick_row_cfg(D):
    """(VEC, G, K) for a row of D floats, None where the C function returns false (row_cfg_for: argument error)."""
    if D < 1 or D > 1024:
        return None
    if D % 4 == 0:
        chunks = D // 4
        if chunks <= 64:
            g = 2
            while g < chunks:
                g <<= 1
            return (4, g, 1)
        return (4, 64, 2 if chunks <= 128 else 4)
    if D <= 4:
        return (1, 4, 1)
    if D <= 16:
        return (1, 16, 1)
    if D <= 64:
        return (1, 64, 1)
    if D <= 256:
        return (1, 64, 4)
    return None


def is_full(D):
    """The launchers' second compile-time split: the lane group covers the row exactly (no tail mask)."""
    v, g, k = pick_row_cfg(D)
    return v * g * k == D


# shape -> (smallest width, largest width).  The small one is ragged for every shape; the large one fills the VEC = 4
# shapes exactly (FULL) and is ragged for the VEC = 1 shapes (a multiple of 4 always takes a VEC = 4 shape).
WIDTHS = {
    (4, 2, 1): (4, 8),
    (4, 4, 1): (12, 16),
    (4, 8, 1): (20, 32),
    (4, 16, 1): (36, 64),
    (4, 32, 1): (68, 128),
    (4, 64, 1): (132, 256),
    (4, 64, 2): (260, 512),
    (4, 64, 4): (516, 1024),
    (1, 4, 1): (1, 3),
    (1, 16, 1): (5, 15),
    (1, 64, 1): (17, 63),
    (1, 64, 4): (65, 255),
}

RAGGED = [small for small, _ in WIDTHS.values()]
LARGE = [large for _, large in WIDTHS.values()]
FULL = [large for large in LARGE if is_full(large)]
ALL = [w for pair in WIDTHS.values() for w in pair]

# every (VEC, G, K, FULL) instantiation a launcher with the FULL split carries: 12 ragged + 8 full
ALL_VARIANTS = {s + (False,) for s in WIDTHS} | {s + (True,) for s in WIDTHS if s[0] == 4}


def variant(D):
    return pick_row_cfg(D) + (is_full(D),)
