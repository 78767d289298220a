# -*- coding: utf-8 -*-
"""tests/row_shapes.py against csrc/score_kernels.h (no GPU): the same set of shapes, the same width -> shape mapping,
the same unsupported widths.  A shape added to TRS_ROW_SHAPES without a pair of widths in row_shapes.WIDTHS fails
here, so the matrix of tests/test_gpu_row_shapes.py cannot silently fall behind the header."""
import os
import re

import row_shapes
from conftest import ROOT

HEADER = os.path.join(ROOT, "torchrecsys_amd", "csrc", "score_kernels.h")


def header_text():
    with open(HEADER) as f:
        return f.read()


def header_shapes(text):
    """The X(v, g, k) entries of `#define TRS_ROW_SHAPES(X)`, continuation lines included."""
    m = re.search(r"#define\s+TRS_ROW_SHAPES\(X\)((?:.*\\\n)*.*)\n", text)
    assert m, "TRS_ROW_SHAPES not found in score_kernels.h"
    entries = re.findall(r"X\(\s*(\d+)\s*,\s*(\d+)\s*,\s*(\d+)\s*\)", m.group(1))
    assert entries
    return [tuple(int(x) for x in e) for e in entries]


def test_header_parser_sees_an_added_shape():
    text = header_text()
    grown = text.replace("X(1, 4, 1)", "X(4, 1, 1) X(1, 4, 1)", 1)
    assert grown != text
    assert set(header_shapes(grown)) - set(row_shapes.WIDTHS) == {(4, 1, 1)}


def test_width_table_matches_the_header():
    shapes = header_shapes(header_text())
    assert len(shapes) == len(set(shapes)), "a shape is listed twice in TRS_ROW_SHAPES"
    assert set(shapes) == set(row_shapes.WIDTHS), (sorted(set(shapes) ^ set(row_shapes.WIDTHS)))
    for shape, (small, large) in row_shapes.WIDTHS.items():
        assert row_shapes.pick_row_cfg(small) == shape, (shape, small)
        assert row_shapes.pick_row_cfg(large) == shape, (shape, large)
        assert small < large
        # smallest and largest: one step outside lands on another shape (or on no shape at all)
        assert row_shapes.pick_row_cfg(small - 1) != shape and row_shapes.pick_row_cfg(large + 1) != shape
        v, g, k = shape
        assert small < v * g * k and not row_shapes.is_full(small)       # the small width is ragged
        assert row_shapes.is_full(large) == (v == 4)                     # the large one fills the VEC = 4 shapes
    # every width 1..1024 the Python restatement supports lands on a listed shape (the header's static_assert, restated)
    for D in range(1, 1025):
        c = row_shapes.pick_row_cfg(D)
        assert c is None or c in row_shapes.WIDTHS, D
    assert set(row_shapes.variant(D) for D in row_shapes.ALL) == row_shapes.ALL_VARIANTS
    assert len(row_shapes.ALL) == 24 and len(row_shapes.RAGGED) == 12 and len(row_shapes.FULL) == 8


def test_unsupported_widths_match_the_message_of_row_cfg_for():
    m = re.search(r'unsupported n_factors D=%d \(need (\d+)\.\.(\d+); D %% 4 != 0 only up to (\d+)\)', header_text())
    assert m, "row_cfg_for's message changed: restate it here and in row_shapes.pick_row_cfg"
    lo, hi, odd_hi = (int(x) for x in m.groups())

    def supported_by_message(D):
        return lo <= D <= hi and (D % 4 == 0 or D <= odd_hi)

    for D in (0, 257, 1023, 1025):
        assert row_shapes.pick_row_cfg(D) is None and not supported_by_message(D), D
    for D in range(-3, 1100):
        assert (row_shapes.pick_row_cfg(D) is not None) == supported_by_message(D), D
