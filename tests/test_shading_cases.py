"""CPU tests of tests/shading_cases.py: the launch rule of the lens shading kernel restated, what the table of its long
launches reaches, and -- from the model alone -- that the frames and tables of the GPU tests (tests/test_gpu_shading.py)
show a segment that starts with the wrong vertical weight or keeps its first node rows."""
import os
import re

import numpy as np
import pytest

import dpc_cases as dc
import shading_cases as shc
import shading_model as shm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "gst-plugins-bad_amd", "csrc", "mibayer_internal.h")).read()
    for name, value in (("kShadeAhead", shc.AHEAD), ("kShadeMaxRows", shc.MAX_ROWS), ("kShadeMinRows", shc.MIN_ROWS),
                        ("kShadeSpread", shc.SPREAD), ("kShadeMaxNodes", shm.MAX_NODES)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), text), name
    kern = open(os.path.join(ROOT, "gst-plugins-bad_amd", "csrc", "mibayer_kernels.hip")).read()
    body = kern[kern.index("mosaic_shade_kernel (ShadeParams p)"):kern.index("hipError_t launch_shade")]
    assert "strip * %du + threadIdx.x" % shc.STRIP_DWORDS in body
    rule = kern[kern.index("hipError_t launch_shade"):kern.index("defective pixel correction")]
    assert "p.y1 - (p.y0 & ~1)" in rule and "rows = (rows + 1) & ~1LL;" in rule


def test_the_rule():
    # a small launch walks 16 rows, the measured one (64 frames of 4K) 64; an odd value is rounded up
    assert shc.seg_rows(3840, 0, 1, 0, 2160) == 16 and shc.seg_rows(3840, 0, 64, 0, 2160) == 64
    assert shc.seg_rows(10, 0, 512, 0, 35) == 18 and dc.seg_rows(10, 0, 512, 0, 35) == 17
    assert shc.segments(1030, 37, 0) == [(0, 16), (16, 32), (32, 37)]
    # rows are counted from the even row at or under y0
    assert shc.segments(266, 116, 0, 1, 17, 59) == [(16, 32), (32, 48), (48, 59)]
    assert shc.seg_rows(10, 0, 1024, 1, 32) == 32 and shc.seg_rows(10, 0, 1024, 2, 32) == 30


def test_long_cases_reach_every_segment_length_and_cell_phase():
    rows = [shc.seg_rows(c.w, c.bits, c.nframes, 0, c.h) for c in shc.LONG_CASES]
    assert rows == [18, 18, 26, 26, 44, 44, 64, 64, 64, 18] and set(rows) == {18, 26, 44, 64}
    # the shapes are those of the other two passes' tables
    assert {c[:5] for c in shc.LONG_CASES} == {tuple(c) for c in dc.LONG_CASES}
    phases = {}
    for c, r in zip(shc.LONG_CASES, rows):
        phases.setdefault(c.ky, {}).setdefault(r, set()).update(shc.cell_phases(c))
    assert phases == {2: {18: {0, 2}, 44: {0}}, 3: {18: {0, 2, 4, 6}, 26: {0, 2}, 44: {0, 4}}, 4: {64: {0}},
                      5: {26: {0, 26}}, 8: {64: {0, 64, 128}}}
    # what the 16-row segments of a small launch cannot give: a phase that is no multiple of 16
    small = {ya & ((1 << ky) - 1) for ky in range(2, 9) for h in (3, 5, 37, 40, 116, 259) for ya, _ in shc.segments(1030, h, 0)}
    assert all(p % 16 == 0 for p in small) and small == {0, 16, 32, 48, 64, 80, 96, 112, 128, 144, 160, 176, 192, 208, 224, 240}
    assert {p for by_rows in phases.values() for ps in by_rows.values() for p in ps if p % 16} == {2, 4, 6, 26}
    # cells of 4 rows: a seam two rows after a segment's start; and a case whose every segment seam is a cell seam
    assert shc.case_segments(shc.LONG_CASES[0]) == [(0, 18), (18, 35)] and 18 + 2 == 5 << 2
    assert shc.cell_phases(shc.LONG_CASES[5]) == {0} and len(shc.case_segments(shc.LONG_CASES[5])) == 2
    # a first stretch shorter than kShadeAhead before a seam, and longer ones
    first = {((ya >> c.ky) + 1 << c.ky) - ya for c in shc.LONG_CASES for ya, _ in shc.case_segments(c)}
    assert {2, 4, 6} <= first and any(s > shc.AHEAD for s in first)
    # a segment seam two rows before a cell seam
    assert any((ya + 2) % (1 << c.ky) == 0 for c in shc.LONG_CASES for ya, _ in shc.case_segments(c)[1:])
    # one cell row for the whole frame, twice; a dword per cell column; one segment
    assert [c.ky for c in shc.LONG_CASES].count(8) == 2 and all(c.h <= 256 for c in shc.LONG_CASES)
    assert any(c.kx == 2 and not c.bits for c in shc.LONG_CASES) and {c.kx for c in shc.LONG_CASES} == {2, 3, 4, 5}
    assert sum(len(shc.case_segments(c)) == 1 for c in shc.LONG_CASES) == 1
    assert max(shc.strips(c.w, c.bits) * c.nframes - 1 for c in shc.LONG_CASES) >= 1023
    for c in shc.LONG_CASES:
        nx, ny = shm.nodes(c.w, c.h, c.kx, c.ky)
        assert nx <= shm.MAX_NODES and ny <= shm.MAX_NODES
        assert c.w * c.h * c.nframes <= (5_000_000 if c == shc.WIDE_LONG_CASE else 1_000_000), shc.case_id(c)
    assert len(set(map(shc.case_id, shc.LONG_CASES))) == len(shc.LONG_CASES)


@pytest.mark.parametrize("case", shc.LONG_CASES, ids=shc.case_id)
def test_long_frames_can_tell_a_wrong_weight_and_stale_nodes(case):
    """random samples under the site planes of the GPU test: a vertical weight that restarts at the segment's first row
    shows in every segment that starts inside a cell row, node rows kept from the segment's first cell row show in every
    segment that crosses a cell-row seam -- and in no other"""
    depth = case.bits or 8
    vmax = (1 << depth) - 1
    rng = np.random.default_rng([9, case.w, case.h, case.ky])
    table = shc.site_planes(case.w, case.h, case.kx, case.ky, rng)
    black = (vmax // 16, vmax // 20, vmax // 18, vmax // 14)
    S = rng.integers(0, vmax + 1, (case.h, case.w))
    want = shm.apply(S, table, case.kx, case.ky, black, depth)
    assert np.array_equal(shc.apply_with(S, table, case.kx, case.ky, black, depth, *shc.rows_of(case)), want)
    restart = shc.apply_with(S, table, case.kx, case.ky, black, depth, *shc.rows_of(case, "restart"))
    stale = shc.apply_with(S, table, case.kx, case.ky, black, depth, *shc.rows_of(case, "stale"))
    ch = 1 << case.ky
    for ya, yb in shc.case_segments(case):
        assert (restart[ya:yb] != want[ya:yb]).any() == bool(ya & (ch - 1)), (shc.case_id(case), ya)
        assert (stale[ya:yb] != want[ya:yb]).any() == shc.crosses_a_cell_seam(case, (ya, yb)), (shc.case_id(case), ya)
