"""CPU tests of tests/dpc_cases.py: what the case table of the defective pixel correction kernels reaches, so that the
GPU tests (tests/test_gpu_dpc.py) cannot quietly stop covering a seam when a constant of the kernel changes."""
import os
import re

import numpy as np
import pytest

import dpc_cases as dc
import dpc_model as dm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_constants_are_the_kernels():
    text = open(os.path.join(ROOT, "gst-plugins-bad_amd", "csrc", "mibayer_internal.h")).read()
    for name, value in (("kDpcMaxRows", dc.MAX_ROWS), ("kDpcMinRows", dc.MIN_ROWS), ("kDpcSpread", dc.SPREAD)):
        assert re.search(r"constexpr int %s = %d;" % (name, value), text), name
    kern = open(os.path.join(ROOT, "gst-plugins-bad_amd", "csrc", "mibayer_kernels.hip")).read()
    body = kern[kern.index("mosaic_dpc_kernel (DpcParams p)"):kern.index("mosaic_dpc_list_kernel (DpcParams p)")]
    assert "strip * %du + threadIdx.x" % dc.STRIP_DWORDS in body and "__launch_bounds__ (%d)" % dc.STRIP_DWORDS in kern


def test_the_table_reaches_every_path():
    got = {dc.case_id(c): dc.reaches(c) for c in dc.CASES}
    for bits in (False, True):
        mine = [r for c, r in zip(dc.CASES, got.values()) if bool(c.bits) == bits]
        assert any(r["mirror_overlaps"] for r in mine) and any(r["strip_seam"] and r["wave_seam"] for r in mine)
        assert any(r["segments"] >= 3 and r["short_last_segment"] for r in mine) and any(r["batch"] for r in mine)
    eight = [r for c, r in zip(dc.CASES, got.values()) if not c.bits]
    assert any(r["one_lane"] for r in eight) and any(r["tail"] and r["strip_seam"] for r in eight)
    assert any(not r["tail"] and r["strip_seam"] for r in eight) and any(r["segments"] == 1 and not r["mirror_overlaps"] for r in eight)
    # the two shapes the kernel's geometry asks for: 2 mod 4 across a wave and a strip seam, a few rows past a segment seam
    assert got["1030x37_8_x1"] == dict(one_lane=False, tail=True, wave_seam=True, strip_seam=True, segments=3,
                                       short_last_segment=True, batch=False, mirror_overlaps=False)
    assert got["518x37_12_x1"]["strip_seam"] and got["518x37_12_x1"]["segments"] == 3
    assert dc.segments(1030, 37, 0) == [(0, 16), (16, 32), (32, 37)]
    # a large launch grows its segments: 64 frames of 4K walk 64 rows
    assert dc.seg_rows(3840, 0, 64, 0, 2160) == 64 and dc.seg_rows(3840, 0, 1, 0, 2160) == 16


def test_seams_and_planted_defects():
    assert dc.column_seams(1030, 0) == {"lane": [4, 8, 1024, 1028], "wave": [256, 512, 768], "strip": [1024]}
    assert dc.column_seams(518, 12) == {"lane": [2, 4, 514, 516], "wave": [128, 256, 384], "strip": [512]}
    assert dc.column_seams(4, 0) == {"lane": [], "wave": [], "strip": []} and dc.seam_columns(4, 0) == [0, 1, 2, 3]
    assert dc.seam_rows(1030, 37, 0) == [0, 1, 14, 15, 16, 17, 30, 31, 32, 33, 35, 36]
    cols = dc.seam_columns(1030, 0)
    assert {1022, 1023, 1024, 1025, 1026, 1027, 1028, 1029} <= set(cols) and {254, 255, 256, 257} <= set(cols)
    for case in dc.CASES:
        where = dc.planted(case.w, case.h, case.bits, case.nframes)
        assert len(where) == len(dc.seam_rows(case.w, case.h, case.bits, case.nframes)) * len(dc.seam_columns(case.w, case.bits))
        assert where[:, 0].max() == case.w - 1 and where[:, 1].max() == case.h - 1 and where.min() == 0
        vmax = (1 << (case.bits or 8)) - 1
        assert sorted(set(dc.phase_of(where))) == [0, 1, 2, 3]
        for f in range(case.nframes):
            for phase in range(4):
                S = dc.seam_samples(case, f, phase)
                assert S.min() == 0 and S.max() == vmax and S.shape == (case.h, case.w)
                # the detection finds exactly the planted samples of the phase, and puts each back among its neighbours
                out = dm.correct(S, vmax // 8, vmax // 8)
                changed = {tuple(c) for c in np.argwhere(out != S)[:, ::-1]}
                assert changed == {tuple(c) for c in where[dc.phase_of(where) == phase]}, (dc.case_id(case), phase)
                assert vmax // 4 <= out.min() and out.max() < vmax
            # all of them at once: neighbours hide each other, which is what the list is for
            S = dc.seam_samples(case, f)
            assert len(np.argwhere(dm.correct(S, vmax // 8, vmax // 8) != S)) < len(where)
            listed = dm.correct(S, -1, -1, where)
            assert {tuple(c) for c in np.argwhere(listed != S)[:, ::-1]} <= {tuple(c) for c in where}


# -- the long launches -----------------------------------------------------------------------------------------------------------

def test_long_cases_reach_every_segment_length():
    """workgroups of 17 rows, of an even and of an odd number between the clamps, and of 64 rows by three routes"""
    rows = {c: dc.seg_rows(c.w, c.bits, c.nframes, 0, c.h) for c in dc.LONG_CASES}
    segs = {c: dc.segments(c.w, c.h, c.bits, c.nframes) for c in dc.LONG_CASES}
    assert [rows[c] for c in dc.LONG_CASES] == [17, 17, 26, 25, 43, 64, 64, 64, 17]
    assert set(rows.values()) == {17, 25, 26, 43, 64}
    assert any(18 <= r <= 62 and r % 2 == 0 and c.h % r == 0 for c, r in rows.items())
    assert any(19 <= r <= 63 and r % 2 == 1 for r in rows.values())
    # 64 as the rule gives it; clamped, with a short last segment; clamped, three segments
    at_max = {c: (dc.unclamped_rows(c), len(segs[c])) for c, r in rows.items() if r == dc.MAX_ROWS}
    assert at_max == {dc.Case(10, 64, 0, False, 1024): (64, 1), dc.Case(6, 67, 12, False, 1000): (65, 2),
                      dc.Case(14, 131, 0, False, 512): (65, 3)}
    assert segs[dc.Case(6, 67, 12, False, 1000)] == [(0, 64), (64, 67)]
    assert segs[dc.Case(14, 131, 0, False, 512)] == [(0, 64), (64, 128), (128, 131)]
    assert segs[dc.Case(10, 35, 0, False, 512)] == [(0, 17), (17, 34), (34, 35)] == segs[dc.WIDE_LONG_CASE]
    assert segs[dc.Case(6, 70, 0, False, 256)] == [(0, 17), (17, 34), (34, 51), (51, 68), (68, 70)]
    assert segs[dc.Case(10, 52, 0, False, 512)] == [(0, 26), (26, 52)]
    assert segs[dc.Case(8, 33, 16, True, 800)] == [(0, 25), (25, 33)]
    assert segs[dc.Case(10, 45, 0, False, 1000)] == [(0, 43), (43, 45)]
    # odd segment starts, last segments of 1, 2 and 3 rows, one segment longer than MIN_ROWS
    assert any(ya & 1 for s in segs.values() for ya, _ in s)
    assert {1, 2, 3} <= {s[-1][1] - s[-1][0] for s in segs.values()}
    assert any(len(s) == 1 and s[0][1] > dc.MIN_ROWS for s in segs.values())
    # the frame / strip split and the list kernel's frame index at large block indices
    assert max(dc.strips(c.w, c.bits) * c.nframes - 1 for c in dc.LONG_CASES) >= 1023
    reach = dc.reaches(dc.WIDE_LONG_CASE)
    assert reach["wave_seam"] and reach["tail"] and not reach["strip_seam"] and dc.reaches(dc.LONG_CASES[0])["tail"]
    assert {c.bits for c in dc.LONG_CASES} == {0, 12, 16} and any(c.sbe for c in dc.LONG_CASES)
    assert len(set(map(dc.case_id, dc.LONG_CASES))) == len(dc.LONG_CASES) and not set(dc.LONG_CASES) & set(dc.CASES)
    # small: under 1 M samples each, but for the wide case
    for c in dc.LONG_CASES:
        assert c.w * c.h * c.nframes <= (5_000_000 if c == dc.WIDE_LONG_CASE else 1_000_000), dc.case_id(c)
    assert sum(c.w * c.h * c.nframes > 1_000_000 for c in dc.LONG_CASES) == 1


@pytest.mark.parametrize("case", dc.LONG_CASES, ids=dc.case_id)
def test_long_frames_can_tell_a_window_that_stops_at_its_segment(case):
    """in the first and the last frame the detection finds exactly the planted samples of a phase, and a model whose
    window is mirrored at the segment's ends (dpc_cases.segment_blind) differs from the model within two rows on each
    side of every interior segment seam"""
    vmax = (1 << (case.bits or 8)) - 1
    segs = dc.segments(case.w, case.h, case.bits, case.nframes)
    where = dc.planted(case.w, case.h, case.bits, case.nframes)
    assert sorted(set(dc.phase_of(where))) == [0, 1, 2, 3]
    for f in (0, case.nframes - 1):
        differs = np.zeros(case.h, bool)
        for phase in range(4):
            S = dc.seam_samples(case, f, phase)
            assert S.min() == 0 and S.max() == vmax and S.shape == (case.h, case.w)
            out = dm.correct(S, vmax // 8, vmax // 8)
            changed = {tuple(c) for c in np.argwhere(out != S)[:, ::-1]}
            assert changed == {tuple(c) for c in where[dc.phase_of(where) == phase]}, (dc.case_id(case), f, phase)
            differs |= (dc.segment_blind(S, segs, vmax // 8, vmax // 8) != out).any(1)
        for ya, _ in segs[1:]:
            assert differs[max(ya - 2, 0):ya].any() and differs[ya:ya + 2].any(), (dc.case_id(case), f, ya)
        # the list for the second launch: every planted position, two workgroups per frame
        lst = dm.sort_defects(dc.long_list(case, np.random.default_rng(f)))
        assert 256 < len(lst) < 512 and {tuple(p) for p in where.tolist()} <= {tuple(p) for p in lst.tolist()}
    assert not np.array_equal(dc.seam_samples(case, 0), dc.seam_samples(case, 1))
    assert not np.array_equal(dc.seam_samples(case, 0), dc.seam_samples(case, 2))
