"""CPU tests of the noise reduction kernel's case table (tests/nr_cases.py): what the shapes reach, and -- from the
model alone -- that the frames exercise the filter on every seam of the kernel's geometry."""
import numpy as np
import pytest

import band_cases as bc
import nr_cases as nc
import nr_model as nm


def test_the_table_reaches_every_path_of_the_geometry():
    r = {c: nc.reaches(c) for c in nc.CASES}
    for deep in (False, True):
        rs = [v for c, v in r.items() if bool(c.bits) == deep]
        assert any(v["wave_seam"] for v in rs) and any(v["strip_seam"] for v in rs)
        assert any(v["segments"] >= 3 and v["short_last_segment"] for v in rs)
        assert any(v["segments"] == 1 for v in rs)
        assert any(v["odd_height"] for v in rs) and any(not v["odd_height"] for v in rs)
        assert any(v["batch"] for v in rs) and any(v["reflections_overlap"] for v in rs)
        assert {(6, 5), (6, 6)} <= {(c.w, c.h) for c in r if bool(c.bits) == deep}
    assert any(v["tail"] and v["strip_seam"] for v in r.values()) and any(not v["tail"] and v["strip_seam"] for c, v in r.items() if not c.bits)
    # a tail in the smallest frame (one whole dword and half a one) and a last whole dword behind a single one
    assert nc.has_tail(6, 0) and nc.row_dwords(6, 0) == 2 and nc.row_dwords(8, 0) == 2 and nc.row_dwords(6, 16) == 3
    assert {nc.depth(c) for c in nc.CASES} == {8, 10, 12, 14, 16}
    assert {c.sbe for c in nc.CASES if c.bits} == {False, True}
    # widths just past the strip: 1024 px of an 8-bit row, 512 px of a deep one
    assert nc.column_seams(1030, 0)["strip"] == [1024] and nc.column_seams(518, 12)["strip"] == [512]
    assert nc.column_seams(1030, 0)["wave"] == [256, 512, 768] and nc.column_seams(518, 12)["wave"] == [128, 256, 384]
    assert nc.segments(1030, 37, 0) == [(0, 16), (16, 32), (32, 37)]
    # rows of a launch that begins and ends inside the frame, as the banded host path makes them
    assert nc.segments(266, 116, 0, 1, 17, 59) == [(17, 33), (33, 49), (49, 59)]
    assert len(set(map(nc.case_id, nc.CASES))) == len(nc.CASES)


def test_the_row_cuts_of_the_host_path():
    """a band denoises up to the last row its demosaic reads: the cuts of 116 rows in 1 .. 8 bands of 16-row units"""
    assert nc.row_cuts(bc.band_rows(1, 116, 16), 116, 1) == []
    assert nc.row_cuts(bc.band_rows(2, 116, 16), 116, 1) == [65]
    assert nc.row_cuts(bc.band_rows(4, 116, 16), 116, 2) == [34, 66, 98]
    for nb in range(1, 9):
        for unit in (8, 16):
            cuts = nc.row_cuts(bc.band_rows(nb, 116, unit), 116, 1)
            assert cuts == sorted(set(cuts)) and all(0 < y < 116 for y in cuts)


@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_id)
def test_the_frames_exercise_the_filter_on_every_seam(case):
    d = nc.depth(case)
    curve = nc.curve_of(case)
    t = curve[0]
    assert t <= nm.t_max(d) and abs(3 * t - 2 * nc.NOISE[d][0]) <= nc.NOISE[d][0] // 4         # about 2 A / 3
    cols = nc.seam_columns(case.w, case.bits)
    rows = nc.seam_rows(case.w, case.h, case.bits, case.nframes)
    shares, at_t, past_t = [], 0, 0
    changed_cols, changed_rows = np.zeros(case.w, bool), np.zeros(case.h, bool)
    for f in range(case.nframes):
        S = nc.seam_samples(case, f)
        assert S.min() >= 0 and S.max() < 1 << d
        diff = np.abs(nm.neighbours(S) - S)
        inc = nm.included(S, curve, d)
        assert np.array_equal(inc, diff <= t)
        cross = np.ix_(range(24), rows, cols)
        shares.append(inc[cross].mean())
        at_t += int((diff == t).sum())
        past_t += int((diff == t + 1).sum())
        changed = nm.denoise(S, curve, d) != S
        changed_cols |= changed.any(0)
        changed_rows |= changed.any(1)
    share = float(np.mean(shares))
    print("%s: mean share of included neighbours at seam crossings %.3f" % (nc.case_id(case), share))
    assert 0.3 <= share <= 0.7, share
    assert at_t > 0 and past_t > 0
    assert changed_cols[cols].all() and changed_rows[rows].all()


@pytest.mark.parametrize("case", [c for c in nc.CASES if c.w >= 10 and c.h >= 7][:6], ids=nc.case_id)
def test_the_planted_boundary(case):
    d = nc.depth(case)
    curve = nc.curve_of(case)
    t = curve[0]
    for at_max in (False, True):
        S, centres = nc.boundary_samples(case, at_max)
        assert centres and S.min() >= 0 and S.max() < 1 << d
        inc = nm.included(S, curve, d)
        out = nm.denoise(S, curve, d)
        right, left = nm.OFFSETS.index((2, 0)), nm.OFFSETS.index((-2, 0))
        up, down = nm.OFFSETS.index((0, -2)), nm.OFFSETS.index((0, 2))
        for x, y in centres:
            assert inc[right, y, x] and not inc[left, y, x] and inc[up, y, x] and not inc[down, y, x]
            # the included ones lie t away (a centre near the border sees them twice), the rest is the centre's level
            cnt = 1 + int(inc[:, y, x].sum())
            far = int((inc[:, y, x] & (nm.neighbours(S)[:, y, x] != S[y, x])).sum())
            q = (2 * far * t + cnt) // (2 * cnt)
            assert far >= 2 and q > 0 and out[y, x] == S[y, x] + (-q if at_max else q)
