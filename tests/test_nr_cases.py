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


def test_long_cases_reach_every_segment_length():
    """workgroups of 17 rows, of an even and of an odd number between the clamps, and of 64 rows by three routes"""
    rows = {c: nc.seg_rows(c.w, c.bits, c.nframes, 0, c.h) for c in nc.LONG_CASES}
    segs = {c: nc.segments(c.w, c.h, c.bits, c.nframes) for c in nc.LONG_CASES}
    assert [rows[c] for c in nc.LONG_CASES] == [17, 17, 26, 25, 43, 64, 64, 64, 17]
    assert set(rows.values()) == {17, 25, 26, 43, 64}
    assert any(18 <= r <= 62 and r % 2 == 0 and c.h % r == 0 for c, r in rows.items())
    assert any(19 <= r <= 63 and r % 2 == 1 for r in rows.values())
    # 64 as the rule gives it; clamped, with a short last segment; clamped, three segments
    at_max = {c: (nc.unclamped_rows(c), len(segs[c])) for c, r in rows.items() if r == nc.MAX_ROWS}
    assert at_max == {nc.Case(10, 64, 0, False, 1024): (64, 1), nc.Case(6, 67, 12, False, 1000): (65, 2),
                      nc.Case(14, 131, 0, False, 512): (65, 3)}
    assert segs[nc.Case(6, 67, 12, False, 1000)] == [(0, 64), (64, 67)]
    assert segs[nc.Case(14, 131, 0, False, 512)] == [(0, 64), (64, 128), (128, 131)]
    assert segs[nc.Case(10, 35, 0, False, 512)] == [(0, 17), (17, 34), (34, 35)] == segs[nc.WIDE_LONG_CASE]
    assert segs[nc.Case(6, 70, 0, False, 256)] == [(0, 17), (17, 34), (34, 51), (51, 68), (68, 70)]
    assert segs[nc.Case(10, 52, 0, False, 512)] == [(0, 26), (26, 52)]
    assert segs[nc.Case(8, 33, 16, True, 800)] == [(0, 25), (25, 33)]
    assert segs[nc.Case(10, 45, 0, False, 1000)] == [(0, 43), (43, 45)]
    # odd segment starts, last segments of 1, 2 and 3 rows (the clamp at the segment's end and the reflection at the
    # frame's bottom in one window), one segment longer than MIN_ROWS
    assert any(ya & 1 for s in segs.values() for ya, _ in s)
    assert {1, 2, 3} <= {s[-1][1] - s[-1][0] for s in segs.values()}
    assert any(len(s) == 1 and s[0][1] > nc.MIN_ROWS for s in segs.values())
    # the frame / strip split at large block indices
    assert max(nc.strips(c.w, c.bits) * c.nframes - 1 for c in nc.LONG_CASES) >= 1023
    reach = nc.reaches(nc.WIDE_LONG_CASE)
    assert reach["wave_seam"] and reach["tail"] and not reach["strip_seam"] and nc.reaches(nc.LONG_CASES[0])["tail"]
    assert {nc.depth(c) for c in nc.LONG_CASES} == {8, 12, 16} and any(c.sbe for c in nc.LONG_CASES)
    assert len(set(map(nc.case_id, nc.LONG_CASES))) == len(nc.LONG_CASES) and not set(nc.LONG_CASES) & set(nc.CASES)
    # small: under 1 M samples each, but for the wide case
    for c in nc.LONG_CASES:
        assert c.w * c.h * c.nframes <= (5_000_000 if c == nc.WIDE_LONG_CASE else 1_000_000), nc.case_id(c)
    assert sum(c.w * c.h * c.nframes > 1_000_000 for c in nc.LONG_CASES) == 1


@pytest.mark.parametrize("case", nc.LONG_CASES, ids=nc.case_id)
def test_long_frames_can_tell_a_window_that_stops_at_its_segment(case):
    """in the first and the last frame about half of the neighbours are included, and a model whose window is reflected
    at the segment's ends (nr_cases.segment_blind) differs from the model within four rows on each side of every interior
    segment seam"""
    d = nc.depth(case)
    curve = nc.curve_of(case)
    segs = nc.segments(case.w, case.h, case.bits, case.nframes)
    rows, cols = nc.seam_rows(case.w, case.h, case.bits, case.nframes), nc.seam_columns(case.w, case.bits)
    assert all(set(range(ya - nc.REACH, ya + nc.REACH)) & set(range(case.h)) <= set(rows) for ya, _ in segs[1:])
    for f in (0, case.nframes - 1):
        S = nc.seam_samples(case, f)
        assert S.min() >= 0 and S.max() < 1 << d
        share = nm.included(S, curve, d)[np.ix_(range(24), rows, cols)].mean()
        assert 0.3 <= share <= 0.7, share
        out = nm.denoise(S, curve, d)
        assert (out != S).any(1)[rows].all()
        differs = (nc.segment_blind(S, segs, curve, d) != out).any(1)
        for ya, _ in segs[1:]:
            assert differs[max(ya - nc.REACH, 0):ya].any() and differs[ya:ya + nc.REACH].any(), (nc.case_id(case), f, ya)
    assert not np.array_equal(nc.seam_samples(case, 0), nc.seam_samples(case, 1))


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
