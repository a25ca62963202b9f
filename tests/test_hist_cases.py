"""The case tables of tests/hist_cases.py reach what they are meant to reach -- asserted from the tables, the mirror of
the kernel's lane states and launch geometry and the model (tests/hist_model.py) alone, so that the GPU tests built on
them (tests/test_gpu_hist_geometry.py) cannot go vacuous when a table is edited."""
import itertools

import numpy as np
import pytest

import hist_cases as tc
import hist_model as hm

LANE_STATES = ((True, True), (True, False), (False, True))      # (in0, in1): a lane with neither is never started
EQUALITIES = {"ee": (True, True), "en": (True, False), "ne": (False, True), "nn": (False, False)}


def test_fusion_families_hold_their_equalities_in_every_dword_and_past_the_row():
    for family, (e02, e13) in EQUALITIES.items():
        raw = tc.fusion_frame(family, tc.FUSION_PAD_STRIDE, 5)
        d = raw.reshape(5, -1, 4)
        assert ((d[..., 0] == d[..., 2]) == e02).all() and ((d[..., 1] == d[..., 3]) == e13).all()
        # the four sites stay apart: no value of one site occurs at another
        sites = [set(raw[s >> 1::2, s & 1::2].reshape(-1).tolist()) for s in range(4)]
        assert all(not (sites[a] & sites[b]) for a in range(4) for b in range(a)), family
        # nothing marks the end of a 258-wide row: the padding continues the pattern
        assert np.array_equal(raw[:, 258:262], raw[:, 2:6])


def test_all_twelve_fusion_tuples_occur_and_which_case_supplies_each():
    """three lane states x four equality states; the two arms nothing reached by construction before are
    in0 && !in1 and !in0 && in1 with an excluded pair that EQUALS its included neighbour"""
    cases = tc.fusion_cases()
    supplied = {}
    for family in tc.FAMILIES:
        for c in cases:
            raw = tc.fusion_frame(family, c.stride, c.H)
            for t in tc.lane_tuples(raw, c.W, c.H, c.win):
                assert (t[2], t[3]) == EQUALITIES[family]
                supplied.setdefault(t, set()).add((family, c.name))
    want = {s + e for s, e in itertools.product(LANE_STATES, EQUALITIES.values())}
    assert set(supplied) == want and len(want) == 12
    names = {t: {n for _, n in v} for t, v in supplied.items()}
    for e in EQUALITIES.values():
        assert names[(True, True) + e] >= {"both", "whole", "in1-first-both-last"}
        assert names[(True, False) + e] >= {"whole", "in0-pair", "inner-in0-last", "padded-stride",
                                           "in1-first-in0-last"}
        assert names[(False, True) + e] >= {"in1-pair", "in1-first-in0-last", "in1-first-both-last",
                                           "inner-in1-first-in0-last"}
        assert "both" not in names[(True, False) + e] | names[(False, True) + e]
    # a 2-column window is one lane state alone
    for c in cases:
        states = {t[:2] for t in tc.lane_tuples(tc.fusion_frame("nn", c.stride, c.H), c.W, c.H, c.win)}
        if c.name in ("in0-pair", "in1-pair"):
            assert c.win[2] == 2 and states == {(c.name == "in0-pair", c.name == "in1-pair")}
        if c.name == "both":
            assert states == {(True, True)}


def test_fusion_tail_dword_sits_in_lane_1_behind_a_wave_and_behind_a_strip():
    assert all(W % 4 == 2 for W in tc.FUSION_WIDTHS)
    where = {c.W: tc.tail_dword_lane(c.W, c.H, c.win) for c in tc.fusion_cases() if c.name == "whole"}
    assert where == {6: (0, 0, 1), 258: (0, 1, 0), 1030: (1, 0, 1)}
    inner = {c.win[2]: tc.tail_dword_lane(c.W, c.H, c.win) for c in tc.fusion_cases() if c.name == "inner-in0-last"}
    assert inner == {258: (0, 1, 0), 1030: (1, 0, 1)}
    assert {c.H for c in tc.fusion_cases()} == {5, 17} and {c.win[1] for c in tc.fusion_cases()} == {0, 1}
    assert any(c.stride > ((c.W + 3) & ~3) for c in tc.fusion_cases())


def test_fusion_expectations_are_the_pixel_loop_and_the_window_sizes():
    for family in tc.FAMILIES:
        for c in tc.fusion_cases():
            if c.H != 5 or c.W == 1030:
                continue
            S = tc.samples(tc.fusion_frame(family, c.stride, c.H), c.W, c.H)
            fast = hm.histogram(S, 8, c.win)
            assert np.array_equal(fast, hm.histogram_slow(S, 8, c.win))
            assert fast.sum(axis=1).tolist() == tc.window_counts(c.W, c.H, c.win)


def test_window_counts_from_the_window_alone():
    assert tc.window_counts(6, 5, (0, 0, 0, 0)) == [9, 9, 6, 6]
    assert tc.window_counts(1030, 35, (2, 1, 1026, 33)) == [513 * 16, 513 * 16, 513 * 17, 513 * 17]
    assert tc.window_counts(8, 4, (2, 1, 2, 1)) == [0, 0, 1, 1]


@pytest.mark.parametrize("bits", (8,) + tc.DEEP_BITS)
def test_value_frames_fill_every_bin_of_every_site_with_256(bits):
    W, H = tc.VALUE_SIZE
    for big_endian in ((False,) if bits == 8 else (False, True)):
        raw = tc.value_frame(bits, big_endian)
        assert raw.nbytes == W * H * (1 if bits == 8 else 2) <= 512 * 1024
        S = tc.samples(raw, W, H, 0 if bits == 8 else bits, big_endian)
        for s in range(4):
            plane = S[s >> 1::2, s & 1::2]
            assert np.array_equal(np.bincount(plane.reshape(-1)), np.full(1 << bits, 1 << (16 - bits)))
        assert (hm.histogram(S, bits) == tc.VALUE_BIN).all()
        if bits not in (8, 16):         # junk above `bits` is there, and is not constant
            junk = raw.view(">u2" if big_endian else "<u2") >> bits
            assert len(np.unique(junk)) == 1 << (16 - bits)


@pytest.mark.parametrize("bits", tc.DEEP_BITS)
def test_edge_frames_sit_on_both_sides_of_every_bin_boundary_and_at_the_extremes(bits):
    W, H = tc.EDGE_SIZE
    shift, vmax = bits - 8, (1 << bits) - 1
    vals = tc.boundary_values(bits)
    assert len(vals) == (510 if shift else 256) and vals[0] == (1 << shift) - 1 and vals[-1] == 255 << shift
    for big_endian in (False, True):
        S = tc.samples(tc.boundary_frame(bits, big_endian), W, H, bits, big_endian)
        assert sorted(set(S.reshape(-1).tolist())) == vals
        h = hm.histogram(S, bits)
        assert int(h.sum()) == W * H and (h.sum(axis=0) > 0).all()
        raw = tc.extremes_frame(bits, big_endian)
        assert (raw.view(">u2" if big_endian else "<u2") | vmax == 0xFFFF).all()       # all-ones junk
        S = tc.samples(raw, W, H, bits, big_endian)
        h = hm.histogram(S, bits)
        assert set(S.reshape(-1).tolist()) == {0, vmax} and (h[:, 1:255] == 0).all()
        assert (h[:, 0] > 0).all() and (h[:, 255] > 0).all() and len({tuple(r) for r in h.tolist()}) == 4


def test_split_cases_cross_frames_strips_segments_and_an_odd_window_origin():
    for case in tc.SPLIT_CASES:
        padded, raws = tc.split_frames(case)
        win, whole = tc.SPLIT_WINDOWS[case.W]
        assert whole == (0, 0, 0, 0) and case.frames == 3
        x0, y0, x1, y1 = tc.resolved(case.W, case.H, win)
        assert y0 % 2 == 1 and x0 == 2 and (case.bits or (x0 % 4, x1 % 4) == (2, 0))
        # strips != frames: a transposed split cannot land on the right tables
        assert tc.strips(case.W, case.H, win, case.bits) == tc.strips(case.W, case.H, whole, case.bits) == 2
        rows = tc.rows_per_workgroup(case.H, 2, case.frames)
        assert rows == 16 and tc.segments(case.H, rows) == [16, 16, 3] and tc.segments(y1 - y0, rows) == [16, 16, 1]
        # padded rows, junk between the frames, a batch that can start at 4 mod 16
        assert case.stride > (2 * case.W if case.bits else case.W) and case.stride % 4 == 0
        assert padded.shape == (3, case.stride * case.H + case.extra) and padded.shape[1] % 4 == 0
        assert (padded[:, -case.extra:] == tc.SPLIT_GAP).all() and tc.SPLIT_OFFSET % 16 == 4
        assert all((r[:, -4:] == tc.SPLIT_PAD).all() for r in raws)
        # every frame's table differs from the others', under both windows
        for w in (win, whole):
            tables = [hm.histogram(tc.samples(r, case.W, case.H, case.bits, case.big_endian), tc.depth(case.bits), w)
                      for r in raws]
            assert len({t.tobytes() for t in tables}) == 3
            assert all(t.sum(axis=1).tolist() == tc.window_counts(case.W, case.H, w) for t in tables)
    assert [(c.bits, c.big_endian) for c in tc.SPLIT_CASES] == [(0, False), (12, True)]


def test_rows_cases_land_on_the_rows_per_workgroup_they_name():
    seen = set()
    for (W, H, frames), (rows, segs) in tc.ROWS_CASES.items():
        nstrips = tc.strips(W, H, (0, 0, 0, 0))
        assert nstrips == (2 if W == 1028 else 1)
        assert tc.rows_per_workgroup(H, nstrips, frames) == rows and tc.segments(H, rows) == segs
        assert W * H * frames <= 2_500_000 or (W, H, frames) == (1028, 40, 128)  # (that one: 5.3 MB, as asked for)
        seen.add(rows)
    # the minimum is A3's; here: between the clamps (even as it comes, and rounded up from odd), and the cap
    assert seen == {40, 22, 256, 20} and tc.rows_per_workgroup(21, 1, 512) == 21 + 1
    assert tc.rows_per_workgroup(1, 1, 1) == tc.MIN_ROWS and tc.rows_per_workgroup(10 ** 6, 8, 16) == tc.MAX_ROWS
    # the two cases of tests/test_gpu_hist.py, as their docstrings state them
    assert tc.rows_per_workgroup(2100, 5, 1) == 20 and tc.rows_per_workgroup(1030, 8, 16) == 256


def test_rows_frames_differ_from_their_neighbours_and_the_batch_model_is_the_model():
    for (W, H, frames) in tc.ROWS_CASES:
        raws = tc.rows_frames(W, H, frames)
        want = tc.histograms(raws)
        assert want.shape == (frames, 4, 256) and want.dtype == np.uint32
        assert all(not np.array_equal(want[f], want[f + 1]) for f in range(frames - 1))
        for f in (0, 1, frames - 1):
            assert np.array_equal(want[f], hm.histogram(raws[f].astype(np.int64), 8))
        assert (want.sum(axis=2) == np.asarray(tc.window_counts(W, H, (0, 0, 0, 0)))).all()


def test_repeat_and_host_cases_are_fusion_cases():
    family, c = tc.REPEAT_CASE
    assert family == "ee" and (True, True, True, True) in tc.lane_tuples(tc.fusion_frame(family, c.stride, c.H), c.W,
                                                                           c.H, c.win)
    family, c = tc.HOST_CASE
    assert c.win[0] % 4 == 2 and c.stride == (c.W + 3) & ~3
    got = tc.lane_tuples(tc.fusion_frame(family, c.stride, c.H), c.W, c.H, c.win)
    assert got == {(False, True, True, False), (True, True, True, False), (True, False, True, False)}
