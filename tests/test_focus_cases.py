"""The case table of tests/focus_cases.py reaches what it is meant to reach -- asserted from the table, the mirror of the
launch geometry and the model (tests/focus_model.py) alone, so that the GPU test built on it
(tests/test_gpu_focus.py::test_case_table) cannot go vacuous when the table is edited."""
import numpy as np

import focus_cases as fc
import focus_model as fm
import stats_model as sm


def contributing(case):
    """(H, W) booleans: the samples whose rh / rv is defined and reaches the case's threshold; and the responses"""
    S = fc.samples(case, fc.frame(case))
    rh, dh, rv, dv = fm.responses(S)
    thr = fc.threshold(case)
    return dh & (rh >= thr), dv & (rv >= thr), (rh, dh, rv, dv)


def test_mirror_is_the_models_grid_and_the_table_names_every_kind_of_seam():
    kinds = {}
    for case in fc.CASES:
        geo = fc.geometry(case)
        assert geo.ch == sm.cell(case.H, case.zones_y) and geo.cw == sm.cell(case.W, case.zones_x)
        assert case.zones_x <= case.W // 2 and case.zones_y <= case.H // 2
        for kind, at in list(fc.column_seams(case).items()) + list(fc.row_seams(case).items()):
            if at:
                kinds.setdefault(kind, []).append(case)
    assert set(kinds) == {"lane", "wave", "strip", "zone-x", "segment", "zone-y"}
    for kind in kinds:      # each in an 8-bit and in a deep case
        assert {bool(c.bits) for c in kinds[kind]} == {False, True}, kind
    # the named geometries: a segment seam inside a zone row, two zone rows of two segments, the 8-bit tail, both orders
    assert fc.row_seams(fc.Case(266, 70, 0, False, 3, 1)) == {"segment": [64], "zone-y": []}
    assert fc.row_seams(fc.Case(1026, 133, 0, False, 3, 2)) == {"segment": [64, 132], "zone-y": [68]}
    assert {c.W % 4 for c in fc.CASES if not c.bits} == {0, 2}
    assert {c.big_endian for c in fc.CASES if c.bits} == {False, True}
    assert {c.bits for c in fc.CASES} >= {0, 10, 12, 16}
    assert any(c.zones_x == 64 and c.zones_y == 64 for c in fc.CASES)


def test_a_contributing_sample_reaches_across_every_seam():
    """across every seam some contributing sample has its neighbour on the other side -- from both sides wherever both
    sides have defined responses"""
    for case in fc.CASES:
        ch, cv, _ = contributing(case)
        W, H = case.W, case.H
        for kind, at in fc.column_seams(case).items():
            for x in at:
                left, right = ch[:, max(x - 2, 0):x].any(), ch[:, x:x + 2].any()   # their x + 2 / x - 2 is across
                assert left or right, (case, kind, x)
                if 4 <= x <= W - 4:
                    assert left and right, (case, kind, x)
        for kind, at in fc.row_seams(case).items():
            for y in at:
                above, below = cv[max(y - 2, 0):y].any(), cv[y:y + 2].any()
                if case in fc.EXEMPT_V:
                    continue
                assert above or below, (case, kind, y)
                if 4 <= y <= H - 4:
                    assert above and below, (case, kind, y)


def test_both_sides_of_the_threshold_in_every_case_and_the_threshold_itself_in_the_table():
    at_thr = below_thr = 0
    for case in fc.CASES:
        _, _, (rh, dh, rv, dv) = contributing(case)
        thr = fc.threshold(case)
        assert 0 < thr <= 2 * fc.vmax_of(case)
        for r, d, exempt in ((rh, dh, fc.EXEMPT_H), (rv, dv, fc.EXEMPT_V)):
            if case in exempt:
                assert not d.any()
                continue
            assert (r[d] >= thr).any() and (r[d] < thr).any(), case
            at_thr += int((r[d] == thr).sum())
            below_thr += int((r[d] == thr - 1).sum())
    assert at_thr > 0 and below_thr > 0
    # exempt are the two kinds the definition names, and nothing else
    assert all(c.W == 4 for c in fc.EXEMPT_H) and all(c.H in (3, 4) for c in fc.EXEMPT_V)
    assert fc.EXEMPT_H and fc.EXEMPT_V and len(fc.EXEMPT_H) + len(fc.EXEMPT_V) < len(fc.CASES) // 2


def test_planted_responses_and_junk():
    """|rh| = thr at x = 2 and thr - 1 at x = 3 of the middle row of every case wide enough; junk above `bits` and 0xFF in
    the padding of every frame that has either"""
    for case in fc.CASES:
        raw = fc.frame(case)
        S = fc.samples(case, raw)
        assert S.max() <= fc.vmax_of(case)
        if case.W >= 8:
            rh = fm.responses(S)[0]
            assert rh[case.H // 2, 2] == fc.threshold(case) and rh[case.H // 2, 3] == fc.threshold(case) - 1, case
        if case.bits and case.bits < 16:
            words = raw.view(">u2" if case.big_endian else "<u2")
            assert (words >> case.bits).any(), case
        if not case.bits and case.W % 4:
            assert (raw[:, case.W:] == 0xFF).all()


def test_the_models_agree_on_the_small_cases():
    for case in fc.CASES:
        if case.W * case.H > 5000:
            continue
        S = fc.samples(case, fc.frame(case))
        for thr in (0, fc.threshold(case)):
            a = fm.zone_focus(S, case.zones_x, case.zones_y, thr, fc.vmax_of(case))
            b = fm.zone_focus_slow(S, case.zones_x, case.zones_y, thr, fc.vmax_of(case))
            assert a.tobytes() == b.tobytes(), (case, thr)
        assert np.array_equal(fc.expected(case, fc.frame(case))["nh"], fm.zone_focus(
            S, case.zones_x, case.zones_y, fc.threshold(case), fc.vmax_of(case))["nh"])
