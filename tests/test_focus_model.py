"""CPU tests of the NumPy model of the mosaic focus statistics (tests/focus_model.py) against itself and against the
closed forms of the definition (include/mibayer.h, group `focus`)."""
import numpy as np
import pytest

import focus_model as fm

SHAPES = [(4, 3), (4, 4), (6, 5), (10, 6), (18, 7), (22, 18), (34, 13)]


def same(got, want):
    for f in ("h", "v", "nh", "nv"):
        assert np.array_equal(got[f], want[f]), f


@pytest.mark.parametrize("W,H", SHAPES)
def test_the_two_models_agree(W, H):
    rng = np.random.default_rng(W * 100 + H)
    for vmax in (255, 4095, 65535):
        S = rng.integers(0, vmax + 1, (H, W))
        for zx, zy in ((1, 1), (min(3, W // 2), min(5, H // 2)), (W // 2, H // 2)):
            for thr in (0, vmax // 4, 2 * vmax):
                same(fm.zone_focus(S, zx, zy, thr, vmax), fm.zone_focus_slow(S, zx, zy, thr, vmax))


@pytest.mark.parametrize("W,H", SHAPES + [(258, 37), (266, 70)])
def test_counts_at_threshold_zero_have_a_closed_form(W, H):
    S = np.random.default_rng(W + H).integers(0, 256, (H, W))
    for zx, zy in ((1, 1), (min(3, W // 2), min(5, H // 2))):
        z = fm.zone_focus(S, zx, zy, 0, 255)
        for s in range(4):
            rows = len(range(s >> 1, H, 2))
            rows_v = len([y for y in range(s >> 1, H, 2) if 2 <= y <= H - 3])
            assert int(z["nh"][..., s].sum()) == rows * ((W - 4) // 2)
            assert int(z["nv"][..., s].sum()) == (W // 2) * rows_v
        nh, nv = fm.counts_at_zero(W, H)
        assert z["nh"].reshape(-1, 4).sum(0).tolist() == nh and z["nv"].reshape(-1, 4).sum(0).tolist() == nv
    if W == 4:
        assert not z["nh"].any() and not z["h"].any()
    if H in (3, 4):
        assert not z["nv"].any() and not z["v"].any()


def test_a_constant_frame_has_zero_sums_and_full_counts():
    W, H = 22, 13
    z = fm.zone_focus(np.full((H, W), 77), 3, 2, 0, 255)
    assert not z["h"].any() and not z["v"].any()
    nh, nv = fm.counts_at_zero(W, H)
    assert z["nh"].reshape(-1, 4).sum(0).tolist() == nh and z["nv"].reshape(-1, 4).sum(0).tolist() == nv
    # ... and with any threshold above zero nothing contributes
    z = fm.zone_focus(np.full((H, W), 77), 3, 2, 1, 255)
    assert not z["nh"].any() and not z["nv"].any()


@pytest.mark.parametrize("vmax", (255, 1023, 65535))
def test_alternating_extremes_give_twice_max_everywhere(vmax):
    W, H = 18, 11
    y, x = np.mgrid[0:H, 0:W]
    S = (((x >> 1) + (y >> 1)) & 1) * vmax              # 0 / max at same-site distance, in both directions
    z = fm.zone_focus(S, 3, 2, 2 * vmax, vmax)
    nh, nv = fm.counts_at_zero(W, H)
    assert z["nh"].reshape(-1, 4).sum(0).tolist() == nh and z["nv"].reshape(-1, 4).sum(0).tolist() == nv
    assert np.array_equal(z["h"], z["nh"].astype(np.uint64) * np.uint64(2 * vmax))
    assert np.array_equal(z["v"], z["nv"].astype(np.uint64) * np.uint64(2 * vmax))


def test_a_sample_belongs_to_the_zone_of_its_own_position():
    """one bright sample: its own response lands in its zone, its neighbours' responses in theirs"""
    W, H = 16, 12
    S = np.zeros((H, W), np.int64)
    S[5, 8] = 100                                       # site 2 (odd row, even column); zones of 8 x 6 pixels
    z = fm.zone_focus(S, 2, 2, 1, 255)
    assert fm.cell(W, 2) == 8 and fm.cell(H, 2) == 6
    assert z["h"][0, 1, 2] == 200 + 100 and z["h"][0, 0, 2] == 100     # x = 8 and 10 right of the seam, x = 6 left
    assert z["v"][0, 1, 2] == 200 + 100 and z["v"][1, 1, 2] == 100     # y = 5 and 3 above the seam, y = 7 below
    assert z["h"].sum() == 400 and z["v"].sum() == 400


def test_bad_arguments_are_rejected():
    S = np.zeros((6, 10), np.int64)
    with pytest.raises(ValueError):
        fm.zone_focus(S, 1, 1, 2 * 255 + 1, 255)
    with pytest.raises(ValueError):
        fm.zone_focus(S, 1, 1, -1, 255)
    with pytest.raises(ValueError):
        fm.zone_focus(S, 6, 1, 0, 255)
    with pytest.raises(ValueError):
        fm.zone_focus(S, 1, 4, 0, 255)
    fm.zone_focus(S, 5, 3, 2 * 255, 255)


def test_score():
    z = np.zeros(2, fm.FOCUS_DTYPE)
    assert fm.score(z, "rggb") == (0, 0.0)
    z["h"][0] = (10, 20, 30, 40)
    z["nh"][0] = (1, 2, 3, 4)
    z["v"][1] = (1, 1, 1, 1)
    z["nv"][1] = (1, 1, 1, 1)
    assert fm.score(z, "rggb", 0) == (1, 11.0 / 2.0)            # R = site 0
    assert fm.score(z, "rggb", 1) == (1, 52.0 / 7.0)            # G = sites 1 and 2
    assert fm.score(z, "bggr", 0) == (1, 41.0 / 5.0)            # R = site 3
    assert fm.score(z, "rggb", 3) == (1, 104.0 / 14.0)
    assert fm.score(z, "rggb", 3, (1.0, 0.0)) == (1, 10.0)
    assert fm.score(z, "rggb", 3, (0.0, 0.0)) == (0, 0.0)
    with pytest.raises(ValueError):
        fm.score(z, "rggb", 3, (1.0, -1.0))
    with pytest.raises(ValueError):
        fm.score(z, "rggb", 3, (1.0, float("nan")))
