"""CPU tests of the NumPy model of the mosaic zone statistics (tests/stats_model.py) against a per-pixel loop, and of
the zone geometry."""
import numpy as np
import pytest

import stats_model as sm


@pytest.mark.parametrize("W,H,zx,zy", [(6, 5, 1, 1), (6, 5, 3, 2), (66, 7, 1, 1), (66, 7, 5, 3), (66, 7, 33, 3)])
@pytest.mark.parametrize("lo,hi", [(0, 255), (16, 200), (77, 77), (0, 0)])
def test_model_matches_the_pixel_loop(W, H, zx, zy, lo, hi):
    rng = np.random.default_rng(W * 131 + H * 7 + zx + lo)
    S = rng.integers(0, 256, (H, W)).astype(np.int64)
    S[0, :4] = (lo, hi, min(hi + 1, 255), max(lo - 1, 0))        # the edges of the range are present
    got, want = sm.zone_stats(S, zx, zy, lo, hi), sm.zone_stats_slow(S, zx, zy, lo, hi)
    for f in ("sum", "count", "clipped"):
        assert np.array_equal(got[f], want[f]), f
    # every sample is in exactly one of: counted, clipped, below lo
    assert int(got["count"].sum()) + int(got["clipped"].sum()) + int((S < lo).sum()) == W * H


def test_zone_geometry():
    assert sm.cell(10, 4) == 4 and sm.cell(10, 5) == 2 and sm.cell(10, 1) == 10 and sm.cell(10, 3) == 4
    assert sm.cell(3840, 32) == 120 and sm.cell(2160, 32) == 68 and sm.cell(258, 64) == 6 and sm.cell(130, 64) == 4
    # W = 10 in 4 zones: cells of 4 pixels hold columns 0-3, 4-7, 8-9; the fourth zone is empty and all zero
    S = np.full((4, 10), 9, np.int64)
    z = sm.zone_stats(S, 4, 1, 0, 255)
    assert z["count"].sum(axis=-1).reshape(-1).tolist() == [16, 16, 8, 0]
    assert z["sum"][0, 3].tolist() == [0, 0, 0, 0] and z["clipped"].sum() == 0
    assert z["sum"][0, 2].tolist() == [18, 18, 18, 18]
    # an odd height: H/2 is not rounded down, so the last row has a zone, with sites 0 and 1 only
    z = sm.zone_stats(np.ones((5, 4), np.int64), 1, 2, 0, 255)
    assert sm.cell(5, 2) == 4 and sm.cell(37, 5) == 8 and sm.cell(3, 1) == 4
    assert z["count"][0, 0].tolist() == [4, 4, 4, 4] and z["count"][1, 0].tolist() == [2, 2, 0, 0]


def test_samples_drop_padding_and_high_bits():
    W, H, stride = 6, 3, 16
    raw = np.full(H * stride, 0xFF, np.uint8)
    words = np.arange(H * W, dtype=np.uint16).reshape(H, W) * 37 + 5
    junk = words | 0xF000
    for be in (False, True):
        rows = raw.reshape(H, stride)
        rows[:, :2 * W] = junk.astype(">u2" if be else "<u2").view(np.uint8).reshape(H, 2 * W)
        assert np.array_equal(sm.samples(raw, W, H, stride, 12, be), words & 0xFFF)
    raw8 = np.full(H * 8, 0xFF, np.uint8)
    raw8.reshape(H, 8)[:, :W] = np.arange(H * W).reshape(H, W)
    assert np.array_equal(sm.samples(raw8, W, H, 8), np.arange(H * W).reshape(H, W))


def test_grey_world_model():
    z = np.zeros(2, sm.STATS_DTYPE)
    z["sum"][0], z["count"][0] = (400, 100, 140, 50), (2, 1, 1, 1)       # rggb: R 200, G 120, B 50
    z["sum"][1], z["count"][1] = (0, 120, 120, 50), (0, 1, 1, 1)
    ok, g = sm.grey_world(z, "rggb")
    assert ok == 1 and g == pytest.approx((120.0 / 200.0, 1.0, 120.0 / 50.0), rel=1e-15)
    ok, g = sm.grey_world(z, "bggr")
    assert ok == 1 and g == pytest.approx((120.0 / 50.0, 1.0, 120.0 / 200.0), rel=1e-15)
    assert sm.grey_world(z, "rggb", (0, 0, 50)) == (0, (1.0, 1.0, 1.0))
    assert sm.grey_world(z, "rggb", (10, 10, 49))[1][2] == 15.99
