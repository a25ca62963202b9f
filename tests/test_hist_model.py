"""CPU tests of the NumPy histogram model itself: the fast form against its pixel-by-pixel twin, both pinned to the
zone-statistics model that the suite already trusts, and the window rules."""
import numpy as np
import pytest

import hist_model as hm
import stats_model as sm


def frame(rng, W, H, depth):
    return rng.integers(0, 1 << depth, (H, W)).astype(np.int64)


@pytest.mark.parametrize("W,H,depth", [(2, 1, 8), (4, 3, 8), (6, 5, 10), (10, 4, 12), (18, 7, 16), (32, 9, 8)])
def test_fast_matches_slow(W, H, depth):
    rng = np.random.default_rng(W * 100 + H)
    S = frame(rng, W, H, depth)
    wins = [(0, 0, 0, 0), (0, 0, 2, 1), (W - 2, H - 1, 2, 1), (0, H - 1, W, 1)]
    if W >= 6 and H >= 3:
        wins += [(2, 1, 4, 2), (2, 0, W - 2, H), (0, 1, W, H - 1), (W - 4, H - 2, 2, 2)]
    for win in wins:
        got = hm.histogram(S, depth, win)
        assert got.dtype == np.uint32 and got.shape == (4, 256)
        assert np.array_equal(got, hm.histogram_slow(S, depth, win)), win
        x0, y0, w, h = hm.window(W, H, win)
        assert int(got.sum()) == w * h


@pytest.mark.parametrize("W,H,depth", [(8, 6, 8), (14, 9, 8), (12, 5, 12), (6, 4, 16)])
def test_pinned_to_the_zone_statistics_model(W, H, depth):
    """per site, the bins add up to the count of a one-zone grid over the full range -- and, where a bin is a value,
    bin-weighted to its sum"""
    rng = np.random.default_rng(W + H + depth)
    S = frame(rng, W, H, depth)
    hist = hm.histogram(S, depth)
    zone = sm.zone_stats(S, 1, 1, 0, (1 << depth) - 1)[0, 0]
    for s in range(4):
        assert int(hist[s].sum()) == int(zone["count"][s])
        if depth == 8:
            assert sum(b * int(hist[s, b]) for b in range(256)) == int(zone["sum"][s])


def test_site_is_in_frame_coordinates():
    """an odd y0 or x0 = 2 (mod 4) does not renumber the sites"""
    S = np.zeros((6, 8), np.int64)
    for s in range(4):
        S[s >> 1::2, s & 1::2] = 10 + 50 * s
    hist = hm.histogram(S, 8, (2, 1, 4, 3))    # rows 1, 2, 3: one even row, two odd ones
    assert [int(hist[s, 10 + 50 * s]) for s in range(4)] == [2, 2, 4, 4]
    assert int(hist.sum()) == 12


def test_deep_bins_drop_the_low_bits():
    S = np.array([[0, 3, 4, 1023], [512, 515, 516, 1020]], np.int64)
    hist = hm.histogram(S, 10)
    assert hist[0, 0] == 1 and hist[0, 1] == 1 and hist[1, 0] == 1 and hist[1, 255] == 1
    assert hist[2, 128] == 1 and hist[2, 129] == 1 and hist[3, 128] == 1 and hist[3, 255] == 1


@pytest.mark.parametrize("win", [(1, 0, 2, 1), (0, 0, 3, 1), (0, 0, 0, 1), (0, 0, 2, 0), (-2, 0, 2, 1), (0, -1, 2, 1),
                                 (10, 0, 2, 1), (0, 6, 2, 1), (4, 0, 8, 1), (0, 1, 2, 6), (0, 0, 10, 0)])
def test_window_rules(win):
    with pytest.raises(ValueError):
        hm.window(10, 6, win)


def test_whole_frame_window_includes_an_odd_last_row():
    assert hm.window(10, 7) == (0, 0, 10, 7) and hm.window(10, 7, (4, 6, 6, 1)) == (4, 6, 6, 1)


def test_percentile_and_exposure_by_hand():
    hist = np.zeros((4, 256), np.uint32)
    hist[0, 10], hist[0, 20] = 99, 1            # rggb: R
    hist[1, 30], hist[2, 40] = 50, 50           # G, pooled over both sites
    hist[3, 100] = 7                            # B
    assert hm.percentile_bin(hist, "rggb", 0, 0.99) == (1, 10) and hm.percentile_bin(hist, "rggb", 0, 0.991) == (1, 20)
    assert hm.percentile_bin(hist, "rggb", 1, 0.5) == (1, 30) and hm.percentile_bin(hist, "rggb", 1, 0.51) == (1, 40)
    assert hm.percentile_bin(hist, "rggb", 2, 0.0) == (1, 100) and hm.percentile_bin(hist, "rggb", 3, 1.0) == (1, 100)
    assert hm.percentile_bin(np.zeros((4, 256), np.uint32), "rggb", 3, 0.5) == (0, -1)
    # levels 10 / 255, 40 / 255, 100 / 255 -> 0.9 * 255 / 100
    assert hm.exposure(hist, "rggb", 8, fraction=0.99, target=0.9, max_gain=4.0) == (1, 0.9 / (100.0 / 255.0))
    assert hm.exposure(hist, "rggb", 8, max_gain=2.0) == (1, 2.0)
    assert hm.exposure(hist, "bggr", 8, gains=(0.0, 0.0, 0.0)) == (0, 1.0)
