"""CPU tests of tests/dpc_model.py, the NumPy restatement of the defective pixel correction (include/mibayer.h, group
`dpc`): the vectorised model against the definition pixel by pixel, the border rule, the order of the pairs and of their
ties, the thresholds' ends, and the property the block exists for -- on a noise-free ramp exactly the planted defects
change, and each lands among its neighbours."""
import numpy as np
import pytest

import dpc_model as dm


@pytest.mark.parametrize("w,h,depth", [(4, 4, 8), (6, 5, 8), (4, 7, 12), (9 + 1, 4, 16), (14, 11, 10), (22, 9, 16)])
def test_model_matches_the_definition_pixel_by_pixel(w, h, depth):
    rng = np.random.default_rng([w, h, depth])
    vmax = (1 << depth) - 1
    for S in (rng.integers(0, vmax + 1, (h, w)), rng.choice([0, vmax], (h, w)), rng.integers(0, 4, (h, w))):
        lst = np.stack([rng.integers(0, w, 6), rng.integers(0, h, 6)], 1)
        for hot, cold, defects in ((0, 0, None), (vmax // 6, -1, None), (-1, vmax // 6, lst), (vmax, vmax, lst), (-1, -1, lst),
                                   (1, 1, lst[:1]), (-1, -1, None)):
            assert np.array_equal(dm.correct(S, hot, cold, defects), dm.correct_slow(S, hot, cold, defects)), (hot, cold)


def test_border_substitution_at_every_edge_and_corner():
    """S[y, x] = 100 y + x names every sample: the neighbour of a coordinate off the frame is the one on the other side"""
    h, w = 7, 9
    y, x = np.mgrid[0:h, 0:w]
    S = 100 * y + x
    n = dm.neighbours(S)
    for yy in range(h):
        for xx in range(w):
            for (dx, dy), arr in n.items():
                nx, ny = xx + 2 * dx, yy + 2 * dy
                nx = nx + 4 if nx < 0 else nx - 4 if nx >= w else nx
                ny = ny + 4 if ny < 0 else ny - 4 if ny >= h else ny
                assert arr[yy, xx] == 100 * ny + nx, (xx, yy, dx, dy)
    assert n[(-1, -1)][0, 0] == 202 and n[(1, 1)][h - 1, w - 1] == 100 * (h - 3) + w - 3       # the corners
    assert n[(-1, 0)][3, 1] == 303 and n[(1, 0)][3, w - 2] == 300 + w - 4 and n[(0, -1)][1, 4] == 304
    lo, hi = dm.mirror(4)
    assert lo.tolist() == [2, 3, 0, 1] and hi.tolist() == [2, 3, 0, 1]         # the smallest frame: both sides coincide
    for bad in ((3, 8), (8, 3), (2, 2)):
        with pytest.raises(ValueError):
            dm.neighbours(np.zeros(bad))


def cross(vals, centre=0):
    """a 5 x 5 frame's worth of same-site neighbours around (4, 4) of a 9 x 9 frame: vals = (l, r, u, d, ul, dr, ur, dl)"""
    S = np.full((9, 9), 50, np.int64)
    l, r, u, d, ul, dr, ur, dl = vals
    S[4, 2], S[4, 6], S[2, 4], S[6, 4], S[2, 2], S[6, 6], S[2, 6], S[6, 2] = l, r, u, d, ul, dr, ur, dl
    S[4, 4] = centre
    return S


def test_pair_order_and_ties():
    """each of H, V, D1, D2 wins when its gradient is the smallest; among equals the first in that order wins; the
    rounding is upwards"""
    base = [(10, 20), (30, 50), (60, 90), (100, 140)]           # gradients 10, 20, 30, 40
    for k in range(4):
        pairs = list(base)
        pairs[0], pairs[k] = pairs[k], pairs[0]                 # pair k gets the gradient 10
        vals = [v for p in pairs for v in p]
        R, win = dm.replacement(cross(vals))
        assert win[4, 4] == k and R[4, 4] == 15, (k, dm.PAIRS[k])
    # ties: all four equal -> H; H larger, the rest equal -> V; only the diagonals equal and smallest -> D1
    for vals, k, r in (((10, 20, 110, 120, 210, 220, 310, 320), 0, 15), ((10, 30, 110, 120, 210, 220, 310, 320), 1, 115),
                       ((10, 30, 110, 130, 210, 220, 320, 310), 2, 215), ((0, 9, 0, 9, 0, 9, 9, 1), 3, 5),
                       ((7, 7, 0, 0, 3, 3, 9, 9), 0, 7), ((0, 1, 5, 5, 3, 3, 9, 9), 1, 5)):
        R, win = dm.replacement(cross(vals))
        assert (win[4, 4], R[4, 4]) == (k, r), vals
    assert dm.replacement(cross((0, 1, 9, 0, 9, 0, 9, 0)))[0][4, 4] == 1       # (0 + 1 + 1) >> 1
    assert dm.replacement(cross((65535, 65535) + (0, 9) * 3))[0][4, 4] == 65535


def test_thresholds_0_max_and_off():
    vmax = 255
    S = cross((50,) * 8, centre=51)
    assert dm.flagged(S, 0, -1)[4, 4] and not dm.flagged(S, 1, -1)[4, 4] and not dm.flagged(S, -1, 0)[4, 4]
    S = cross((50,) * 8, centre=49)
    assert dm.flagged(S, -1, 0)[4, 4] and not dm.flagged(S, -1, 1)[4, 4] and not dm.flagged(S, 0, -1)[4, 4]
    S = cross((50,) * 8, centre=50)
    assert not dm.flagged(S, 0, 0)[4, 4]                # equal is neither hot nor cold
    # one neighbour at the sample's level is enough to keep it
    assert not dm.flagged(cross((50,) * 7 + (200,), centre=200), 0, -1)[4, 4]
    assert not dm.flagged(cross((50,) * 7 + (3,), centre=3), -1, 0)[4, 4]
    # at max nothing can be flagged, whatever the frame; off flags nothing either
    rng = np.random.default_rng(1)
    S = rng.choice([0, vmax], (12, 14))
    assert not dm.flagged(S, vmax, vmax).any() and not dm.flagged(S, -1, -1).any()
    lone = cross((0,) * 8, centre=vmax)
    lone[lone == 50] = 0
    assert dm.flagged(lone, vmax - 1, -1)[4, 4] and not dm.flagged(lone, vmax, -1)[4, 4]


def test_identity_when_everything_is_off():
    rng = np.random.default_rng(2)
    S = rng.integers(0, 1 << 14, (11, 18))
    assert np.array_equal(dm.correct(S), S) and np.array_equal(dm.correct(S, -1, -1, np.zeros((0, 2), np.uint32)), S)
    assert np.array_equal(dm.correct(S, 0, 0, None, y0=5, y1=5), S)
    part = dm.correct(S, 0, 0, None, y0=3, y1=8)
    full = dm.correct(S, 0, 0)
    assert np.array_equal(part[3:8], full[3:8]) and np.array_equal(part[:3], S[:3]) and np.array_equal(part[8:], S[8:])


def test_the_list():
    lst = [(5, 7), (1, 2), (5, 7), (0, 7), (9, 0)]
    assert dm.sort_defects(lst).tolist() == [[9, 0], [1, 2], [0, 7], [5, 7]] and dm.sort_defects([]).shape == (0, 2)
    S = np.arange(12 * 10).reshape(10, 12) % 7
    with pytest.raises(ValueError):
        dm.correct(S, -1, -1, [(12, 0)])
    with pytest.raises(ValueError):
        dm.correct(S, -1, -1, [(0, 10)])
    out = dm.correct(S, -1, -1, lst)
    R, _ = dm.replacement(S)
    changed = {(x, y) for y, x in np.argwhere(out != S)}
    assert changed <= set(lst) and all(out[y, x] == R[y, x] for x, y in lst)
    # two listed defects of one site two pixels apart see each other: the neighbours are the source's
    S = np.full((9, 9), 50)
    S[4, 4] = S[4, 6] = 255
    assert dm.correct(S, -1, -1, [(4, 4), (6, 4)])[4, 4] == 50         # (V wins: H has the other defect in it)
    S[2, 4] = 0
    assert dm.correct(S, -1, -1, [(4, 4), (6, 4)])[4, 4] == 50         # D1


@pytest.mark.parametrize("depth,w,h", [(12, 96, 64), (8, 64, 40), (16, 50, 34)])
def test_the_ramp_property(depth, w, h):
    """a noise-free ramp with per-site offsets whose same-site step is <= the thresholds, stuck-at-0 and stuck-at-max
    samples at least 5 pixels apart: exactly the planted samples change, each lands within [lo, hi] of its neighbours,
    and a clean ramp changes nowhere.  Exact, no tolerance."""
    vmax = (1 << depth) - 1
    t = vmax // 64
    y, x = np.mgrid[0:h, 0:w]
    step = max(1, t // 4)                               # per pixel: the same-site step is 2 or 4 of them, <= t
    clean = vmax // 4 + step * (x // 2) + step * (y // 2) + (vmax // 32) * (2 * (y & 1) + (x & 1))
    assert clean.max() < vmax - t and clean.min() > t
    n = np.stack(list(dm.neighbours(clean).values()))
    assert np.abs(n - clean).max() <= t
    assert np.array_equal(dm.correct(clean, t, t), clean)
    rng = np.random.default_rng([depth, w])
    where = [(xx + int(rng.integers(0, 2)), yy + int(rng.integers(0, 2))) for yy in range(0, h - 1, 6) for xx in range(0, w - 1, 6)]
    where.append((w - 1, h - 1))
    S = clean.copy()
    for k, (xx, yy) in enumerate(where):
        S[yy, xx] = vmax if k % 2 else 0
    out = dm.correct(S, t, t)
    changed = {(xx, yy) for yy, xx in np.argwhere(out != S)}
    assert changed == set(where) and len(where) > 50
    n = np.stack(list(dm.neighbours(S).values()))
    for xx, yy in where:
        assert n[:, yy, xx].min() <= out[yy, xx] <= n[:, yy, xx].max()
        assert abs(out[yy, xx] - clean[yy, xx]) <= 2 * step


def test_the_defect_file_reader(tmp_path):
    p = tmp_path / "defects.txt"
    p.write_text("# sensor 0042\n\n3 4\n  10\t7   # a comment\n3 4\n")
    assert dm.read_defect_file(str(p)).tolist() == [[3, 4], [10, 7], [3, 4]]
    p.write_text("3 4 5\n")
    with pytest.raises(ValueError):
        dm.read_defect_file(str(p))
