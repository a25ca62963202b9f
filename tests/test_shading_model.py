"""CPU tests of the NumPy model of the lens shading correction (tests/shading_model.py; include/mibayer.h, group
`shading`): identities, node positions, the extremes of the integer ranges, and a vignetted flat field taken through
statistics -> mibayer_stats_shading (the model's and the library's, which must agree to the last bit) -> apply."""
import numpy as np
import pytest

import shading_model as shm
import stats_model as sm


def planes(nx, ny, values):
    """a table whose four site planes are constant `values`"""
    return np.stack([np.full((ny, nx), v, np.uint16) for v in values])


@pytest.mark.parametrize("depth", [8, 10, 12, 14, 16])
@pytest.mark.parametrize("kx,ky", [(2, 2), (8, 8), (2, 8), (5, 3)])
def test_unity_table_is_the_identity_whatever_the_black_level(depth, kx, ky):
    rng = np.random.default_rng(depth * 100 + kx * 10 + ky)
    W, H, vmax = 70, 37, (1 << depth) - 1
    S = rng.integers(0, vmax + 1, (H, W))
    S[0, :4] = (0, vmax, 0, vmax)
    nx, ny = shm.nodes(W, H, kx, ky)
    for black in ((0, 0, 0, 0), (vmax,) * 4, tuple(rng.integers(0, vmax + 1, 4))):
        assert np.array_equal(shm.apply(S, planes(nx, ny, (4096,) * 4), kx, ky, black, depth), S)


@pytest.mark.parametrize("kx,ky", [(2, 2), (8, 8), (2, 8), (5, 3)])
def test_gain_equals_the_node_value_at_node_positions(kx, ky):
    W, H = 2 * (1 << kx) + 6, 2 * (1 << ky) + 3
    nx, ny = shm.nodes(W, H, kx, ky)
    table = np.random.default_rng(kx + 9 * ky).integers(0, 32768, (4, ny, nx)).astype(np.uint16)
    G = shm.gain_map(table, W, H, kx, ky)
    for j in range(ny):
        for i in range(nx):
            x, y = i << kx, j << ky
            if x < W and y < H:
                assert G[y, x] == table[2 * (y & 1) + (x & 1), j, i]         # both even: site 0
    # one pixel right of / below a node of an even row and column: sites 1 and 2, weights (cw - 1, 1) / (ch - 1, 1)
    cw, ch = 1 << kx, 1 << ky
    t = table.astype(np.int64)
    assert G[0, 1] == ((t[1, 0, 0] * (cw - 1) + t[1, 0, 1]) * ch + (1 << (kx + ky - 1))) >> (kx + ky)
    assert G[1, 0] == ((t[2, 0, 0] * (ch - 1) + t[2, 1, 0]) * cw + (1 << (kx + ky - 1))) >> (kx + ky)


def test_vectorised_and_pixel_by_pixel_models_agree():
    rng = np.random.default_rng(5)
    for (W, H, kx, ky, depth) in [(38, 21, 2, 3, 8), (70, 9, 5, 2, 12), (20, 33, 3, 4, 16)]:
        nx, ny = shm.nodes(W, H, kx, ky)
        table = rng.integers(0, 32768, (4, ny, nx)).astype(np.uint16)
        vmax = (1 << depth) - 1
        S = rng.integers(0, vmax + 1, (H, W))
        black = rng.integers(0, vmax + 1, 4)
        assert np.array_equal(shm.apply(S, table, kx, ky, black, depth), shm.apply_slow(S, table, kx, ky, black, depth))


@pytest.mark.parametrize("depth", [8, 16])
def test_extremes_stay_inside_32_bits_and_clamp(depth):
    """gain 0 and 32767, S = 0 and max, black = 0 and max, the largest cells: gain_map () and apply () assert that
    their intermediate values fit uint32 / int32"""
    kx = ky = 8
    W, H, vmax = 260, 259, (1 << depth) - 1
    nx, ny = shm.nodes(W, H, kx, ky)
    for S_val in (0, vmax):
        S = np.full((H, W), S_val, np.int64)
        for gain in (0, 32767):
            for black in (0, vmax):
                out = shm.apply(S, planes(nx, ny, (gain,) * 4), kx, ky, (black,) * 4, depth)
                d = S_val - black
                want = min(max(black + ((d * gain + 2048) >> 12), 0), vmax)
                assert (out == want).all(), (S_val, gain, black)
    # gain 0 leaves the black level, the largest gain saturates white and keeps black at zero
    S = np.full((H, W), vmax, np.int64)
    assert (shm.apply(S, planes(nx, ny, (0,) * 4), kx, ky, (7,) * 4, depth) == 7).all()
    assert (shm.apply(S, planes(nx, ny, (32767,) * 4), kx, ky, (0,) * 4, depth) == vmax).all()
    assert (shm.apply(S * 0, planes(nx, ny, (32767,) * 4), kx, ky, (vmax,) * 4, depth) == 0).all()


def test_nodes_rule():
    assert shm.nodes(4, 3, 2, 2) == (2, 2)
    assert shm.nodes(5, 5, 2, 2) == (3, 3)              # W - 1 exactly on a cell boundary
    assert shm.nodes(512, 508, 2, 2) == (129, 128)
    for bad in ((513, 4, 2, 2), (4, 513, 2, 2), (4, 4, 1, 2), (4, 4, 2, 9), (0, 4, 2, 2)):
        with pytest.raises(ValueError):
            shm.nodes(*bad)


def flat_field(W, H, levels, black, depth):
    """a flat field under cos^4 fall-off (focal length = the half diagonal: the corners lose two stops), four site
    levels over a black pedestal"""
    y, x = np.mgrid[0:H, 0:W]
    r2 = ((x - (W - 1) / 2.0) ** 2 + (y - (H - 1) / 2.0) ** 2) / (((W - 1) / 2.0) ** 2 + ((H - 1) / 2.0) ** 2)
    fall = 1.0 / (1.0 + r2) ** 2                        # cos^4 (atan (r / f))
    lv = np.asarray(levels, float)[2 * (y & 1) + (x & 1)]
    S = np.rint(black + lv * fall).astype(np.int64)
    assert S.max() <= (1 << depth) - 1
    return S


def stats_shading(pkg, zones, *args):
    """the model's answer and mibayer_stats_shading's (pure host code: no device needed), which must be the same to the
    last bit"""
    ok, table = shm.stats_shading(zones, *args)
    lib_ok, lib_table = pkg.stats_shading(zones, *args)
    assert lib_ok == ok and lib_table.dtype == table.dtype
    assert np.array_equal(lib_table, table), np.argwhere(lib_table != table)[:5]
    return ok, table


# code values per site, measured with this model (the docstring below)
RESIDUAL_PER_SITE = (211, 169, 167, 112)
RESIDUAL_INNER = (60, 36, 39, 17)


def test_vignetted_flat_field_comes_out_flat(pkg):
    """640 x 480, 12 bits, black 64, site levels 3000 / 2600 / 2500 / 1800 at the centre, corners at a quarter of that;
    statistics over 40 x 30 zones (16 x 16 pixels each), cells of 32 x 32, max_gain 7.99.  What bilinear interpolation
    over zone means, clamped at the borders, leaves: per site, max - min of the corrected field.  Measured with this
    model (the library's table is the same to the last bit, which the test asserts too), sites 0 .. 3: 211, 169, 167,
    112 code values over the whole frame (7 % of the level, against a spread of 75 % before), and 60, 36, 39, 17 without
    the outermost cell on every side (2 %).  The border carries the largest error:
    the nodes at x = 0 and y = 0 and those past the last pixel lie outside the outermost zone centres, where the zone
    mean is held and not extrapolated, and the fall-off is steepest there.  The assertions take these values plus one
    code value."""
    W, H, depth, black = 640, 480, 12, 64
    levels = (3000, 2600, 2500, 1800)
    S = flat_field(W, H, levels, black, depth)
    before = [int(np.ptp(S[s >> 1::2, s & 1::2])) for s in range(4)]
    zones = sm.zone_stats(S, 40, 30, 0, 4095)
    ok, table = stats_shading(pkg, zones, W, H, (black,) * 4, 5, 5, 7.99)
    assert ok == 1 and table.min() >= 4096 and table.max() <= 32727
    out = shm.apply(S, table, 5, 5, (black,) * 4, depth)
    spread = [int(np.ptp(out[s >> 1::2, s & 1::2])) for s in range(4)]
    inner = [int(np.ptp(out[32:-32, 32:-32][s >> 1::2, s & 1::2])) for s in range(4)]
    print("spread before", before, "after", spread, "without the outermost cells (32 pixels)", inner)
    for s in range(4):
        assert before[s] > 0.7 * levels[s]
        assert spread[s] <= RESIDUAL_PER_SITE[s] + 1, (s, spread)
        assert inner[s] <= RESIDUAL_INNER[s] + 1, (s, inner)
    # the field is corrected TO its brightest node: the centre keeps its level
    for s in range(4):
        centre = out[s >> 1::2, s & 1::2][H // 4, W // 4] - black
        assert abs(int(centre) - levels[s]) <= RESIDUAL_INNER[s] + 1


def test_stats_shading_refuses_empty_and_dark_sites(pkg):
    W, H = 64, 48
    S = np.full((H, W), 100, np.int64)
    zones = sm.zone_stats(S, 4, 3, 0, 255)
    ok, table = stats_shading(pkg, zones, W, H, None, 4, 4, 4.0)
    assert ok == 1 and (table == 4096).all()            # a flat field without fall-off: unity
    ok, table = stats_shading(pkg, zones, W, H, (0, 100, 0, 0), 4, 4, 4.0)
    assert ok == 0 and (table == 4096).all()            # site 1: mean == black
    z = zones.copy()
    z["count"][..., 2] = 0
    ok, table = stats_shading(pkg, z, W, H, None, 4, 4, 4.0)
    assert ok == 0 and (table == 4096).all()            # site 2 has no samples
    z = zones.copy()
    z["count"][0, 0, :] = 0                             # one empty zone: its neighbour's mean
    ok, table = stats_shading(pkg, z, W, H, None, 4, 4, 4.0)
    assert ok == 1 and (table == 4096).all()
    # the clamp: a zone 16 times darker asks for gain 16 and gets max_gain
    z = zones.copy()
    z["sum"][0, 0, :] //= 16
    ok, table = stats_shading(pkg, z, W, H, None, 4, 4, 7.99)
    assert ok == 1 and table[:, 0, 0].tolist() == [int(7.99 * 4096 + 0.5)] * 4
