"""CPU tests of the noise reduction's definition (tests/nr_model.py, include/mibayer.h group `nr`): the properties the
definition claims, the vectorised model against the pixel-by-pixel one, the threshold interpolation, and the reciprocal
the kernel divides with -- proven over its whole domain."""
import numpy as np
import pytest

import nr_model as nm

DEPTHS = (8, 10, 12, 14, 16)


def noisy_mosaic(rng, w, h, depth, sigma_share=1 / 64):
    """four site levels plus rounded Gaussian noise"""
    vmax = (1 << depth) - 1
    y, x = np.mgrid[0:h, 0:w]
    levels = vmax // 4 + (vmax // 8) * (2 * (y & 1) + (x & 1))
    return np.clip(levels + np.rint(rng.normal(0, vmax * sigma_share, (h, w))).astype(np.int64), 0, vmax)


@pytest.mark.parametrize("depth", DEPTHS)
def test_model_is_the_definition_pixel_by_pixel(depth):
    rng = np.random.default_rng([1, depth])
    vmax = (1 << depth) - 1
    for w, h in ((6, 5), (6, 6), (14, 11), (22, 9)):
        for S in (rng.integers(0, vmax + 1, (h, w)), noisy_mosaic(rng, w, h, depth)):
            curve = rng.integers(0, nm.t_max(depth) + 1, nm.NODES)
            out = nm.denoise(S, curve, depth)
            assert np.array_equal(out, nm.denoise_slow(S, curve, depth))
            assert out.min() >= 0 and out.max() <= vmax


def test_frames_smaller_than_the_window_are_refused():
    for w, h in ((4, 8), (8, 4), (6, 4)):
        with pytest.raises(ValueError):
            nm.denoise(np.zeros((h, w), np.int64), [0] * nm.NODES, 8)


@pytest.mark.parametrize("depth", DEPTHS)
def test_zero_curve_is_the_identity(depth):
    rng = np.random.default_rng([2, depth])
    S = rng.integers(0, 1 << depth, (13, 18))
    assert np.array_equal(nm.denoise(S, [0] * nm.NODES, depth), S)


@pytest.mark.parametrize("depth", DEPTHS)
def test_four_constant_sites_are_unchanged_under_the_largest_curve(depth):
    vmax = (1 << depth) - 1
    y, x = np.mgrid[0:11, 0:14]
    for levels in ((0, vmax, vmax // 2, 1), (vmax, 0, 0, vmax)):
        S = np.choose(2 * (y & 1) + (x & 1), levels)
        assert np.array_equal(nm.denoise(S, [nm.t_max(depth)] * nm.NODES, depth), S)


@pytest.mark.parametrize("depth", DEPTHS)
def test_output_lies_within_the_included_samples(depth):
    rng = np.random.default_rng([3, depth])
    S = noisy_mosaic(rng, 34, 21, depth, 1 / 32)
    # thresholds of up to two standard deviations: some neighbours are in and some are out
    curve = rng.integers(0, min(nm.t_max(depth), (1 << depth) // 16) + 1, nm.NODES)
    out = nm.denoise(S, curve, depth)
    n, inc = nm.neighbours(S), nm.included(S, curve, depth)
    lo = np.minimum(np.where(inc, n, S).min(0), S)
    hi = np.maximum(np.where(inc, n, S).max(0), S)
    assert (out >= lo).all() and (out <= hi).all()
    assert 0.05 < inc.mean() < 0.95


def test_a_step_larger_than_t_is_unchanged():
    S = np.full((16, 24), 60, np.int64)
    S[:, 12:] = 160
    assert np.array_equal(nm.denoise(S, [12] * nm.NODES, 8), S)
    # ... and one of exactly t is not
    S[:, 12:] = 72
    assert not np.array_equal(nm.denoise(S, [12] * nm.NODES, 8), S)


def test_a_flat_noisy_field_gets_quieter():
    rng = np.random.default_rng(4)
    S = np.clip(128 + np.rint(rng.normal(0, 4, (96, 128))).astype(np.int64), 0, 255)
    out = nm.denoise(S, [12] * nm.NODES, 8)
    print("sigma %.3f -> %.3f" % (S.std(), out.std()))
    assert out.std() < S.std()


@pytest.mark.parametrize("depth", DEPTHS)
def test_threshold_interpolation_at_every_node_and_between(depth):
    rng = np.random.default_rng([5, depth])
    sh = depth - 4
    s = 1 << sh
    curve = rng.integers(0, nm.t_max(depth) + 1, nm.NODES)
    nodes = np.arange(16) << sh
    assert np.array_equal(nm.threshold(nodes, curve, depth), curve[:16])
    mid = nodes + (s >> 1)
    assert np.array_equal(nm.threshold(mid, curve, depth), (curve[:16] + curve[1:] + 1) >> 1)
    # the last sample of every interval, max included (k = 15, f = s - 1: node 16 is never reached, only approached)
    end = nodes + s - 1
    assert np.array_equal(nm.threshold(end, curve, depth), (curve[:16] + curve[1:] * (s - 1) + (s >> 1)) >> sh)
    assert end[-1] == (1 << depth) - 1
    # every value: between the two nodes, and what exact rational arithmetic rounds to
    S = np.arange(1 << depth)
    t = nm.threshold(S, curve, depth)
    k = S >> sh
    assert (t >= np.minimum(curve[k], curve[k + 1])).all() and (t <= np.maximum(curve[k], curve[k + 1])).all()
    f = S & (s - 1)
    assert np.array_equal(t, np.floor((curve[k] * (s - f) + curve[k + 1] * f) / s + 0.5).astype(np.int64))
    # the kernel's form: curve[k] + ((curve[k + 1] - curve[k]) f + s / 2 >> sh), with a shift that floors
    assert np.array_equal(t, curve[k] + (((curve[k + 1] - curve[k]) * f + (s >> 1)) >> sh))
    with pytest.raises(ValueError):
        nm.threshold(S, [nm.t_max(depth) + 1] * nm.NODES, depth)


def test_the_reciprocal_is_exact_over_its_whole_domain():
    """for cnt = 1 .. 25 and every 2 |v| + cnt with |v| <= 24 * 2047, the high 32 bits of the product with
    ceil (2^32 / (2 cnt)) are the floor quotient by 2 cnt"""
    v = np.arange(24 * 2047 + 1, dtype=np.uint64)
    for cnt in range(1, 26):
        m = nm.reciprocal(cnt)
        assert m == -(-(1 << 32) // (2 * cnt)) and m < 1 << 32
        num = 2 * v + np.uint64(cnt)
        assert np.array_equal((num * np.uint64(m)) >> np.uint64(32), num // np.uint64(2 * cnt)), cnt


def test_noise_curve():
    assert nm.noise_curve(8, 0, 2, 0, 1.5) == [3] * 17
    c = nm.noise_curve(12, 256, 4, 0.5, 2)
    assert c[0] == c[1] == 8 and c == sorted(c) and c[16] == int(2 * (16 + 0.5 * (4096 - 256)) ** 0.5 + 0.5)
    assert nm.noise_curve(16, 0, 0, 1e9, 1e9) == [0] + [2047] * 16
    assert nm.noise_curve(8, 0, 1e6, 0, 1) == [255] * 17 and nm.noise_curve(10, 0, 1e6, 0, 1) == [1023] * 17
    for bad in ((-1, 2, 0, 1), (0, float("nan"), 0, 1), (0, 2, float("inf"), 1), (0, 2, 0, -0.5)):
        with pytest.raises(ValueError):
            nm.noise_curve(8, *bad)
