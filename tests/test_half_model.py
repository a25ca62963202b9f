"""CPU tests of tests/half_model.py (MIBAYER_FLAG_HALF): the model tied to the reference-pinned full-resolution oracle.

The full demosaic leaves every sample where it is: at a red site its R IS the sample, at a green site its G, at a blue
site its B -- borders and odd heights included.  So the half-size pixel of a quad is the full-resolution frame's R at
the quad's red site, its B at the blue site and (G_a + G_b + 1) >> 1 of its G at the two green sites: an identity between
half_model.native_rgb_half and oracle/bayer2rgb_np.py (8-bit) / highbit_model.native_rgb (deep) with no arithmetic in
between but the green mean."""
import numpy as np
import pytest

import colour_model as cm
import half_model as hf
import highbit_model as hm
import planar_model as pm
from oracle import bayer2rgb_np

SIZES = ((4, 3), (6, 4), (6, 5), (10, 7), (34, 9), (514, 6))
ORDERS = ("bggr", "gbrg", "grbg", "rggb")


def at_sites(full, order, oh, ow):
    """the full-resolution (H, W, 3) frame's R at the quads' red sites, G at both green sites, B at the blue sites"""
    (ry, rx), (ay, ax), (by_, bx), (ly, lx) = hf.SITES[order]
    pick = lambda dy, dx, c: full[dy:2 * oh:2, dx:2 * ow:2, c]         # noqa: E731
    return pick(ry, rx, 0), pick(ay, ax, 1), pick(by_, bx, 1), pick(ly, lx, 2)


def check(half, full, order, w, h):
    ow, oh = hf.out_size(w, h)
    assert half.shape == (oh, ow, 3) and (ow, oh) == (w // 2, h >> 1)
    r, ga, gb, b = at_sites(full.astype(np.int64), order, oh, ow)
    assert np.array_equal(half[..., 0], r), (order, w, h)
    assert np.array_equal(half[..., 2], b), (order, w, h)
    assert np.array_equal(half[..., 1], (ga + gb + 1) >> 1), (order, w, h)


@pytest.mark.parametrize("order", ORDERS)
def test_half_is_the_oracles_frame_at_the_quads_own_sites(order):
    rng = np.random.default_rng(11)
    for w, h in SIZES:
        S = rng.integers(0, 256, (h, w), dtype=np.uint8)
        full = bayer2rgb_np.bayer2rgb(S, order, 0, 1, 2).reshape(h, w, 4)[..., :3]
        check(hf.native_rgb_half(S, order), full, order, w, h)
        # ... and the full-resolution sites hold the samples themselves
        (ry, rx), _, _, (ly, lx) = hf.SITES[order]
        assert np.array_equal(full[ry::2, rx::2, 0], S[ry::2, rx::2]) and np.array_equal(full[ly::2, lx::2, 2], S[ly::2, lx::2])


@pytest.mark.parametrize("order", ORDERS)
def test_half_is_the_deep_models_frame_at_the_quads_own_sites_at_12_bits(order):
    rng = np.random.default_rng(12)
    for w, h in SIZES:
        S = rng.integers(0, 1 << 12, (h, w), dtype=np.int64)
        S[0, 0], S[-1, -1], S[0, -1], S[-1, 0] = 4095, 4095, 0, 4095
        check(hf.native_rgb_half(S, order), hm.native_rgb(S, order), order, w, h)


def test_the_pattern_may_be_a_number_and_the_domain_is_the_mosaics():
    S = np.arange(24, dtype=np.int64).reshape(4, 6)
    for name, num in hf.PATTERNS.items():
        assert np.array_equal(hf.native_rgb_half(S, num), hf.native_rgb_half(S, name))
    for bad in ((3, 2), (3, 5), (2, 6)):
        with pytest.raises(ValueError):
            hf.native_rgb_half(np.zeros(bad, np.int64), "bggr")
    # rggb, quad (0, 0) of rows 0-1: R = S(0,0), G = avg (S(1,0), S(0,1)), B = S(1,1)
    assert tuple(hf.native_rgb_half(S, "rggb")[0, 0]) == (0, (1 + 6 + 1) >> 1, 7)
    assert tuple(hf.native_rgb_half(S, "gbrg")[1, 2]) == (S[3, 4], (S[2, 4] + S[3, 5] + 1) >> 1, S[2, 5])


def test_layouts_compose_with_the_existing_models():
    """4-byte, 8-byte, 3-byte and planar frames of one mosaic hold the same values; the padding is the guard"""
    rng = np.random.default_rng(13)
    w, h = 10, 7
    S = rng.integers(0, 1 << 12, (h, w), dtype=np.int64)
    src = hm.pack(S | 0xF000)                                   # junk above the 12 bits
    ow, oh = hf.out_size(w, h)
    rgb = hf.native_rgb_half(S, "grbg")
    four = hf.frame(src, w, h, "grbg", "xBGR", bits=12)
    assert four.shape == (oh, 4 * ow) and np.array_equal(four.reshape(oh, ow, 4)[..., 3], rgb[..., 0] >> 4)
    wide = hf.frame(src, w, h, "grbg", "ARGB64", bits=12, dst_big_endian=True, dst_stride=8 * ow + 8)
    assert wide.shape == (oh, 8 * ow + 8) and (wide[:, 8 * ow:] == hf.GUARD).all()
    assert np.array_equal(wide[:, :8 * ow].copy().view(">u2").reshape(oh, ow, 4)[..., 1:], rgb << 4)
    three = hf.frame(src, w, h, "grbg", "BGR", bits=12)
    assert three.shape == (oh, 16) and (three[:, 15:] == hf.GUARD).all()
    assert np.array_equal(three[:, :15].reshape(oh, ow, 3)[..., ::-1], rgb >> 4)
    planar = hf.frame(src, w, h, "grbg", "GBR", bits=12).reshape(3, oh, 8)
    for c in range(3):
        assert np.array_equal(planar[pm.FORMATS["GBR"][c], :, :ow], rgb[..., c] >> 4)
    assert (planar[:, :, ow:] == hf.GUARD).all()
    col = dict(black=(64, 64, 64), matrix=(8192, 0, 0, 0, 4096, 0, 0, 0, 2048), tone=None)
    staged = hf.frame(src, w, h, "grbg", "RGBx", bits=12, colour=col)
    assert np.array_equal(staged.reshape(oh, ow, 4)[..., :3], cm.stage(rgb, 12, **col))
