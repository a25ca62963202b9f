"""CPU tests of the deep-sample model (tests/highbit_model.py): the arithmetic the GPU tests hold the kernel to.
With 8-bit-valued samples the widened closed form IS the reference's 8-bit output, so the model is pinned to the
reference fixtures first; then the worked example, masking, byte order and the two output conversions."""
import re

import numpy as np
import pytest

import highbit_model as hm

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
FMT8 = ("RGBx", "BGRx", "xRGB", "xBGR")


def golden_cases(golden):
    for key in golden.files:
        m = re.match(r"out_(\d+)x(\d+)_(\w+?)_(\w+)$", key)
        if m:
            yield key, int(m.group(1)), int(m.group(2)), m.group(3), m.group(4)


def test_model_on_8bit_values_is_the_reference(golden):
    """every fixture of tests/golden/bayer2rgb_small.npz, every order and layout: 16-bit words holding the 8-bit
    mosaic, bits = 16, 16-bit output -> the low byte of every channel (alpha 0xffff -> 0xff) is the reference frame;
    bits = 8-equivalent (an 8-bit mosaic) with 8-bit output is the reference frame itself"""
    n = 0
    for key, w, h, pattern, fmt in golden_cases(golden):
        S8 = golden["in_%dx%d" % (w, h)][:, :w]
        want = golden[key]
        words = hm.pack(S8.astype(np.uint16))
        out16 = hm.bayer2rgb_highbit(words, w, h, pattern, fmt, 16, out16=True)
        lo = out16.reshape(h, 4 * w, 2)[..., 0]              # little-endian words: low byte first
        assert np.array_equal(lo, want), key
        hi = out16.reshape(h, 4 * w, 2)[..., 1]
        assert (hi[:, hm.LAYOUTS[fmt][0]::4] == 0).all()     # v << 0 of an 8-bit value: high byte zero
        out8 = hm.bayer2rgb_highbit(S8, w, h, pattern, fmt, 8, out16=False)
        assert np.array_equal(out8, want), key
        n += 1
    assert n >= 100


def test_worked_12bit_example():
    S = np.array([[161, 3215, 487, 2880], [1449, 4002, 1134, 83], [800, 1931, 4085, 13], [534, 1240, 2266, 3556]])
    want = [[(4002, 2332, 161), (4002, 3215, 324), (4002, 2175, 487), (83, 2880, 487)],
            [(4002, 1449, 481), (4002, 1933, 1384), (4002, 1134, 2286), (83, 1291, 2286)],
            [(2621, 1462, 800), (2621, 1931, 2443), (2621, 1816, 4085), (1820, 13, 4085)],
            [(1240, 534, 481), (1240, 1987, 1384), (1240, 2266, 2286), (3556, 1857, 2286)]]
    rgb = hm.native_rgb(S, "bggr")
    assert rgb.tolist() == [[list(p) for p in row] for row in want]
    argb64 = hm.bayer2rgb_highbit(hm.pack(S), 4, 4, "bggr", "ARGB64", 12, out16=True).view("<u2").reshape(4, 4, 4)
    assert (argb64[..., 0] == 0xFFFF).all()
    assert np.array_equal(argb64[..., 1:], np.array(want) << 4)
    rgbx = hm.bayer2rgb_highbit(hm.pack(S), 4, 4, "bggr", "RGBx", 12, out16=False).reshape(4, 4, 4)
    assert np.array_equal(rgbx[..., :3], np.array(want) >> 4) and (rgbx[..., 3] == 255).all()


@pytest.mark.parametrize("bits", [10, 12, 14, 16])
def test_bits_above_the_depth_are_ignored(bits):
    rng = np.random.default_rng(bits)
    w, h = 22, 9
    S = rng.integers(0, 1 << bits, (h, w))
    junk = S | (rng.integers(0, 1 << 16, (h, w)) & ~((1 << bits) - 1) & 0xFFFF)
    if bits < 16:
        assert (junk != S).any()
    for pattern in ORDERS:
        a = hm.bayer2rgb_highbit(hm.pack(S), w, h, pattern, "ARGB64", bits, out16=True)
        b = hm.bayer2rgb_highbit(hm.pack(junk), w, h, pattern, "ARGB64", bits, out16=True)
        assert np.array_equal(a, b)
        assert hm.unpack(hm.pack(junk), w, h, bits=bits).max() < (1 << bits)


def test_little_and_big_endian_containers_agree():
    rng = np.random.default_rng(5)
    w, h = 18, 7
    S = rng.integers(0, 1 << 16, (h, w))
    le, be = hm.pack(S), hm.pack(S, big_endian=True)
    assert not np.array_equal(le, be)
    for bits in (10, 16):
        a = hm.bayer2rgb_highbit(le, w, h, "grbg", "BGRx", bits, out16=False)
        b = hm.bayer2rgb_highbit(be, w, h, "grbg", "BGRx", bits, out16=False, src_big_endian=True)
        assert np.array_equal(a, b)
        c = hm.bayer2rgb_highbit(le, w, h, "grbg", "ARGB64", bits, out16=True)
        d = hm.bayer2rgb_highbit(be, w, h, "grbg", "ARGB64", bits, out16=True, src_big_endian=True,
                                 dst_big_endian=True)
        assert np.array_equal(c.view("<u2"), d.view(">u2"))
    # padded rows: the padding is not part of the frame
    padded = hm.pack(S, stride=2 * w + 12)
    padded[:, 2 * w:] = 0xEE
    assert np.array_equal(hm.unpack(padded, w, h, stride=2 * w + 12), S)


def test_output_conversions():
    rgb = np.array([[[0, 1, 1023], [512, 1000, 3]]], np.int64)
    o16 = hm.to_output(rgb, 10, "RGBA64", out16=True).view("<u2").reshape(1, 2, 4)
    assert o16.tolist() == [[[0, 64, 65472, 65535], [32768, 64000, 192, 65535]]]
    o16be = hm.to_output(rgb, 10, "RGBA64", out16=True, dst_big_endian=True).view(">u2").reshape(1, 2, 4)
    assert np.array_equal(o16, o16be)
    o8 = hm.to_output(rgb, 10, "BGRx", out16=False).reshape(1, 2, 4)
    assert o8.tolist() == [[[255, 0, 0, 255], [0, 250, 128, 255]]]     # >> 2, truncating
    # an 8-bit mosaic with 16-bit output: v << 8
    assert hm.to_output(np.array([[[255, 1, 0]]]), 8, "ARGB64", True).view("<u2").tolist() == [[65535, 65280, 256, 0]]
