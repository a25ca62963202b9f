"""CPU tests of tests/colour_model.py, the NumPy statement of the fused colour stage (include/mibayer.h,
MIBAYER_FLAG_COLOUR): the two identities the header promises and hand-computed answers for every step."""
import numpy as np
import pytest

import colour_model as cm
import highbit_model as hm
import mhc_model as mm


def px(r, g, b):
    return np.array([[[r, g, b]]], np.int64)


def one(rgb, depth, **kw):
    return cm.stage(px(*rgb), depth, **kw)[0, 0].tolist()


def mosaic(rng, w, h, bits):
    if bits == 0:
        return rng.integers(0, 256, (h, (w + 3) & ~3), dtype=np.uint8)
    return hm.pack(rng.integers(0, 1 << bits, (h, w)))


@pytest.mark.parametrize("method", ["bilinear", "mhc"])
@pytest.mark.parametrize("bits", [0, 10, 12, 14, 16])
def test_identity_equals_the_plain_output(method, bits):
    """zero black level + identity matrix, no tone curve == the same cfg without the flag, every output arm"""
    rng = np.random.default_rng(bits + len(method))
    w, h = 22, 9
    buf = mosaic(rng, w, h, bits)
    stride = buf.shape[1]
    for layout, out16, dbe in (("BGRx", False, False), ("xRGB", False, False), ("ARGB64", True, False),
                               ("BGRA64", True, True)):
        if method == "mhc":
            plain = mm.bayer2rgb_mhc(buf, w, h, "grbg", layout, bits=bits, out16=out16, dst_big_endian=dbe, stride=stride)
        else:
            plain = hm.bayer2rgb_highbit(buf, w, h, "grbg", layout, bits or 8, out16, dst_big_endian=dbe, stride=stride)
        got = cm.bayer2rgb_colour(buf, w, h, "grbg", layout, bits=bits, out16=out16, method=method, dst_big_endian=dbe,
                                  stride=stride)
        assert np.array_equal(got, plain), (layout, out16, dbe)


@pytest.mark.parametrize("bits", [0, 10, 12, 14, 16])
def test_linear_tone_leaves_16bit_output_unchanged(bits):
    rng = np.random.default_rng(100 + bits)
    w, h = 18, 7
    buf = mosaic(rng, w, h, bits)
    linear = [256 * i for i in range(257)]
    for method in ("bilinear", "mhc"):
        a = cm.bayer2rgb_colour(buf, w, h, "rggb", "ARGB64", bits=bits, out16=True, method=method, stride=buf.shape[1])
        b = cm.bayer2rgb_colour(buf, w, h, "rggb", "ARGB64", bits=bits, out16=True, method=method, tone=linear,
                                stride=buf.shape[1])
        assert np.array_equal(a, b)
    # every value of the depth, not only the ones a frame happens to hold
    depth = bits or 8
    v = np.arange(1 << depth, dtype=np.int64).reshape(1, -1, 1).repeat(3, axis=2)
    assert np.array_equal(cm.stage(v, depth, tone=linear, out16=True), v << (16 - depth))


def test_black_level_clamps_at_zero():
    assert one((10, 200, 5), 8, black=(20, 50, 5)) == [0, 150, 0]
    assert one((10, 200, 5), 8, black=(20, 50, 5), out16=True) == [0, 150 << 8, 0]
    assert one((1023, 64, 63), 10, black=(64, 64, 64)) == [959 >> 2, 0, 0]


def test_negative_matrix_entries_and_clamp_at_zero():
    m = (4096, -2048, 0, -4096, 4096, 0, 0, -8192, 4096)
    # R' = 100 - 100 = 0, G' = -100 + 200 = 100, B' = -400 + 300 = -100 -> 0
    assert one((100, 200, 300), 10, matrix=m, out16=True) == [0, 100 << 6, 0]
    assert one((300, 200, 300), 10, matrix=m, out16=True) == [200 << 6, 0, 0]


def test_saturation_at_max():
    m = (8192, 0, 0, 0, 8192, 0, 0, 0, 8192)
    assert one((4000, 2047, 2048), 12, matrix=m, out16=True) == [4095 << 4, 4094 << 4, 4095 << 4]
    assert one((200, 127, 128), 8, matrix=m) == [255, 254, 255]


def test_rounding_at_one_half():
    """(acc + 2048) >> 12 with an arithmetic shift: halves round up, towards +infinity, negative sums included"""
    half = (2048, 0, 0, 0, 4096, 0, 0, 0, 4096)
    assert one((1, 0, 0), 8, matrix=half)[0] == 1           # 0.5 -> 1
    assert one((3, 0, 0), 8, matrix=half)[0] == 2           # 1.5 -> 2
    assert one((2, 0, 0), 8, matrix=half)[0] == 1
    m = (-2048, 4096, 0, 0, 4096, 0, 0, 0, 4096)
    assert one((1, 5, 0), 8, matrix=m)[0] == 5              # 4.5 -> 5
    assert one((3, 5, 0), 8, matrix=m)[0] == 4              # 3.5 -> 4
    assert one((3, 1, 0), 8, matrix=m)[0] == 0              # -0.5 -> (−2048 + 2048) >> 12 = 0
    assert one((5, 1, 0), 8, matrix=m)[0] == 0              # -1.5 -> -1 -> clamped
    m4095 = (4095, 0, 0, 0, 4097, 0, 0, 0, 4096)
    assert one((2048, 2048, 0), 12, matrix=m4095, out16=True)[:2] == [2048 << 4, 2049 << 4]   # 2047.5 -> 2048, 2048.5 -> 2049
    assert one((2047, 2047, 0), 12, matrix=m4095, out16=True)[:2] == [2047 << 4, 2047 << 4]


def test_tone_curve_interpolation_and_last_segment():
    linear = [256 * i for i in range(257)]
    # depth 16, c' = 65535: i = 255, f = 255 -> (65280 * 1 + 65536 * 255 + 128) >> 8 = 65535
    assert one((65535, 65535, 65535), 16, tone=linear, out16=True) == [65535] * 3
    # a table that ends flat at 65536: the last segment is used and the result is capped at 65535
    flat = [256 * i for i in range(255)] + [65536, 65536]
    assert one((65535, 0xFF00, 0xFE80), 16, tone=flat, out16=True) == [65535, 65535, (65024 * 128 + 65536 * 128 + 128) >> 8]
    # 8-bit samples sit on the nodes: i = c', f = 0
    tone = [(i * i) & 0xFFFF for i in range(256)] + [65536]
    assert one((255, 16, 3), 8, tone=tone, out16=True) == [tone[255], tone[16], tone[3]]
    assert one((255, 16, 3), 8, tone=tone) == [tone[255] >> 8, tone[16] >> 8, tone[3] >> 8]
    # 12-bit: t = c' << 4; c' = 0x123 -> i = 0x12, f = 0x30
    t = [1000 * i for i in range(66)] + [65536] * 191
    want = (t[0x12] * (256 - 0x30) + t[0x13] * 0x30 + 128) >> 8
    assert one((0x123, 0, 0), 12, tone=t, out16=True)[0] == want
    assert one((0x123, 0, 0), 12, tone=t)[0] == want >> 8


def test_sixteen_fold_gain_needs_more_than_32_bits():
    """the matrix sum of three 17-bit x 16-bit products passes 2^32: 32-bit accumulation, signed or not, is wrong"""
    m = (65535, 3, 0, 0, 4096, 0, 0, 0, 4096)
    rgb = (65535, 65535, 0)
    acc = 65535 * 65535 + 3 * 65535
    assert acc == (1 << 32) + 65534
    assert one(rgb, 16, matrix=m, out16=True)[0] == 65535
    wrapped_u32 = min(((acc & 0xFFFFFFFF) + 2048) >> 12, 65535)
    assert wrapped_u32 == 16                                # what uint32 accumulation would give
    acc2 = 65535 * 65535                                     # 15.9998 x 65535, one product alone
    as_i32 = acc2 - (1 << 32)
    assert as_i32 < 0                                       # what int32 accumulation would see: clamps to 0
    assert one((65535, 0, 0), 16, matrix=(65535, 0, 0, 0, 4096, 0, 0, 0, 4096), out16=True)[0] == 65535
    # the split the kernel uses is exact: m = hi * 4096 + lo, (acc + 2048) >> 12 = sum(hi v) + ((sum(lo v) + 2048) >> 12)
    rng = np.random.default_rng(1)
    mm_ = rng.integers(-65535, 65536, (2000, 3))
    v = rng.integers(0, 65536, (2000, 3))
    exact = ((mm_ * v).sum(axis=1) + 2048) >> 12
    hi, lo = mm_ >> 12, mm_ & 4095
    assert np.abs((hi * v).sum(axis=1)).max() < 1 << 31 and (lo * v).sum(axis=1).max() < 1 << 31
    assert np.array_equal((hi * v).sum(axis=1) + (((lo * v).sum(axis=1) + 2048) >> 12), exact)


def test_pack_layouts_and_byte_order():
    v = np.array([[[0x1122, 0x3344, 0x5566]]], np.int64)
    assert cm.pack(v, "ARGB64", True).tolist() == [[0xFF, 0xFF, 0x22, 0x11, 0x44, 0x33, 0x66, 0x55]]
    assert cm.pack(v, "BGRA64", True, dst_big_endian=True).tolist() == [[0x55, 0x66, 0x33, 0x44, 0x11, 0x22, 0xFF, 0xFF]]
    assert cm.pack(v >> 8, "xBGR", False).tolist() == [[0xFF, 0x55, 0x33, 0x11]]
