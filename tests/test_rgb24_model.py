"""CPU tests of tests/rgb24_model.py: the model of packed 24-bit output is the 4-byte models' RGBx / BGRx frame with
byte 3 dropped, so on the committed fixtures of tests/golden/bayer2rgb_small.npz -- frames of the reference's own
functions -- its rows are the golden rows without their fourth bytes.  That is the pin to the reference; the model adds
layout only."""
import re

import numpy as np

import highbit_model as hm
import mhc_model as mm
import rgb24_model as rm


def golden_cases(golden):
    for key in golden.files:
        m = re.match(r"out_(\d+)x(\d+)_(\w+?)_(RGBx|BGRx)$", key)
        if m:
            yield key, int(m.group(1)), int(m.group(2)), m.group(3), m.group(4)[:3]


def test_model_rows_are_the_golden_rows_without_byte_3(golden):
    n = 0
    for key, w, h, pattern, fmt in golden_cases(golden):
        src = golden["in_%dx%d" % (w, h)]
        want4 = golden[key]
        assert want4.shape == (h, 4 * w) and (want4[:, 3::4] == 255).all()
        want = want4.reshape(h, w, 4)[:, :, :3].reshape(h, 3 * w)
        got = rm.bayer2rgb_rgb24(src, w, h, pattern, fmt, src_stride=src.shape[1])
        assert got.shape == (h, rm.default_stride(w))
        assert np.array_equal(got[:, :3 * w], want), key
        off = rm.OFFSETS[fmt]
        px = got[:, :3 * w].reshape(h, w, 3)
        four = want4.reshape(h, w, 4)
        assert all(np.array_equal(px[..., off[c]], four[..., off[c]]) for c in range(3))
        n += 1
    assert n >= 8, n                    # four Bayer orders x RGBx / BGRx at one size at least


def test_default_stride_and_padding_left_as_given(golden):
    assert [rm.default_stride(w) for w in (4, 6, 20, 22, 258, 2730)] == [12, 20, 60, 68, 776, 8192]
    key, w, h, pattern, fmt = next(c for c in golden_cases(golden) if c[1] % 4 == 2 or c[1] >= 6)
    src = golden["in_%dx%d" % (w, h)]
    plain = rm.bayer2rgb_rgb24(src, w, h, pattern, fmt, src_stride=src.shape[1])
    assert (plain[:, 3 * w:] == rm.GUARD).all()
    stride = rm.default_stride(w) + 8
    dst = np.arange(h * stride, dtype=np.uint32).astype(np.uint8).reshape(h, stride)
    out = rm.bayer2rgb_rgb24(src, w, h, pattern, fmt, src_stride=src.shape[1], dst_stride=stride, dst=dst)
    assert out.shape == (h, stride) and np.array_equal(out[:, 3 * w:], dst[:, 3 * w:])
    assert np.array_equal(out[:, :3 * w], plain[:, :3 * w])
    assert out is not dst and dst[0, 0] == 0      # the given frame itself is not written


def test_every_arm_is_its_four_byte_model_without_byte_3():
    """deep mosaics, MHC and the colour stage: no arithmetic of the model's own"""
    import colour_model as cm
    rng = np.random.default_rng(1)
    w, h = 22, 7
    S = rng.integers(0, 1 << 12, (h, w))
    buf = hm.pack(S)
    tone = tuple(min(65536, 300 * i) for i in range(257))
    stage = dict(black=(64, 64, 64), matrix=(5000, -300, 10, 0, 4096, 0, 7, -9, 6000), tone=tone)
    for fmt, four in rm.FOUR_BYTE.items():
        rows = {
            "deep": (hm.bayer2rgb_highbit(buf, w, h, "grbg", four, 12, False), {}),
            "mhc": (mm.bayer2rgb_mhc(buf, w, h, "grbg", four, bits=12), dict(method="mhc")),
            "colour": (cm.bayer2rgb_colour(buf, w, h, "grbg", four, bits=12, method="mhc", **stage),
                       dict(method="mhc", colour=stage)),
        }
        for name, (rows4, kw) in rows.items():
            got = rm.bayer2rgb_rgb24(buf, w, h, "grbg", fmt, bits=12, **kw)
            assert np.array_equal(got[:, :3 * w], rows4.reshape(h, w, 4)[:, :, :3].reshape(h, 3 * w)), (fmt, name)
            assert (got[:, 3 * w:] == rm.GUARD).all() and got.shape[1] == 68
