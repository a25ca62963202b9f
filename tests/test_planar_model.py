"""CPU tests of tests/planar_model.py: the model of planar output deals the bytes of the 4-byte models' RGBx frame to
three planes, so on the committed fixtures of tests/golden/bayer2rgb_small.npz -- frames of the reference's own
functions -- its planes, put together again, are the golden RGBx frames.  That is the pin to the reference; the model
adds layout only."""
import re

import numpy as np

import highbit_model as hm
import mhc_model as mm
import planar_model as pm


def golden_cases(golden):
    for key in golden.files:
        m = re.match(r"out_(\d+)x(\d+)_(\w+?)_RGBx$", key)
        if m:
            yield key, int(m.group(1)), int(m.group(2)), m.group(3)


def test_planes_put_together_again_are_the_golden_rgbx_frame(golden):
    n = 0
    for key, w, h, pattern in golden_cases(golden):
        src = golden["in_%dx%d" % (w, h)]
        want4 = golden[key]
        assert want4.shape == (h, 4 * w) and (want4[:, 3::4] == 255).all()
        for fmt in pm.FORMATS:
            got = pm.bayer2rgb_planar(src, w, h, pattern, fmt, src_stride=src.shape[1])
            assert got.shape == (3, h, pm.default_stride(w))
            assert np.array_equal(pm.interleave(got, w, fmt), want4), (key, fmt)
        n += 1
    assert n >= 4, n                    # four Bayer orders at one size at least


def test_six_permutations_differ_in_plane_order_only(golden):
    key, w, h, pattern = next(golden_cases(golden))
    src = golden["in_%dx%d" % (w, h)]
    rgbp = pm.bayer2rgb_planar(src, w, h, pattern, "RGBP", src_stride=src.shape[1])
    assert len(set(pm.PERMUTATIONS)) == 6 and set(pm.FORMATS.values()) <= set(pm.PERMUTATIONS)
    for off in pm.PERMUTATIONS:
        got = pm.bayer2rgb_planar(src, w, h, pattern, off, src_stride=src.shape[1])
        for c in range(3):              # plane off[c] holds channel c, which RGBP has in plane c
            assert np.array_equal(got[off[c]], rgbp[c]), (off, c)
    assert np.array_equal(pm.bayer2rgb_planar(src, w, h, pattern, "GBR", src_stride=src.shape[1])[0], rgbp[1])


def test_default_stride_and_padding_left_as_given():
    assert [pm.default_stride(w) for w in (4, 6, 20, 22, 258, 2730)] == [4, 8, 20, 24, 260, 2732]
    rng = np.random.default_rng(2)
    w, h = 22, 7
    src = rng.integers(0, 256, (h, w), dtype=np.uint8)
    plain = pm.bayer2rgb_planar(src, w, h, "rggb", "BGRP")
    assert plain.shape == (3, h, 24) and (plain[:, :, w:] == pm.GUARD).all()    # width % 4 == 2: two guard bytes a row
    stride = 32
    dst = np.arange(3 * h * stride, dtype=np.uint32).astype(np.uint8).reshape(3, h, stride)
    out = pm.bayer2rgb_planar(src, w, h, "rggb", "BGRP", dst_stride=stride, dst=dst)
    assert out.shape == (3, h, stride) and np.array_equal(out[:, :, w:], dst[:, :, w:])
    assert np.array_equal(out[:, :, :w], plain[:, :, :w])
    assert out is not dst and dst[0, 0, 0] == 0           # the given frame itself is not written


def test_every_arm_is_its_four_byte_model_dealt_to_planes():
    """deep mosaics, MHC and the colour stage: no arithmetic of the model's own"""
    import colour_model as cm
    rng = np.random.default_rng(1)
    w, h = 22, 7
    S = rng.integers(0, 1 << 12, (h, w))
    buf = hm.pack(S)
    tone = tuple(min(65536, 300 * i) for i in range(257))
    stage = dict(black=(64, 64, 64), matrix=(5000, -300, 10, 0, 4096, 0, 7, -9, 6000), tone=tone)
    rows = {
        "deep": (hm.bayer2rgb_highbit(buf, w, h, "grbg", "RGBx", 12, False), {}),
        "mhc": (mm.bayer2rgb_mhc(buf, w, h, "grbg", "RGBx", bits=12), dict(method="mhc")),
        "colour": (cm.bayer2rgb_colour(buf, w, h, "grbg", "RGBx", bits=12, method="mhc", **stage),
                   dict(method="mhc", colour=stage)),
    }
    for name, (rows4, kw) in rows.items():
        px = rows4.reshape(h, w, 4)
        for fmt, off in pm.FORMATS.items():
            got = pm.bayer2rgb_planar(buf, w, h, "grbg", fmt, bits=12, **kw)
            assert got.shape == (3, h, 24) and (got[:, :, w:] == pm.GUARD).all()
            for c in range(3):
                assert np.array_equal(got[off[c], :, :w], px[:, :, c]), (name, fmt, c)
