"""GPU tests of the colour-stage properties of bayer2rgb and hipbayer2rgb: gst-launch pipelines with gains, a ccm and
tone-curve=srgb compared byte for byte with the NumPy model of tests/colour_model.py (matrix and tone table from the
library's helpers, as the elements build them), and the same pipelines with default properties still giving the
reference's recorded bytes."""
import hashlib
import os

import numpy as np
import pytest

import colour_model as cm
import highbit_model as hm
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = [pytest.mark.gpu, needs_gst]

GAINS = (1.85, 1.0, 1.4)
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)
PROPS = "black-level=%d red-gain=1.85 blue-gain=1.4 ccm=" + ",".join("%g" % v for v in CCM) + " tone-curve=srgb"


def stage(pkg, black):
    return dict(black=(black,) * 3, matrix=pkg.colour_matrix(GAINS, CCM), tone=pkg.colour_tone(pkg.TONE_SRGB))


def file_pipeline(tmp, src, w, h, order, fmt, bpp, extra, tag):
    inp = os.path.join(str(tmp), "in_%s.raw" % tag)
    outp = os.path.join(str(tmp), "out_%s.raw" % tag)
    src.tofile(inp)
    res = launch(tmp, "filesrc location=%s blocksize=%d ! video/x-bayer,format=%s,width=%d,height=%d,framerate=1/1 "
                      "! bayer2rgb %s ! video/x-raw,format=%s ! filesink location=%s"
                 % (inp, src[0].size, order, w, h, extra, fmt, outp))
    assert res.returncode == 0, res.stderr[-1500:]
    assert "WARNING" not in res.stderr and "ERROR" not in res.stderr, res.stderr[-1500:]
    data = np.fromfile(outp, np.uint8)
    assert data.size == src.shape[0] * bpp * w * h
    return data.reshape(src.shape[0], h, bpp * w)


@pytest.mark.parametrize("extra", ["", "method=mhc", "inflight=3 devices=0,0"])
def test_bayer2rgb_8bit(plugin, gpu_pkg, tmp_path, extra):
    w, h, n = 640, 480, 4
    src = np.random.default_rng(640).integers(0, 256, (n, h, w), dtype=np.uint8)
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, (PROPS % 16 + " " + extra).strip(), "c8")
    method = "mhc" if "mhc" in extra else "bilinear"
    for i in range(n):
        want = cm.bayer2rgb_colour(src[i], w, h, "rggb", "BGRx", method=method, **stage(gpu_pkg, 16))
        assert np.array_equal(got[i], want), (extra, i)


@pytest.mark.parametrize("fmt,out16", [("ARGB64", True), ("BGRx", False)])
def test_bayer2rgb_12bit(plugin, gpu_pkg, tmp_path, fmt, out16):
    w, h, n = 322, 50, 2
    rng = np.random.default_rng(12)
    src = np.stack([hm.pack(rng.integers(0, 1 << 16, (h, w))) for _ in range(n)])
    for method in ("bilinear", "mhc"):
        got = file_pipeline(tmp_path, src, w, h, "bggr12le", fmt, 8 if out16 else 4,
                            PROPS % 256 + " method=" + method, "c12" + method)
        for i in range(n):
            want = cm.bayer2rgb_colour(src[i], w, h, "bggr", fmt, bits=12, out16=out16, method=method,
                                       **stage(gpu_pkg, 256))
            assert np.array_equal(got[i], want), (fmt, method, i)


def test_gamma_curve_and_a_bad_ccm(plugin, gpu_pkg, tmp_path):
    w, h = 66, 20
    src = np.random.default_rng(3).integers(0, 256, (1, h, (w + 3) & ~3), dtype=np.uint8)
    got = file_pipeline(tmp_path, src, w, h, "gbrg", "xRGB", 4, "tone-curve=gamma gamma=1.8", "gam")
    want = cm.bayer2rgb_colour(src[0], w, h, "gbrg", "xRGB", stride=src.shape[2],
                               tone=gpu_pkg.colour_tone(gpu_pkg.TONE_GAMMA, 1.8))
    assert np.array_equal(got[0], want)
    inp = str(tmp_path / "in_gam.raw")
    for bad in ("ccm=1,2,3", "ccm=1,0,0,0,1,0,0,0,x", "red-gain=15 ccm=2,0,0,0,1,0,0,0,1"):
        res = launch(tmp_path, "filesrc location=%s blocksize=%d ! video/x-bayer,format=gbrg,width=%d,height=%d,"
                               "framerate=1/1 ! bayer2rgb %s ! fakesink" % (inp, src[0].size, w, h, bad))
        assert res.returncode != 0 and "colour stage" in res.stderr, (bad, res.stderr[-800:])


def test_hipbayer2rgb(plugin, gpu_pkg, oracle, tmp_path):
    """hipupload ! hipbayer2rgb <colour properties> batch=4 ! hipdownload, both methods; without them the reference.
    8-bit only: hipbayer2rgb's caps have no deep mosaics, so the 12-bit pipelines are bayer2rgb's (above)."""
    w, h, n = 1280, 720, 6
    inp = str(tmp_path / "in.raw")
    src = np.random.default_rng(7).integers(0, 256, (n, h, w), dtype=np.uint8)
    src.tofile(inp)
    for extra, method in ((PROPS % 16, "bilinear"), (PROPS % 16 + " method=mhc", "mhc"), ("", None)):
        outp = str(tmp_path / ("out_%s.raw" % method))
        res = launch(tmp_path,
                     "filesrc location=%s blocksize=%d ! video/x-bayer,format=grbg,width=%d,height=%d,framerate=30/1 "
                     "! hipupload ! hipbayer2rgb %s batch=4 ! hipdownload ! video/x-raw,format=xBGR ! filesink location=%s"
                     % (inp, w * h, w, h, extra, outp))
        assert res.returncode == 0, res.stderr[-2000:]
        got = np.fromfile(outp, np.uint8).reshape(n, h, 4 * w)
        if method is None:
            assert np.array_equal(got, oracle.bayer2rgb_batch(src, w, "grbg", 3, 2, 1, nthreads=4))
            continue
        for i in range(n):
            want = cm.bayer2rgb_colour(src[i], w, h, "grbg", "xBGR", method=method, **stage(gpu_pkg, 16))
            assert np.array_equal(got[i], want), (method, i)


def test_default_properties_give_the_recorded_reference_bytes(plugin, gpu_pkg, oracle, tmp_path):
    """every colour property at its default, spelled out: the flag is not set, the md5s are the reference element's
    (64x48 seed 7 default caps, 1920x1080 seed 1 rggb -> BGRx)"""
    defaults = "black-level=0 red-gain=1 green-gain=1 blue-gain=1 ccm=\"\" tone-curve=linear gamma=2.2"
    for (w, h, seed, order, fmt, md5) in ((64, 48, 7, "bggr", "RGBx", "5e213c796b18997f2a81d54aee9afcd8"),
                                          (1920, 1080, 1, "rggb", "BGRx", "f14f6ad248ef0bac0f28546db6d14813")):
        src = oracle.fill_synthetic(w, h, 1, seed=seed)
        for extra in ("", defaults, defaults.replace("gamma=2.2", "gamma=3")):
            got = file_pipeline(tmp_path, src, w, h, order, fmt, 4, extra, "def%d" % w)
            assert hashlib.md5(got[0].tobytes()).hexdigest() == md5, (w, extra)
