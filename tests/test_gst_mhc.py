"""GPU tests of `method=mhc` on bayer2rgb and hipbayer2rgb: gst-launch pipelines compared byte for byte with the NumPy
model of tests/mhc_model.py, and the same pipelines without `method` still giving the reference's bytes."""
import os

import numpy as np
import pytest

import mhc_model as mm
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = [pytest.mark.gpu, needs_gst]


def file_pipeline(tmp, src, w, h, order, fmt, bpp, extra):
    inp = os.path.join(str(tmp), "in.raw")
    outp = os.path.join(str(tmp), "out_%s.raw" % extra.replace(" ", "_").replace("=", "-").replace(",", "-"))
    src.tofile(inp)
    res = launch(tmp, "filesrc location=%s blocksize=%d ! video/x-bayer,format=%s,width=%d,height=%d,framerate=1/1 "
                      "! bayer2rgb %s ! video/x-raw,format=%s ! filesink location=%s"
                 % (inp, src[0].size, order, w, h, extra, fmt, outp))
    assert res.returncode == 0, res.stderr[-1500:]
    assert "WARNING" not in res.stderr and "ERROR" not in res.stderr, res.stderr[-1500:]
    data = np.fromfile(outp, np.uint8)
    assert data.size == src.shape[0] * bpp * w * h
    return data.reshape(src.shape[0], h, bpp * w)


@pytest.mark.parametrize("extra", ["", "inflight=3", "inflight=3 devices=0,0"])
def test_bayer2rgb_640x480_sync_and_queued(plugin, gpu_pkg, oracle, tmp_path, extra):
    w, h, n = 640, 480, 5
    src = np.random.default_rng(640).integers(0, 256, (n, h, w), dtype=np.uint8)
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, ("method=mhc " + extra).strip())
    for i in range(n):
        assert np.array_equal(got[i], mm.bayer2rgb_mhc(src[i], w, h, "rggb", "BGRx")), (extra, i)
    # the same pipeline without `method` (and with method=bilinear) is still the reference's algorithm
    want = oracle.bayer2rgb_batch(src, w, "rggb", 2, 1, 0)
    for method in ("", "method=bilinear "):
        got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, (method + extra).strip() or "inflight=1")
        assert np.array_equal(got, want), (method, extra)


def test_bayer2rgb_deep_caps(plugin, gpu_pkg, tmp_path):
    w, h, n = 322, 50, 2
    rng = np.random.default_rng(12)
    src = np.stack([mm.pack(rng.integers(0, 1 << 16, (h, w))) for _ in range(n)])
    got = file_pipeline(tmp_path, src, w, h, "bggr12le", "ARGB64", 8, "method=mhc")
    for i in range(n):
        assert np.array_equal(got[i], mm.bayer2rgb_mhc(src[i], w, h, "bggr", "ARGB64", bits=12, out16=True)), i


def test_hipbayer2rgb_batch_4(plugin, gpu_pkg, oracle, tmp_path):
    """hipupload ! hipbayer2rgb method=mhc batch=4 ! hipdownload: 11 frames = two list launches of 4 and a tail at EOS"""
    w, h, n = 1280, 720, 11
    inp, outp, out2 = str(tmp_path / "in.raw"), str(tmp_path / "out.raw"), str(tmp_path / "out2.raw")
    res = launch(tmp_path,
                 "videotestsrc num-buffers=%d pattern=snow ! video/x-bayer,format=grbg,width=%d,height=%d,framerate=30/1 "
                 "! tee name=t t. ! queue ! filesink location=%s t. ! queue ! hipupload ! hipbayer2rgb method=mhc batch=4 "
                 "! hipdownload ! video/x-raw,format=xBGR ! filesink location=%s" % (n, w, h, inp, outp))
    assert res.returncode == 0, res.stderr[-2000:]
    src = np.fromfile(inp, np.uint8).reshape(n, h, w)
    got = np.fromfile(outp, np.uint8).reshape(n, h, 4 * w)
    for i in range(n):
        assert np.array_equal(got[i], mm.bayer2rgb_mhc(src[i], w, h, "grbg", "xBGR")), i
    # without `method`: the reference's bytes
    res = launch(tmp_path,
                 "filesrc location=%s blocksize=%d ! video/x-bayer,format=grbg,width=%d,height=%d,framerate=30/1 "
                 "! hipupload ! hipbayer2rgb batch=4 ! hipdownload ! video/x-raw,format=xBGR ! filesink location=%s"
                 % (inp, w * h, w, h, out2))
    assert res.returncode == 0, res.stderr[-2000:]
    assert np.array_equal(np.fromfile(out2, np.uint8).reshape(n, h, 4 * w),
                          oracle.bayer2rgb_batch(src, w, "grbg", 3, 2, 1, nthreads=4))
