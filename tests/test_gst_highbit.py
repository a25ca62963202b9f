"""GPU tests of the bayer2rgb element on deep mosaics (its second caps structures): gst-launch pipelines and the
GstHarness driver, every output compared with the NumPy model of tests/highbit_model.py."""
import os

import numpy as np
import pytest

import highbit_model as hm
from test_gst_element import launch, needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_harness import CAPS, harness, run  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, needs_gst]


def frames(seed, w, h, n, bits, big_endian=False):
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        words = rng.integers(0, 1 << 16, (h, w))             # the bits above `bits` must be ignored
        out.append(hm.pack(words, big_endian=big_endian))
    return np.stack(out)


def file_pipeline(tmp, src, w, h, order, fmt, bpp, extra=""):
    inp, outp = os.path.join(str(tmp), "in.raw"), os.path.join(str(tmp), "out_%s_%s.raw" % (order, fmt))
    src.tofile(inp)
    res = launch(tmp, "filesrc location=%s blocksize=%d ! video/x-bayer,format=%s,width=%d,height=%d,framerate=1/1 "
                      "! bayer2rgb %s ! video/x-raw,format=%s ! filesink location=%s"
                 % (inp, src[0].size, order, w, h, extra, fmt, outp))
    assert res.returncode == 0, res.stderr[-1500:]
    assert "WARNING" not in res.stderr and "ERROR" not in res.stderr, res.stderr[-1500:]
    data = np.fromfile(outp, np.uint8)
    assert data.size == src.shape[0] * bpp * w * h
    return data.reshape(src.shape[0], h, bpp * w)


@pytest.mark.parametrize("fmt,out16", [("ARGB64", True), ("BGRx", False)])
def test_bggr12le_pipeline(plugin, gpu_pkg, tmp_path, fmt, out16):
    w, h = 322, 50
    src = frames(12, w, h, 2, 12)
    got = file_pipeline(tmp_path, src, w, h, "bggr12le", fmt, 8 if out16 else 4)
    for i in range(2):
        assert np.array_equal(got[i], hm.bayer2rgb_highbit(src[i], w, h, "bggr", fmt, 12, out16)), (fmt, i)


def test_rggb16be_640x480(plugin, gpu_pkg, tmp_path):
    w, h = 640, 480
    src = frames(16, w, h, 1, 16, big_endian=True)
    for fmt, out16 in (("ARGB64", True), ("RGBx", False)):
        got = file_pipeline(tmp_path, src, w, h, "rggb16be", fmt, 8 if out16 else 4)
        assert np.array_equal(got[0], hm.bayer2rgb_highbit(src[0], w, h, "rggb", fmt, 16, out16, src_big_endian=True))


def test_queued_mode_on_two_shards(plugin, gpu_pkg, tmp_path):
    w, h, n = 642, 36, 9
    src = frames(10, w, h, n, 10)
    got = file_pipeline(tmp_path, src, w, h, "gbrg10le", "ARGB64", 8, extra="inflight=3 devices=0,0")
    for i in range(n):
        assert np.array_equal(got[i], hm.bayer2rgb_highbit(src[i], w, h, "gbrg", "ARGB64", 10, True)), i


def test_switch_from_8bit_to_10bit_mid_stream(plugin, gpu_pkg, harness, tmp_path):
    """bggr -> bggr10le while the stream runs (default output RGBx both times): the frames in flight under the 8-bit
    caps come out first, the pool is rebuilt for 16-bit words, every frame of both halves converted in order"""
    w, h, n1, n2 = 66, 20, 5, 4
    rng = np.random.default_rng(8)
    a = rng.integers(0, 256, (n1, h, (w + 3) & ~3), dtype=np.uint8)
    b = frames(11, w, h, n2, 10)
    fa, fb, outp = tmp_path / "a.raw", tmp_path / "b.raw", tmp_path / "out.raw"
    a.tofile(fa)
    b.tofile(fb)
    kv = run(harness, tmp_path, "renegotiate", "bayer2rgb inflight=3", CAPS % ("bggr", w, h), fa, a[0].size,
             CAPS % ("bggr10le", w, h), fb, b[0].size, outp)
    assert kv["pushed"] == str(n1 + n2) and kv["pulled"] == str(n1 + n2)
    got = np.fromfile(outp, np.uint8).reshape(n1 + n2, h, 4 * w)
    for i in range(n1):
        want = hm.bayer2rgb_highbit(a[i], w, h, "bggr", "RGBx", 8, False, stride=(w + 3) & ~3)
        assert np.array_equal(got[i], want), ("8-bit", i)
    for i in range(n2):
        assert np.array_equal(got[n1 + i], hm.bayer2rgb_highbit(b[i], w, h, "bggr", "RGBx", 10, False)), ("10-bit", i)
