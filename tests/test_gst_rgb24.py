"""Packed 24-bit output through the elements: `hipbayer2rgb` offers `video/x-raw(memory:HIPMemory), format={RGB, BGR}`
as a second structure after its 4-byte formats and converts with MIBAYER_FLAG_DST_24BIT, offsets and stride from
GstVideoInfo (ROUND_UP_4 (3 w), passed to the library explicitly).  Pipelines on the real library against
tests/rgb24_model.py; the two bytes behind a width % 4 == 2 row are padding and are not compared.

`bayer2rgb` (the host-memory element) does not offer the formats: tests/test_highbit_abi.py pins the number of
`video/x-raw` structures of its src template."""
import re
import subprocess

import numpy as np
import pytest

import rgb24_model as rm
from test_gst_element import GST_INSPECT, gst_env, needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = needs_gst

FIRST_SRC = ("format: { (string)RGBx, (string)xRGB, (string)BGRx, (string)xBGR, (string)RGBA, "
             "(string)ARGB, (string)BGRA, (string)ABGR }")
SECOND_SRC = "format: { (string)RGB, (string)BGR }"


def inspect(tmp_path, what):
    return subprocess.run([GST_INSPECT, what], capture_output=True, text=True, env=gst_env(tmp_path),
                          timeout=120).stdout


def test_hipbayer2rgb_lists_the_new_structure_last(plugin, tmp_path):  # noqa: F811
    out = inspect(tmp_path, "hipbayer2rgb")
    assert FIRST_SRC in out and SECOND_SRC in out
    assert out.index(FIRST_SRC) < out.index(SECOND_SRC)            # default negotiation keeps landing on RGBx
    assert len(re.findall(r"^\s+video/x-raw\(memory:HIPMemory\)$", out, re.M)) == 2
    assert len(re.findall(r"^\s+video/x-bayer\(memory:HIPMemory\)$", out, re.M)) == 1
    assert out.count("Availability: Always") == 2
    # the sibling direction and the host-memory elements are what they were
    for other in ("hiprgb2bayer", "rgb2bayer", "bayer2rgb"):
        assert SECOND_SRC not in inspect(tmp_path, other), other


@pytest.mark.parametrize("fmt", ["RGB", "BGR"])
@pytest.mark.parametrize("props", ["", "batch=4", "method=mhc batch=2"])
def test_hipbayer2rgb_over_the_test_double_hands_the_stride_down(rig, tmp_path, fmt, props):  # noqa: F811
    """the element's own logic over tests/check/mock_mibayer.c: the 24-bit caps negotiate, buffers are
    ROUND_UP_4 (3 w) h bytes, every frame leaves once and in order.  The double defaults dst_stride to 4 w and fills
    dst_stride * h bytes per frame: were the stride of GstVideoInfo not passed down explicitly, it would write 4 w h
    bytes into each 776 h byte buffer, which the rig's sanitizer build reports"""
    w, h, n = 258, 18, 9
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=40).tofile(inp)
    pipe = ("hipupload ! hipbayer2rgb %s ! capsfilter caps=\"video/x-raw(memory:HIPMemory),format=%s\" ! hipdownload"
            % (props, fmt))
    kv = run(rig, "caps", pipe, B2R % ("grbg", w, h), 260 * h)
    assert kv["caps_accepted"] == "1" and kv["errors"] == "0", kv
    kv = run(rig, "convert", pipe, B2R % ("grbg", w, h), inp, 260 * h, outp)
    assert kv["pushed"] == str(n) and kv["pulled"] == str(n), kv
    seq, fill = stamps(outp, n, rm.default_stride(w) * h)
    assert fill == list(range(40, 40 + n)) and seq == list(range(n))
    # an odd geometry is refused at negotiation, as with 4-byte caps
    kv = run(rig, "caps", pipe, B2R % ("grbg", 63, h), 64 * h)
    assert kv["caps_accepted"] == "0", kv


def convert(tmp_path, w, h, n, order, fmt, props, caps_before_download=True):
    """videotestsrc mosaic -> file, and -> hipupload ! hipbayer2rgb ! hipdownload -> file; returns both"""
    inp, outp = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    device_caps = "! video/x-raw(memory:HIPMemory),format=%s ! hipdownload" % fmt
    host_caps = "! hipdownload ! video/x-raw,format=%s" % fmt
    res = launch(tmp_path,
                 "videotestsrc num-buffers=%d pattern=snow ! video/x-bayer,format=%s,width=%d,height=%d,framerate=30/1 "
                 "! tee name=t t. ! queue ! filesink location=%s t. ! queue ! hipupload ! hipbayer2rgb %s %s "
                 "! filesink location=%s" % (n, order, w, h, inp, props,
                                             device_caps if caps_before_download else host_caps, outp))
    assert res.returncode == 0, res.stderr[-3000:]
    sstride = (w + 3) & ~3
    src = np.fromfile(inp, np.uint8).reshape(n, h, sstride)
    got = np.fromfile(outp, np.uint8)
    return src, got


@pytest.mark.gpu
@pytest.mark.parametrize("fmt,order,props,before", [
    ("RGB", "grbg", "batch=4", True),           # list launches of 4 separately allocated frames, and the drained rest
    ("BGR", "bggr", "", True),                  # frame by frame
    ("BGR", "rggb", "batch=4 method=mhc", False),
    ("RGB", "gbrg", "method=mhc", False),
])
def test_hipbayer2rgb_converts_to_packed_24_bit(plugin, gpu_pkg, tmp_path, fmt, order, props, before):  # noqa: F811
    w, h, n = 258, 18, 9
    src, got = convert(tmp_path, w, h, n, order, fmt, props, before)
    stride = rm.default_stride(w)
    assert stride == 776 and got.size == n * stride * h            # GstVideoInfo's size of RGB / BGR: ROUND_UP_4 (3 w) h
    got = got.reshape(n, h, stride)
    method = "mhc" if "mhc" in props else "bilinear"
    for f in range(n):
        want = rm.bayer2rgb_rgb24(src[f], w, h, order, fmt, method=method, src_stride=src.shape[2])
        assert np.array_equal(got[f][:, :3 * w], want[:, :3 * w]), (fmt, order, props, f)


@pytest.mark.gpu
def test_hipbayer2rgb_width_on_the_grid_and_default_negotiation(plugin, gpu_pkg, oracle, tmp_path):  # noqa: F811
    """width % 4 == 0: no padding, every byte of the file is the model's; and with nothing asked for downstream the
    element still lands on RGBx, 4 bytes per pixel, the oracle's bytes"""
    w, h, n = 260, 17, 3
    src, got = convert(tmp_path, w, h, n, "bggr", "BGR", "batch=2")
    assert got.size == n * 3 * w * h
    got = got.reshape(n, h, 3 * w)
    for f in range(n):
        assert np.array_equal(got[f], rm.bayer2rgb_rgb24(src[f], w, h, "bggr", "BGR", src_stride=w)), f
    inp, outp = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    res = launch(tmp_path,
                 "videotestsrc num-buffers=2 pattern=snow ! video/x-bayer,format=bggr,width=%d,height=%d,framerate=30/1 "
                 "! tee name=t t. ! queue ! filesink location=%s t. ! queue ! hipupload ! hipbayer2rgb ! hipdownload "
                 "! filesink location=%s" % (w, h, inp, outp))
    assert res.returncode == 0, res.stderr[-3000:]
    src = np.fromfile(inp, np.uint8).reshape(2, h, w)
    got = np.fromfile(outp, np.uint8)
    assert got.size == 2 * 4 * w * h
    assert np.array_equal(got.reshape(2, h, 4 * w), oracle.bayer2rgb_batch(src, w, "bggr", 0, 1, 2))
