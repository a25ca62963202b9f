"""`method=half` on bayer2rgb: the property (CPU), and gst-launch pipelines compared byte for byte with the NumPy model
of tests/half_model.py (GPU).  The element's caps scale with the method: the raw side is width / 2 x height >> 1 of the
bayer side, and anything else is not-negotiated."""
import os
import subprocess

import numpy as np
import pytest

import half_model as hf
from test_gst_element import GST_INSPECT, gst_env, needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = needs_gst

W, H, N = 258, 37, 3
OW, OH = 129, 18
SRC_STRIDE = 260


@pytest.fixture(scope="module")
def mosaics(tmp_path_factory):
    """three frames as filesrc reads them: rows padded to a multiple of four bytes"""
    rng = np.random.default_rng(258)
    src = np.full((N, H, SRC_STRIDE), 0x5A, np.uint8)
    src[:, :, :W] = rng.integers(0, 256, (N, H, W), dtype=np.uint8)
    path = str(tmp_path_factory.mktemp("half") / "in.raw")
    src.tofile(path)
    return src, path


def pipeline(inp, outp, raw_caps, extra="method=half"):
    return ("filesrc location=%s blocksize=%d ! video/x-bayer,format=rggb,width=%d,height=%d,framerate=1/1 "
            "! bayer2rgb %s ! %s ! filesink location=%s" % (inp, SRC_STRIDE * H, W, H, extra, raw_caps, outp))


def test_inspect_lists_the_method(plugin, tmp_path):
    out = subprocess.run([GST_INSPECT, "bayer2rgb"], capture_output=True, text=True, env=gst_env(tmp_path),
                         timeout=120).stdout
    at = out.index("method ")
    block = out[at:at + 1500]
    for nick in ("bilinear", "mhc", "half"):
        assert "(%d): %s" % (("bilinear", "mhc", "half").index(nick), nick) in block, block
    assert "Default: 0, \"bilinear\"" in block
    # hipbayer2rgb keeps its two methods
    hip = subprocess.run([GST_INSPECT, "hipbayer2rgb"], capture_output=True, text=True, env=gst_env(tmp_path),
                         timeout=120).stdout
    if "method " in hip:
        assert "(2): half" not in hip


@pytest.mark.gpu
def test_258x37_rggb_to_bgrx_is_129x18_and_the_models_bytes(plugin, gpu_pkg, mosaics, tmp_path):
    src, inp = mosaics
    outp = str(tmp_path / "out.raw")
    res = launch(tmp_path, pipeline(inp, outp, "video/x-raw,format=BGRx"))
    assert res.returncode == 0, res.stderr[-1500:]
    assert "WARNING" not in res.stderr and "ERROR" not in res.stderr, res.stderr[-1500:]
    data = np.fromfile(outp, np.uint8)
    assert data.size == N * OW * OH * 4
    got = data.reshape(N, OH, 4 * OW)
    for i in range(N):
        want = hf.frame(src[i], W, H, "rggb", "BGRx", src_stride=SRC_STRIDE)
        assert np.array_equal(got[i], want), i
    # the size spelled out downstream negotiates to the same bytes
    out2 = str(tmp_path / "out2.raw")
    res = launch(tmp_path, pipeline(inp, out2, "video/x-raw,format=BGRx,width=%d,height=%d" % (OW, OH)))
    assert res.returncode == 0, res.stderr[-1500:]
    assert np.array_equal(np.fromfile(out2, np.uint8), data)


@pytest.mark.gpu
def test_a_downstream_width_of_128_fails_to_negotiate(plugin, gpu_pkg, mosaics, tmp_path):
    src, inp = mosaics
    outp = str(tmp_path / "out.raw")
    res = launch(tmp_path, pipeline(inp, outp, "video/x-raw,format=BGRx,width=128"))
    assert res.returncode != 0
    said = res.stderr + res.stdout      # refused when the caps filter is linked, or by set_caps at the first buffer
    assert "can't handle caps" in said or "not-negotiated" in said, said[-1500:]
    assert not os.path.exists(outp) or os.path.getsize(outp) == 0
    # ... and so does the mosaic's own size: the default method's caps are not the half method's
    res = launch(tmp_path, pipeline(inp, outp, "video/x-raw,format=BGRx,width=%d,height=%d" % (W, H)))
    assert res.returncode != 0
    # while the default method still converts at full size
    full = str(tmp_path / "full.raw")
    res = launch(tmp_path, pipeline(inp, full, "video/x-raw,format=BGRx,width=%d,height=%d" % (W, H), extra=""))
    assert res.returncode == 0, res.stderr[-1500:]
    assert os.path.getsize(full) == N * W * H * 4
