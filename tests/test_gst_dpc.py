"""GPU tests of bayer2rgb dpc-hot-threshold / dpc-cold-threshold / defect-file: a gst-launch pipeline over a 258 x 37
stream, compared byte for byte with the CPU oracle applied to the model-corrected mosaic (tests/dpc_model.py), and
lists that cannot be used, which must end in an element error."""
import os

import numpy as np
import pytest

import dpc_model as dm
from test_gst_colour import file_pipeline
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = [pytest.mark.gpu, needs_gst]

W, H = 258, 37
LIST = "# a comment\n\n0 0\n257 36   # the last pixel\n  100\t17\n4 20\n0 0\n"


@pytest.mark.parametrize("extra", ["", "inflight=3 devices=0,0"])
def test_bayer2rgb_dpc_equals_the_model(plugin, gpu_pkg, oracle, tmp_path, extra):
    n, stride = 3, 260
    src = np.full((n, H, stride), 0x5A, np.uint8)
    src[:, :, :W] = np.random.default_rng(2580).integers(0, 256, (n, H, W))
    path = os.path.join(str(tmp_path), "defects.txt")
    open(path, "w").write(LIST)
    lst = dm.read_defect_file(path)
    assert len(lst) == 5
    r, g, b = gpu_pkg.FORMATS["BGRx"]
    for k, (hot, cold, use_list) in enumerate(((40, 25, True), (-1, -1, True), (0, -1, False))):
        props = "dpc-hot-threshold=%d dpc-cold-threshold=%d %s %s" % (hot, cold, "defect-file=%s" % path if use_list else "", extra)
        got = file_pipeline(tmp_path, src, W, H, "grbg", "BGRx", 4, " ".join(props.split()), "dpc%d" % k)
        for i in range(n):
            fixed = dm.correct_raw(src[i], src[i], W, H, stride, 0, False, hot, cold, lst if use_list else None).reshape(H, stride)
            assert not np.array_equal(fixed, src[i])
            assert np.array_equal(got[i], oracle.bayer2rgb(fixed, W, "grbg", r, g, b)), (extra, k, i)
    # the defaults, spelled out: the reference's bytes
    plain = file_pipeline(tmp_path, src, W, H, "grbg", "BGRx", 4, 'dpc-hot-threshold=-1 dpc-cold-threshold=-1 defect-file=""', "plain")
    assert np.array_equal(plain[0], oracle.bayer2rgb(src[0], W, "grbg", r, g, b))


def test_a_list_that_cannot_be_used_is_an_element_error(plugin, gpu_pkg, tmp_path):
    src = np.zeros((1, H, 260), np.uint8)
    inp, outp = os.path.join(str(tmp_path), "in.raw"), os.path.join(str(tmp_path), "out.raw")
    src.tofile(inp)
    outside, junk = os.path.join(str(tmp_path), "outside.txt"), os.path.join(str(tmp_path), "junk.txt")
    open(outside, "w").write("3 4\n0 37\n")
    open(junk, "w").write("3 4\n5\n")
    for bad in ("defect-file=%s" % outside, "defect-file=%s" % junk, "defect-file=%s" % os.path.join(str(tmp_path), "missing.txt"),
                "dpc-hot-threshold=256"):
        res = launch(tmp_path, "filesrc location=%s blocksize=%d ! video/x-bayer,format=grbg,width=%d,height=%d,framerate=1/1 "
                               "! bayer2rgb %s ! video/x-raw,format=BGRx ! filesink location=%s"
                     % (inp, src[0].size, W, H, bad, outp))
        assert res.returncode != 0 and "defective pixel correction" in res.stderr, (bad, res.stderr[-800:])
