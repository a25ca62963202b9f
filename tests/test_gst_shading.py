"""GPU tests of bayer2rgb shading-file=...: a gst-launch pipeline over a 258 x 37 stream, compared byte for byte with the
CPU oracle applied to the model-shaded mosaic (tests/shading_model.py), and a file whose node count does not fit the
negotiated size, which must end in an element error."""
import os

import numpy as np
import pytest

import shading_model as shm
from test_gpu_shading import site_planes
from test_gst_colour import file_pipeline
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = [pytest.mark.gpu, needs_gst]

W, H, KX, KY = 258, 37, 5, 3
BLACK = (5, 9, 7, 3)


@pytest.mark.parametrize("extra", ["", "inflight=3 devices=0,0"])
def test_bayer2rgb_shading_file_equals_the_model(plugin, gpu_pkg, oracle, tmp_path, extra):
    n, stride = 3, 260
    src = np.full((n, H, stride), 0x5A, np.uint8)
    src[:, :, :W] = np.random.default_rng(258).integers(0, 256, (n, H, W))
    table = site_planes(W, H, KX, KY)
    path = os.path.join(str(tmp_path), "lens.mish")
    shm.write_file(path, KX, KY, table, BLACK)
    got = file_pipeline(tmp_path, src, W, H, "grbg", "BGRx", 4, ("shading-file=%s %s" % (path, extra)).strip(), "shade")
    r, g, b = gpu_pkg.FORMATS["BGRx"]
    for i in range(n):
        shaded = shm.shade_raw(src[i], table, KX, KY, BLACK, W, H, stride).reshape(H, stride)
        assert np.array_equal(got[i], oracle.bayer2rgb(shaded, W, "grbg", r, g, b)), (extra, i)
    # the default, spelled out: the reference's bytes
    plain = file_pipeline(tmp_path, src, W, H, "grbg", "BGRx", 4, 'shading-file=""', "plain")
    assert np.array_equal(plain[0], oracle.bayer2rgb(src[0], W, "grbg", r, g, b))


def test_a_file_of_the_wrong_node_count_is_an_element_error(plugin, gpu_pkg, tmp_path):
    src = np.zeros((1, H, 260), np.uint8)
    inp, outp = os.path.join(str(tmp_path), "in.raw"), os.path.join(str(tmp_path), "out.raw")
    src.tofile(inp)
    path = os.path.join(str(tmp_path), "other.mish")
    shm.write_file(path, KX, KY, site_planes(W + 64, H, KX, KY), BLACK)      # the table of a wider frame
    for bad in (path, os.path.join(str(tmp_path), "missing.mish"), inp):
        res = launch(tmp_path, "filesrc location=%s blocksize=%d ! video/x-bayer,format=grbg,width=%d,height=%d,framerate=1/1 "
                               "! bayer2rgb shading-file=%s ! video/x-raw,format=BGRx ! filesink location=%s"
                     % (inp, src[0].size, W, H, bad, outp))
        assert res.returncode != 0 and "shading-file" in res.stderr, (bad, res.stderr[-800:])
