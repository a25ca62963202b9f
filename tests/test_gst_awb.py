"""GPU tests of white-balance=grey-world on bayer2rgb and hipbayer2rgb: gst-launch pipelines over identical frames with
a strong colour cast and awb-speed=1, compared byte for byte with the colour model (tests/colour_model.py) under the
gains the loop must hold: the red-gain / blue-gain properties for the first frame, green-gain x the grey-world gains
of the frame (tests/stats_model.py, 1 x 1 zones, lo = max(black-level, 1), hi = 255 - (255 >> 4)) once a measurement
has been used.  One test runs the loop below awb-speed=1 (0.5, and the default 0.25) and follows every step of it.
white-balance=manual, spelled out, still gives the reference's recorded bytes."""
import hashlib

import numpy as np
import pytest

import colour_model as cm
import stats_model as sm
from test_gst_colour import file_pipeline
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = [pytest.mark.gpu, needs_gst]

BLACK, MANUAL = 8, (1.25, 1.0, 0.75)
PROPS = "black-level=%d red-gain=%g blue-gain=%g white-balance=grey-world awb-speed=1" % (BLACK, MANUAL[0], MANUAL[2])


def cast_frames(w, h, n, seed):
    """n copies of one rggb frame whose red sites are at half and whose blue sites at three quarters of the greens"""
    f = np.random.default_rng(seed).integers(24, 232, (h, w)).astype(np.float64)
    f[0::2, 0::2] *= 0.5
    f[1::2, 1::2] *= 0.75
    return np.repeat(f.astype(np.uint8)[None], n, axis=0)


def models(pkg, frame, w, h, fmt):
    """(output under the manual gains, output under the grey-world gains of the frame)"""
    zones = sm.zone_stats(sm.samples(frame, w, h, w), 1, 1, max(BLACK, 1), 255 - (255 >> 4))
    ok, gw = sm.grey_world(zones, "rggb", (BLACK,) * 3)
    assert ok == 1 and gw[0] > 1.5 and gw[2] > 1.2          # the cast is there
    out = [cm.bayer2rgb_colour(frame, w, h, "rggb", fmt, black=(BLACK,) * 3, matrix=pkg.colour_matrix(g, None))
           for g in (MANUAL, (MANUAL[1] * gw[0], MANUAL[1], MANUAL[1] * gw[2]))]
    assert not np.array_equal(out[0], out[1])
    return out


def test_bayer2rgb_synchronous_follows_every_frame(plugin, gpu_pkg, tmp_path):
    w, h, n = 320, 50, 4
    src = cast_frames(w, h, n, 1)
    manual, grey = models(gpu_pkg, src[0], w, h, "BGRx")
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, PROPS, "awb")
    assert np.array_equal(got[0], manual)
    for i in range(1, n):
        assert np.array_equal(got[i], grey), i


@pytest.mark.parametrize("speed", [0.5, None], ids=["0.5", "default"])
def test_bayer2rgb_synchronous_moves_by_awb_speed(plugin, gpu_pkg, tmp_path, speed):
    """awb-speed below 1 (None: the property left out, 0.25): frame 0 under the manual gains, frame i under
    g_i = g_(i-1) + s (green_gain x gw - g_(i-1)), in doubles and in the operation order of gst_mi_awb_step"""
    w, h, n = 320, 50, 5
    src = cast_frames(w, h, n, 1)
    s = 0.25 if speed is None else speed
    props = PROPS.replace(" awb-speed=1", "" if speed is None else " awb-speed=%g" % speed)
    assert ("awb-speed" in props) == (speed is not None) and "grey-world" in props
    zones = sm.zone_stats(sm.samples(src[0], w, h, w), 1, 1, max(BLACK, 1), 255 - (255 >> 4))
    ok, gw = sm.grey_world(zones, "rggb", (BLACK,) * 3)
    assert ok == 1
    gains = [(MANUAL[0], MANUAL[2])]
    for _ in range(1, n):
        gains.append(tuple(min(max(g + s * (MANUAL[1] * gw[2 * k] - g), 0.0), 15.99) for k, g in enumerate(gains[-1])))
    # the quantised matrix of every step does not hang on the last bit of a gain
    matrices = [gpu_pkg.colour_matrix((r, MANUAL[1], b), None) for r, b in gains]
    for (r, b), m in zip(gains, matrices):
        for r2 in (np.nextafter(r, -np.inf), np.nextafter(r, np.inf)):
            for b2 in (np.nextafter(b, -np.inf), np.nextafter(b, np.inf)):
                assert gpu_pkg.colour_matrix((float(r2), MANUAL[1], float(b2)), None) == m
    want = [cm.bayer2rgb_colour(src[0], w, h, "rggb", "BGRx", black=(BLACK,) * 3, matrix=m) for m in matrices]
    assert all(not np.array_equal(want[i], want[j]) for i in range(n) for j in range(i))    # the loop cannot be frozen
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, props, "awbs")
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i


def test_bayer2rgb_queued_converges(plugin, gpu_pkg, tmp_path):
    w, h, n = 320, 50, 12
    src = cast_frames(w, h, n, 2)
    manual, grey = models(gpu_pkg, src[0], w, h, "RGBx")
    got = file_pipeline(tmp_path, src, w, h, "rggb", "RGBx", 4, PROPS + " inflight=3 devices=0,0", "awbq")
    assert np.array_equal(got[0], manual) and np.array_equal(got[n - 1], grey)


def test_hipbayer2rgb_batch_converges(plugin, gpu_pkg, tmp_path):
    w, h, n = 640, 480, 12
    src = cast_frames(w, h, n, 3)
    manual, grey = models(gpu_pkg, src[0], w, h, "xBGR")
    inp, outp = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    src.tofile(inp)
    res = launch(tmp_path,
                 "filesrc location=%s blocksize=%d ! video/x-bayer,format=rggb,width=%d,height=%d,framerate=30/1 "
                 "! hipupload ! hipbayer2rgb %s batch=4 ! hipdownload ! video/x-raw,format=xBGR ! filesink location=%s"
                 % (inp, w * h, w, h, PROPS, outp))
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.fromfile(outp, np.uint8).reshape(n, h, 4 * w)
    assert np.array_equal(got[0], manual) and np.array_equal(got[n - 1], grey)


def test_manual_spelled_out_gives_the_recorded_reference_bytes(plugin, gpu_pkg, oracle, tmp_path):
    """the md5s of tests/test_gst_colour.py: the flag is not set, awb-speed alone changes nothing"""
    for (w, h, seed, order, fmt, md5) in ((64, 48, 7, "bggr", "RGBx", "5e213c796b18997f2a81d54aee9afcd8"),
                                          (1920, 1080, 1, "rggb", "BGRx", "f14f6ad248ef0bac0f28546db6d14813")):
        src = oracle.fill_synthetic(w, h, 1, seed=seed)
        for extra in ("white-balance=manual", "white-balance=manual awb-speed=1"):
            got = file_pipeline(tmp_path, src, w, h, order, fmt, 4, extra, "man%d" % w)
            assert hashlib.md5(got[0].tobytes()).hexdigest() == md5, (w, extra)
