"""GPU tests of exposure=auto on bayer2rgb and hipbayer2rgb: gst-launch pipelines over identical dark frames, compared
byte for byte with the colour model (tests/colour_model.py) under the gains the loop must hold: the gain properties for
the first frame, then gain_k x e with e += ae-speed x (x - e), x the exposure factor of the frame's whole-frame histogram
(tests/hist_model.py: 99th percentile, black-level, the gains before e, ae-target, ae-max-gain) once a measurement has
been used.  exposure=manual, spelled out, still gives the reference's recorded bytes."""
import hashlib

import numpy as np
import pytest

import colour_model as cm
import hist_model as hm
import stats_model as sm
from test_gst_colour import file_pipeline
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

pytestmark = [pytest.mark.gpu, needs_gst]

BLACK, MANUAL, TARGET, MAX_GAIN = 8, (1.25, 1.0, 0.75), 0.9, 4.0
PROPS = "black-level=%d red-gain=%g blue-gain=%g exposure=auto ae-speed=1" % (BLACK, MANUAL[0], MANUAL[2])


def dark_frames(w, h, n, seed):
    """n copies of one frame that uses a quarter of the range"""
    f = np.random.default_rng(seed).integers(10, 70, (h, w)).astype(np.uint8)
    return np.repeat(f[None], n, axis=0)


def factor(frame, w, h, gains=MANUAL, target=TARGET, max_gain=MAX_GAIN):
    ok, x = hm.exposure(hm.histogram(sm.samples(frame, w, h, w), 8), "rggb", 8, (BLACK,) * 3, gains, 0.99, target, max_gain)
    assert ok == 1 and 1.5 < x < max_gain      # dark, and not at the clamp
    return x


def stage(pkg, gains, e):
    """the quantised matrix of gain_k x e -- which must not hang on the last bit of e"""
    m = pkg.colour_matrix(tuple(min(max(g * e, 0.0), 15.99) for g in gains), None)
    for e2 in (np.nextafter(e, -np.inf), np.nextafter(e, np.inf)):
        assert pkg.colour_matrix(tuple(min(max(g * float(e2), 0.0), 15.99) for g in gains), None) == m
    return m


def model(frame, w, h, fmt, matrix):
    return cm.bayer2rgb_colour(frame, w, h, "rggb", fmt, black=(BLACK,) * 3, matrix=matrix)


def test_bayer2rgb_synchronous_follows_every_frame(plugin, gpu_pkg, tmp_path):
    w, h, n = 320, 50, 4
    src = dark_frames(w, h, n, 1)
    e = 1.0 + 1.0 * (factor(src[0], w, h) - 1.0)
    first, later = (model(src[0], w, h, "BGRx", stage(gpu_pkg, MANUAL, v)) for v in (1.0, e))
    assert not np.array_equal(first, later)
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, PROPS, "ae")
    assert np.array_equal(got[0], first)
    for i in range(1, n):
        assert np.array_equal(got[i], later), i


@pytest.mark.parametrize("speed", [0.5, None], ids=["0.5", "default"])
def test_bayer2rgb_synchronous_moves_by_ae_speed(plugin, gpu_pkg, tmp_path, speed):
    """ae-speed below 1 (None: the property left out, 0.25), with another target and ceiling: frame i under
    e_i = e_(i-1) + s (x - e_(i-1)), in doubles and in the operation order of gst_mi_auto_step"""
    w, h, n = 320, 50, 5
    src = dark_frames(w, h, n, 1)
    s = 0.25 if speed is None else speed
    props = PROPS.replace(" ae-speed=1", "" if speed is None else " ae-speed=%g" % speed) + " ae-target=0.7 ae-max-gain=3"
    x = factor(src[0], w, h, target=0.7, max_gain=3.0)
    es = [1.0]
    for _ in range(1, n):
        es.append(es[-1] + s * (x - es[-1]))
    want = [model(src[0], w, h, "BGRx", stage(gpu_pkg, MANUAL, e)) for e in es]
    assert all(not np.array_equal(want[i], want[j]) for i in range(n) for j in range(i))    # the loop cannot be frozen
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, props, "aes")
    for i in range(n):
        assert np.array_equal(got[i], want[i]), i


def test_bayer2rgb_queued_converges(plugin, gpu_pkg, tmp_path):
    w, h, n = 320, 50, 12
    src = dark_frames(w, h, n, 2)
    e = 1.0 + 1.0 * (factor(src[0], w, h) - 1.0)
    got = file_pipeline(tmp_path, src, w, h, "rggb", "RGBx", 4, PROPS + " inflight=3 devices=0,0", "aeq")
    assert np.array_equal(got[0], model(src[0], w, h, "RGBx", stage(gpu_pkg, MANUAL, 1.0)))
    assert np.array_equal(got[n - 1], model(src[0], w, h, "RGBx", stage(gpu_pkg, MANUAL, e)))


def test_hipbayer2rgb_batch_converges(plugin, gpu_pkg, tmp_path):
    w, h, n = 320, 50, 12
    src = dark_frames(w, h, n, 3)
    e = 1.0 + 1.0 * (factor(src[0], w, h) - 1.0)
    inp, outp = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    src.tofile(inp)
    res = launch(tmp_path,
                 "filesrc location=%s blocksize=%d ! video/x-bayer,format=rggb,width=%d,height=%d,framerate=30/1 "
                 "! hipupload ! hipbayer2rgb %s batch=4 ! hipdownload ! video/x-raw,format=xBGR ! filesink location=%s"
                 % (inp, w * h, w, h, PROPS, outp))
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.fromfile(outp, np.uint8).reshape(n, h, 4 * w)
    assert np.array_equal(got[0], model(src[0], w, h, "xBGR", stage(gpu_pkg, MANUAL, 1.0)))
    assert np.array_equal(got[n - 1], model(src[0], w, h, "xBGR", stage(gpu_pkg, MANUAL, e)))


def test_with_grey_world_the_white_balance_step_runs_first(plugin, gpu_pkg, tmp_path):
    """both loops at speed 1: after frame 0 the gains are green-gain x the grey-world gains, and x is taken under those"""
    w, h, n = 320, 50, 4
    src = dark_frames(w, h, n, 4)
    src[:, 0::2, 0::2] //= 2            # rggb: a red deficit for the white balance to find
    zones = sm.zone_stats(sm.samples(src[0], w, h, w), 1, 1, max(BLACK, 1), 255 - (255 >> 4))
    ok, gw = sm.grey_world(zones, "rggb", (BLACK,) * 3)
    assert ok == 1 and gw[0] > 1.5
    wb = (min(max(MANUAL[0] + 1.0 * (MANUAL[1] * gw[0] - MANUAL[0]), 0.0), 15.99), MANUAL[1],
          min(max(MANUAL[2] + 1.0 * (MANUAL[1] * gw[2] - MANUAL[2]), 0.0), 15.99))
    e = 1.0 + 1.0 * (factor(src[0], w, h, gains=wb) - 1.0)
    got = file_pipeline(tmp_path, src, w, h, "rggb", "BGRx", 4, PROPS + " white-balance=grey-world awb-speed=1", "aewb")
    assert np.array_equal(got[0], model(src[0], w, h, "BGRx", stage(gpu_pkg, MANUAL, 1.0)))
    later = model(src[0], w, h, "BGRx", stage(gpu_pkg, wb, e))
    for i in range(1, n):
        assert np.array_equal(got[i], later), i


def test_manual_spelled_out_gives_the_recorded_reference_bytes(plugin, gpu_pkg, oracle, tmp_path):
    """the md5s of tests/test_gst_colour.py: the flag is not set, the ae-* properties alone change nothing"""
    for (w, h, seed, order, fmt, md5) in ((64, 48, 7, "bggr", "RGBx", "5e213c796b18997f2a81d54aee9afcd8"),
                                          (1920, 1080, 1, "rggb", "BGRx", "f14f6ad248ef0bac0f28546db6d14813")):
        src = oracle.fill_synthetic(w, h, 1, seed=seed)
        for extra in ("exposure=manual", "exposure=manual ae-target=0.5 ae-speed=1 ae-max-gain=8"):
            got = file_pipeline(tmp_path, src, w, h, order, fmt, 4, extra, "man%d" % w)
            assert hashlib.md5(got[0].tobytes()).hexdigest() == md5, (w, extra)
