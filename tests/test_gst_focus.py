"""GPU tests of bayer2rgb focus-zones-x / focus-zones-y / focus-threshold: a gst-launch -m pipeline over a 258 x 37 stream
of three different frames, 8-bit and 12-bit.  One `mibayer-focus` element message per frame, its score and zone scores
the model's doubles exactly (GStreamer serialises doubles round-trip), the output bytes those of the same pipeline
without the properties, and no message with the defaults."""
import os
import re
import subprocess

import numpy as np
import pytest

import focus_model as fm
import strip_cases as sc
from test_gst_element import GST_LAUNCH, gst_env, needs_gst, plugin  # noqa: F401  (fixture)

pytestmark = [pytest.mark.gpu, needs_gst]

W, H = 258, 37


def pipeline(tmp, src, order, fmt, bpp, props, tag):
    """(frames, [message fields]) of filesrc ! bayer2rgb `props` ! filesink under gst-launch -m"""
    inp = os.path.join(str(tmp), "in_%s.raw" % tag)
    outp = os.path.join(str(tmp), "out_%s.raw" % tag)
    src.tofile(inp)
    line = ("filesrc location=%s blocksize=%d ! video/x-bayer,format=%s,width=%d,height=%d,framerate=1/1 "
            "! bayer2rgb %s ! video/x-raw,format=%s ! filesink location=%s" % (inp, src[0].size, order, W, H, props, fmt, outp))
    res = subprocess.run([GST_LAUNCH, "-m"] + line.split(), capture_output=True, text=True, env=gst_env(tmp), timeout=300)
    assert res.returncode == 0, res.stderr[-1500:]
    assert "WARNING" not in res.stderr and "ERROR" not in res.stderr, res.stderr[-1500:]
    data = np.fromfile(outp, np.uint8)
    assert data.size == src.shape[0] * bpp * W * H
    msgs = []
    for ln in res.stdout.splitlines():
        if "mibayer-focus" not in ln:
            continue
        field = lambda name, kind: re.search(r"%s=\(%s\)([^,;<]+)" % (name, kind), ln).group(1).strip()  # noqa: E731
        scores = re.search(r"zone-scores=\(double\)<([^>]*)>", ln).group(1)
        msgs.append(dict(frame=int(field("frame", "guint64")), zx=int(field("zones-x", "int")),
                         zy=int(field("zones-y", "int")), thr=int(field("threshold", "uint")),
                         score=float(field("score", "double")), zones=[float(v) for v in scores.split(",")]))
    return data.reshape(src.shape[0], H, bpp * W), msgs


def check(msgs, samples, order, zx, zy, thr, vmax):
    assert [m["frame"] for m in msgs] == list(range(len(samples)))
    for m, S in zip(msgs, samples):
        assert (m["zx"], m["zy"], m["thr"]) == (zx, zy, thr)
        z = fm.zone_focus(S, zx, zy, thr, vmax)
        assert m["score"] == fm.score(z, order, 1)[1]
        assert m["zones"] == [fm.score(one, order, 1)[1] for one in z.reshape(-1)]
    assert msgs[2]["score"] < msgs[0]["score"]          # frame 2 is the blurred copy of frame 0


def blurred(S):
    B = S.copy()
    B[:, 2:-2] = (S[:, :-4] + 2 * S[:, 2:-2] + S[:, 4:] + 2) // 4
    B[2:-2] = (B[:-4] + 2 * B[2:-2] + B[4:] + 2) // 4
    return B


@pytest.mark.parametrize("extra", ["", "inflight=3 devices=0,0"])
def test_bayer2rgb_focus_messages_8bit(plugin, gpu_pkg, tmp_path, extra):
    rng = np.random.default_rng(2583)
    S = rng.integers(0, 256, (3, H, W))
    S[2] = blurred(S[0])
    src = np.full((3, H, 260), 0x5A, np.uint8)
    src[:, :, :W] = S
    plain, none = pipeline(tmp_path, src, "grbg", "BGRx", 4, extra or "inflight=1", "plain")
    assert none == []                                   # the defaults post nothing
    for k, (zx, zy, thr) in enumerate(((3, 5, 0), (1, 1, 40))):
        got, msgs = pipeline(tmp_path, src, "grbg", "BGRx", 4,
                             "focus-zones-x=%d focus-zones-y=%d focus-threshold=%d %s" % (zx, zy, thr, extra), "f%d" % k)
        assert np.array_equal(got, plain)
        check(msgs, list(S), "grbg", zx, zy, thr, 255)
    # one of the two at 0 is off as well
    got, msgs = pipeline(tmp_path, src, "grbg", "BGRx", 4, "focus-zones-x=3 focus-threshold=9 " + extra, "half")
    assert msgs == [] and np.array_equal(got, plain)


def test_bayer2rgb_focus_messages_12bit(plugin, gpu_pkg, tmp_path):
    rng = np.random.default_rng(2584)
    S = rng.integers(0, 4096, (3, H, W)).astype(np.int64)
    S[2] = blurred(S[0])
    src = np.stack([sc.frame_bytes(S[i], 12, rng) for i in range(3)])
    plain, none = pipeline(tmp_path, src, "rggb12le", "ARGB64", 8, "inflight=1", "plain12")
    assert none == []
    got, msgs = pipeline(tmp_path, src, "rggb12le", "ARGB64", 8, "focus-zones-x=4 focus-zones-y=3 focus-threshold=500", "f12")
    assert np.array_equal(got, plain)
    check(msgs, list(S), "rggb", 4, 3, 500, 4095)


def test_a_grid_the_library_refuses_is_an_element_error(plugin, gpu_pkg, tmp_path):
    src = np.zeros((1, H, 260), np.uint8)
    inp = os.path.join(str(tmp_path), "in.raw")
    src.tofile(inp)
    for props in ("focus-zones-x=3 focus-zones-y=19", "focus-zones-x=1 focus-zones-y=1 focus-threshold=511"):
        line = ("filesrc location=%s blocksize=%d ! video/x-bayer,format=grbg,width=%d,height=%d,framerate=1/1 "
                "! bayer2rgb %s ! video/x-raw,format=BGRx ! fakesink" % (inp, src[0].size, W, H, props))
        res = subprocess.run([GST_LAUNCH, "-q"] + line.split(), capture_output=True, text=True, env=gst_env(tmp_path),
                             timeout=300)
        assert res.returncode != 0 and "cannot set up focus statistics" in res.stderr, res.stderr[-1500:]
