"""exposure=auto and white-balance=grey-world under scenes that MOVE: every frame of a sequence has a brightness and a
channel balance of its own, so which frame's measurement steers which later frame shows in the bytes.  gst-launch
pipelines, compared byte for byte with the colour model (tests/colour_model.py) under the state a Python restatement
of gst_mi_auto_step / gst_mi_awb_step (gst/gstmicolour.h) holds -- doubles, in their operation order, fed with
tests/hist_model.py and tests/stats_model.py.  One test at the top runs without a GPU: it asserts, for every sequence
used below, that the scenes can tell any two candidate states apart."""
import collections
import functools

import numpy as np
import pytest

import colour_model as cm
import hist_model as hm
import stats_model as sm
from test_gst_colour import file_pipeline
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_hipmemory import launch

W, H = 320, 50
MANUAL = (1.25, 1.0, 0.75)
GAIN_MAX = 15.99
ORDERS = ("rggb", "bggr", "gbrg", "grbg")
# per frame of a sequence: how bright, and where the red and the blue sites sit against the green ones.  Red is the
# brightest channel, before and after the gains: a histogram read under another Bayer order has another percentile
BRIGHT = (0.30, 0.52, 0.38, 0.60, 0.26, 0.45, 0.34, 0.56, 0.41, 0.28, 0.49, 0.36, 0.58, 0.32, 0.47, 0.43)
RED = (1.10, 1.40, 1.22, 1.50, 1.30, 1.16, 1.44, 1.26, 1.12, 1.36, 1.20, 1.48, 1.32, 1.14, 1.42, 1.24)
BLUE = (0.75, 0.60, 0.90, 0.50, 0.80, 0.66, 0.54, 0.86, 0.70, 0.58, 0.94, 0.62, 0.78, 0.68, 0.52, 0.84)

Setup = collections.namedtuple("Setup", "order bits n ae awb ae_speed awb_speed max_gain ccm bright seed",
                               defaults=("rggb", 0, 6, False, False, 0.5, 0.5, 8.0, None, BRIGHT, 1))
MODES = {"ae": dict(ae=True), "awb": dict(awb=True), "both": dict(ae=True, awb=True)}
# C5: with ccm = 2 x identity a red gain x e past 15.99 / 2 leaves the matrix range: frames 1, 2 and 4 are that dark
REFUSED = Setup(ae=True, max_gain=GAIN_MAX, ccm=(2, 0, 0, 0, 2, 0, 0, 0, 2),
                bright=(0.40, 0.07, 0.075, 0.50, 0.0727, 0.45), seed=5)
REFUSED_STEPS = (True, False, False, True, False, True)


def depth(su):
    return su.bits or 8


def black(su):
    return 8 << (depth(su) - 8)


def props(su):
    s = "black-level=%d red-gain=%g blue-gain=%g" % (black(su), MANUAL[0], MANUAL[2])
    if su.ae:
        s += " exposure=auto ae-speed=%g ae-max-gain=%g" % (su.ae_speed, su.max_gain)
    if su.awb:
        s += " white-balance=grey-world awb-speed=%g" % su.awb_speed
    if su.ccm:
        s += " ccm=" + ",".join("%g" % v for v in su.ccm)
    return s


@functools.lru_cache(maxsize=None)
def scene(su):
    """(n, H, W) samples: frame j random over most of the range, times BRIGHT[j], its red sites times RED[j] and its
    blue sites times BLUE[j]"""
    rng = np.random.default_rng([su.seed, su.bits, ORDERS.index(su.order)])
    vmax = (1 << depth(su)) - 1
    yy, xx = np.mgrid[0:H, 0:W]
    k = np.asarray(sm.SITE_COLOUR[su.order])[2 * (yy & 1) + (xx & 1)]
    out = []
    for j in range(su.n):
        base = rng.integers(vmax // 10, vmax - vmax // 10, (H, W)).astype(np.float64)
        out.append((base * su.bright[j] * np.asarray((RED[j], 1.0, BLUE[j]))[k]).astype(np.int64))
    S = np.stack(out)
    S.setflags(write=False)
    return S


def source(su):
    """the bytes gst-launch reads: a byte per sample, or 16-bit little-endian words with random junk above `bits`"""
    S = scene(su)
    if not su.bits:
        return S.astype(np.uint8)
    junk = np.random.default_rng(su.seed).integers(0, 1 << 16, S.shape) << su.bits & 0xFFFF
    return (S | junk).astype("<u2").view(np.uint8).reshape(su.n, H, 2 * W)


def clamp(g):
    return min(max(g, 0.0), GAIN_MAX)


class Loop:
    """gst_mi_auto_step (exposure=auto, with or without grey-world) / gst_mi_awb_step (grey-world alone, where e stays
    1 and gain x 1.0 is the gain): the state an element holds, and the quantised matrix of its colour stage"""

    def __init__(self, pkg, su, order=None):
        self.pkg, self.su, self.order = pkg, su, order or su.order
        self.wb, self.e = [MANUAL[0], MANUAL[2]], 1.0
        self.xs = []            # every exposure factor a step was given
        self.matrix = pkg.colour_matrix(MANUAL, su.ccm)

    def measure(self, S):
        """(grey-world gains or None, the function q -> exposure factor or None) of one frame"""
        su, d, b = self.su, depth(self.su), (float(black(self.su)),) * 3
        vmax = (1 << d) - 1
        ok, gw = sm.grey_world(sm.zone_stats(S, 1, 1, max(black(su), 1), vmax - (vmax >> 4)), self.order, b)
        hist = hm.histogram(S, d)

        def x(q):
            have, v = hm.exposure(hist, self.order, d, b, q, 0.99, 0.9, su.max_gain)
            return v if have == 1 else None
        return (gw if ok == 1 else None), x

    def step(self, S):
        """TRUE: the stage moved; FALSE: refused or nothing measured, and nothing changes"""
        su = self.su
        gw, x = self.measure(S)
        q, e, moved = list(MANUAL), self.e, False
        if su.awb:
            q[0], q[2] = self.wb
            if gw is not None:
                for k in range(2):
                    q[2 * k] = clamp(self.wb[k] + su.awb_speed * (MANUAL[1] * gw[2 * k] - self.wb[k]))
                moved = True
        if su.ae:
            v = x(q)
            if v is not None:
                self.xs.append(v)
                e += su.ae_speed * (v - e)
                moved = True
        if not moved:
            return False
        try:
            matrix = self.pkg.colour_matrix([clamp(g * e) for g in q], su.ccm)
        except self.pkg.MibayerError:
            return False
        self.wb, self.e, self.matrix = [q[0], q[2]], e, matrix
        return True

    def neighbours(self):
        """the matrices of the states a few last bits of e or of a gain away: all must be self.matrix"""
        out = []
        for de in (-4, 0, 4):
            for dg in (-4, 0, 4):
                e = self.e * (1.0 + de * 2.0 ** -52)
                q = [self.wb[0] * (1.0 + dg * 2.0 ** -52), MANUAL[1], self.wb[1] * (1.0 + dg * 2.0 ** -52)]
                out.append(self.pkg.colour_matrix([clamp(g * e) for g in q], self.su.ccm))
        return out


@functools.lru_cache(maxsize=None)
def plain(su, i):
    """frame i demosaiced without a colour stage: what every state's output is computed from"""
    return cm.plain_argb64(source(su)[i], W, H, su.order, su.bits)[0]


def fmt_of(su, hip=False):
    return "xBGR" if hip else "ARGB64" if su.bits else "BGRx"


def render(su, i, matrix, hip=False, rows=slice(None)):
    """frame i under `matrix` (the stage works pixel by pixel: `rows` gives those rows of the frame alone)"""
    return cm.colour(plain(su, i)[rows], depth(su), fmt_of(su, hip), bool(su.bits), (black(su),) * 3, matrix)


def states_in_order(pkg, su):
    """[matrix before frame 0, after the step of frame 0, after that of frame 1, ...] and which steps moved"""
    loop = Loop(pkg, su)
    out, moved = [loop.matrix], []
    for S in scene(su):
        moved.append(loop.step(S))
        assert all(m == loop.matrix for m in loop.neighbours())
        out.append(loop.matrix)
    assert all(1.0 / 16 < x < su.max_gain for x in loop.xs)      # under the moving gains too: never a clamped factor
    return out, moved


def states_by_frame(pkg, su):
    """speed 1: {-1: the matrix of the properties, j: the matrix once frame j has been measured}"""
    assert (su.ae_speed, su.awb_speed) == (1.0, 1.0) and su.ae != su.awb
    out = {-1: Loop(pkg, su).matrix}
    for j, S in enumerate(scene(su)):
        loop = Loop(pkg, su)
        assert loop.step(S) and all(m == loop.matrix for m in loop.neighbours())
        out[j] = loop.matrix
    return out


def sync_setups():
    for order in ORDERS:
        for mode, kw in MODES.items():
            yield "%s-%s" % (mode, order), Setup(order=order, **kw)
    for mode, kw in MODES.items():
        yield "%s-rggb12le" % mode, Setup(bits=12, seed=3, **kw)


def queued_setups():
    for mode, kw in MODES.items():
        yield mode, Setup(n=10, seed=2, **kw)


def batch_setups():
    yield "ae", Setup(n=12, ae=True, ae_speed=1.0, awb_speed=1.0, seed=4)
    yield "awb", Setup(n=12, awb=True, ae_speed=1.0, awb_speed=1.0, seed=4)


SYNC, QUEUED, BATCH = dict(sync_setups()), dict(queued_setups()), dict(batch_setups())


# ------------------------------------------------------------------------------------------------------------ CPU

def distinct(su, matrices, hip=False):
    """every frame of the sequence comes out different under any two of the matrices"""
    for i in range(su.n):
        outs = [render(su, i, m, hip).tobytes() for m in matrices]
        assert len(set(outs)) == len(matrices), i


@pytest.mark.parametrize("name", ["sync:" + k for k in SYNC] + ["queued:" + k for k in QUEUED]
                         + ["batch:" + k for k in BATCH] + ["refused"])
def test_scenes_tell_any_two_candidate_states_apart(pkg, name):
    kind, _, key = name.partition(":")
    su = REFUSED if kind == "refused" else {"sync": SYNC, "queued": QUEUED, "batch": BATCH}[kind][key]
    S = scene(su)
    vmax = (1 << depth(su)) - 1
    assert S.shape == (su.n, H, W) and S.min() >= 0 and S.max() <= vmax
    # the measurements of the frames: pairwise distinct, away from both clamps -- and a histogram or a zone read under
    # another order gives another answer
    xs, gws = [], []
    for frame in S:
        gw, x = Loop(pkg, su).measure(frame)
        xs.append(x(MANUAL))
        gws.append(gw)
        assert 1.0 / 16 * 1.05 < xs[-1] < su.max_gain * 0.95
        if kind != "refused":           # (frames that dark have no usable means; the sequence runs exposure=auto alone)
            assert gw[0] < 0.95 and gw[2] > 1.05 and all(1.0 / 16 * 1.05 < g < GAIN_MAX * 0.95 for g in gw)
        for other in ORDERS:
            if other != su.order:
                gw2, x2 = Loop(pkg, su, other).measure(frame)
                assert x2(MANUAL) != xs[-1] and gw2 != gw, other
    assert len(set(xs)) == su.n
    assert kind == "refused" or len({g[0] for g in gws}) == len({g[2] for g in gws}) == su.n
    if kind == "batch":
        distinct(su, list(states_by_frame(pkg, su).values()), hip=True)
        return
    states, moved = states_in_order(pkg, su)
    if kind == "refused":
        assert tuple(moved) == REFUSED_STEPS
        # a refused step leaves the matrix as it was; the others move it
        assert [states[i + 1] == states[i] for i in range(su.n)] == [not m for m in REFUSED_STEPS]
        distinct(su, [states[0]] + [states[i + 1] for i in range(su.n) if moved[i]])
        # what was refused would have fitted without the ccm, and is no clamp of the exposure helper
        assert all(Loop(pkg, su._replace(ccm=None)).step(frame) for frame in S)
    else:
        assert all(moved)
        distinct(su, states)


# ------------------------------------------------------------------------------------------------------------ GPU

def run_bayer2rgb(tmp_path, su, extra=""):
    bpp = 8 if su.bits else 4
    order = su.order + ("12le" if su.bits else "")
    return file_pipeline(tmp_path, source(su), W, H, order, fmt_of(su), bpp, (props(su) + " " + extra).strip(), "scene")


@pytest.mark.gpu
@needs_gst
@pytest.mark.parametrize("name", list(SYNC))
def test_bayer2rgb_synchronous_every_frame_under_its_predecessors(plugin, gpu_pkg, tmp_path, name):
    """C1 / C4: frame i under the state built from the measurements of frames 0 .. i - 1, in order -- for every Bayer
    order (the pattern reaches the helpers) and for a 12-bit mosaic with 16-bit output (the depth does)"""
    su = SYNC[name]
    states, _ = states_in_order(gpu_pkg, su)
    got = run_bayer2rgb(tmp_path, su)
    for i in range(su.n):
        assert np.array_equal(got[i], render(su, i, states[i])), i


@pytest.mark.gpu
@needs_gst
def test_bayer2rgb_refused_steps_leave_the_state(plugin, gpu_pkg, tmp_path):
    """C5: the steps of frames 1, 2 and 4 would take red-gain x e x ccm past 15.99 and are refused: frames 2, 3 and 5
    run under the state of their predecessor, and the loop moves again with the steps of frames 3 and 5"""
    su = REFUSED
    states, moved = states_in_order(gpu_pkg, su)
    assert tuple(moved) == REFUSED_STEPS
    got = run_bayer2rgb(tmp_path, su)
    for i in range(su.n):
        assert np.array_equal(got[i], render(su, i, states[i])), i


@pytest.mark.gpu
@needs_gst
@pytest.mark.parametrize("extra,capacity", [("inflight=3", 3), ("inflight=3 devices=0,0", 6)])
@pytest.mark.parametrize("name", list(QUEUED))
def test_bayer2rgb_queued_every_frame_under_the_collected_ones(plugin, gpu_pkg, tmp_path, name, extra, capacity):
    """C2.  The rule, read from gstmibayerelement.c and mibayer_pool.cpp: everything happens on the streaming thread.
    element_generate_output submits the frame it was given (mibayer_pool_submit keeps the pool's colour stage of that
    moment WITH the frame) and then collects the oldest frame -- the step of gst_mi_auto_step / gst_mi_awb_step runs
    inside element_collect_locked, in submission order -- when nothing has left the element yet (frame 0, for the
    preroll) or when `capacity` = inflight x devices frames are pending.  So frame 0 runs under the properties, frames
    1 .. capacity under the state after the step of frame 0 alone, and frame i > capacity under the state after the
    steps of frames 0 .. i - capacity.  No thread timing enters: mibayer_pool_wait hands frames back in order, and
    the drain at EOS collects without submitting."""
    su = QUEUED[name]
    assert su.n > capacity + 2
    states, _ = states_in_order(gpu_pkg, su)
    got = run_bayer2rgb(tmp_path, su, extra)
    for i in range(su.n):
        steps = 0 if i == 0 else max(1, i - capacity + 1)
        assert np.array_equal(got[i], render(su, i, states[steps])), (i, steps)


@pytest.mark.gpu
@needs_gst
@pytest.mark.parametrize("name", list(BATCH))
def test_hipbayer2rgb_batch_every_frame_under_one_earlier_measurement(plugin, gpu_pkg, tmp_path, name):
    """C3: the measurement is polled through an event, so which frames get measured depends on timing.  At speed 1
    the state is a function of the last measured frame alone: every output frame i must be the model of frame i under
    the properties (j = -1) or under the measurement of ONE frame j < i, j must never go back, and the last frame must
    not still be under the properties"""
    su = BATCH[name]
    states = states_by_frame(gpu_pkg, su)
    inp, outp = str(tmp_path / "in.raw"), str(tmp_path / "out.raw")
    source(su).tofile(inp)
    res = launch(tmp_path,
                 "filesrc location=%s blocksize=%d ! video/x-bayer,format=%s,width=%d,height=%d,framerate=30/1 "
                 "! hipupload ! hipbayer2rgb %s batch=4 ! hipdownload ! video/x-raw,format=xBGR ! filesink location=%s"
                 % (inp, W * H, su.order, W, H, props(su), outp))
    assert res.returncode == 0, res.stderr[-2000:]
    got = np.fromfile(outp, np.uint8).reshape(su.n, H, 4 * W)
    js = []
    for i in range(su.n):
        top = slice(0, 2)               # the candidates that fit the first rows, then the whole frame for those
        match = [j for j, m in states.items() if np.array_equal(got[i][top], render(su, i, m, True, top))]
        match = [j for j in match if np.array_equal(got[i], render(su, i, states[j], True))]
        assert len(match) == 1, (i, match)
        js.append(match[0])
    print("hipbayer2rgb batch=4 %s: j per output frame = %s" % (name, js))
    assert all(j < i for i, j in enumerate(js)), js
    assert all(a <= b for a, b in zip(js, js[1:])), js
    assert js[-1] != -1, js
