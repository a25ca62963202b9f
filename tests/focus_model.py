"""NumPy model of the mosaic focus statistics and of the focus score (include/mibayer.h, group `focus`): the definition
restated, for the CPU and GPU tests to compare the library against.

Samples, sites and the zone grid are those of tests/stats_model.py.  Per sample the same-site second differences
rh = 2 S(x, y) - S(x - 2, y) - S(x + 2, y), defined for 2 <= x <= W - 3 only, and rv = 2 S(x, y) - S(x, y - 2) -
S(x, y + 2), defined for 2 <= y <= H - 3 only; nothing is reflected.  A defined response contributes when |r| >= thr,
to the zone of its own (x, y): per zone and site the sums of |rh| and |rv| and the numbers of contributing ones."""
import numpy as np

from stats_model import SITE_COLOUR, cell, samples  # noqa: F401  (samples: re-exported for the tests)

FOCUS_DTYPE = np.dtype([("h", np.uint64, 4), ("v", np.uint64, 4), ("nh", np.uint32, 4), ("nv", np.uint32, 4)])


def check(S, zones_x, zones_y, thr, vmax):
    H, W = S.shape
    if not (1 <= zones_x <= min(64, W // 2) and 1 <= zones_y <= min(64, H // 2)):
        raise ValueError("zone grid %d x %d outside the rule for %d x %d" % (zones_x, zones_y, W, H))
    if not 0 <= thr <= 2 * vmax:
        raise ValueError("thr %d outside 0 .. 2 * %d" % (thr, vmax))


def responses(S):
    """(|rh|, defined_h, |rv|, defined_v), each (H, W); undefined responses are 0"""
    S = np.asarray(S, np.int64)
    H, W = S.shape
    rh, rv = np.zeros((H, W), np.int64), np.zeros((H, W), np.int64)
    dh, dv = np.zeros((H, W), bool), np.zeros((H, W), bool)
    if W >= 5:
        rh[:, 2:W - 2] = np.abs(2 * S[:, 2:W - 2] - S[:, :W - 4] - S[:, 4:])
        dh[:, 2:W - 2] = True
    if H >= 5:
        rv[2:H - 2] = np.abs(2 * S[2:H - 2] - S[:H - 4] - S[4:])
        dv[2:H - 2] = True
    return rh, dh, rv, dv


def zone_focus(S, zones_x, zones_y, thr, vmax):
    """(zones_y, zones_x) FOCUS_DTYPE of the (H, W) sample array S of samples 0 .. vmax"""
    check(S, zones_x, zones_y, thr, vmax)
    H, W = S.shape
    cw, ch = cell(W, zones_x), cell(H, zones_y)
    zone = (np.arange(H)[:, None] // ch) * zones_x + np.arange(W)[None, :] // cw
    rh, dh, rv, dv = responses(S)
    out = np.zeros((zones_y, zones_x), FOCUS_DTYPE)
    n = zones_x * zones_y
    for s in range(4):
        z = zone[s >> 1::2, s & 1::2].reshape(-1)
        for r, d, fs, fn in ((rh, dh, "h", "nh"), (rv, dv, "v", "nv")):
            a = r[s >> 1::2, s & 1::2].reshape(-1)
            on = d[s >> 1::2, s & 1::2].reshape(-1) & (a >= thr)
            # float64 weights are exact here: a sum stays far below 2^53
            out[fs][..., s] = np.bincount(z[on], a[on].astype(np.float64), n).astype(np.uint64).reshape(zones_y, zones_x)
            out[fn][..., s] = np.bincount(z[on], minlength=n).reshape(zones_y, zones_x)
    return out


def zone_focus_slow(S, zones_x, zones_y, thr, vmax):
    """the same, pixel by pixel"""
    check(S, zones_x, zones_y, thr, vmax)
    H, W = S.shape
    cw, ch = cell(W, zones_x), cell(H, zones_y)
    out = np.zeros((zones_y, zones_x), FOCUS_DTYPE)
    for y in range(H):
        for x in range(W):
            z = out[y // ch, x // cw]
            s, c = 2 * (y & 1) + (x & 1), int(S[y, x])
            if 2 <= x <= W - 3:
                r = abs(2 * c - int(S[y, x - 2]) - int(S[y, x + 2]))
                if r >= thr:
                    z["h"][s] += np.uint64(r)
                    z["nh"][s] += 1
            if 2 <= y <= H - 3:
                r = abs(2 * c - int(S[y - 2, x]) - int(S[y + 2, x]))
                if r >= thr:
                    z["v"][s] += np.uint64(r)
                    z["nv"][s] += 1
    return out


def counts_at_zero(W, H):
    """(nh[4], nv[4]) over all zones with thr = 0: every defined response contributes"""
    nh, nv = [], []
    for s in range(4):
        rows = len(range(s >> 1, H, 2))
        rows_v = len([y for y in range(s >> 1, H, 2) if 2 <= y <= H - 3])
        nh.append(rows * ((W - 4) // 2))
        nv.append((W // 2) * rows_v)
    return nh, nv


def score(zones, pattern, colour=1, weights=None):
    """(ok, score) as mibayer_focus_score: doubles, zone by zone, no fused multiply-add"""
    zones = np.asarray(zones).reshape(-1)
    if weights is not None:
        weights = [float(w) for w in np.asarray(weights, np.float64).reshape(-1)]
        assert len(weights) == zones.size
        if any(not (w >= 0.0) or w == float("inf") for w in weights):
            raise ValueError("weights must be finite and >= 0")
    sites = [s for s in range(4) if colour == 3 or SITE_COLOUR[pattern][s] == colour]
    A = N = 0.0
    for i, z in enumerate(zones):
        az = sum(int(z["h"][s]) + int(z["v"][s]) for s in sites) & (2 ** 64 - 1)
        nz = sum(int(z["nh"][s]) + int(z["nv"][s]) for s in sites)
        w = 1.0 if weights is None else weights[i]
        A += w * float(az)
        N += w * float(nz)
    if not N > 0.0:
        return 0, 0.0
    return 1, A / N
