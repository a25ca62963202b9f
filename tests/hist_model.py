"""NumPy model of the mosaic histogram and of its two host helpers (include/mibayer.h, group `hist`): the definition
restated, for the CPU and GPU tests to compare the library against.

A sample S is what stats_model.samples gives (the byte of an 8-bit mosaic, or the 16-bit word in the given byte order
masked to `bits`); depth is 8 or `bits`; site s = 2 (y & 1) + (x & 1) in frame coordinates; bin = S >> (depth - 8).
bin[s][b] counts the samples of site s inside the window (x0, y0, w, h) whose bin is b; (0, 0, 0, 0) is the whole frame."""
import math

import numpy as np

from stats_model import SITE_COLOUR, samples  # noqa: F401  (samples: re-exported for the tests)

BINS = 256


def window(W, H, win=(0, 0, 0, 0)):
    """the window resolved against a W x H frame, or ValueError where the library answers MIBAYER_ERR_ARG"""
    x0, y0, w, h = win
    if (x0, y0, w, h) == (0, 0, 0, 0):
        return 0, 0, W, H
    if x0 < 0 or y0 < 0 or x0 & 1 or w & 1 or w < 2 or h < 1 or x0 + w > W or y0 + h > H:
        raise ValueError("window %r of a %d x %d frame" % (win, W, H))
    return x0, y0, w, h


def histogram(S, depth, win=(0, 0, 0, 0)):
    """(4, 256) uint32 histogram of the (H, W) sample array S"""
    H, W = S.shape
    x0, y0, w, h = window(W, H, win)
    out = np.zeros((4, BINS), np.uint32)
    inside = np.zeros((H, W), bool)
    inside[y0:y0 + h, x0:x0 + w] = True
    for s in range(4):
        v = S[s >> 1::2, s & 1::2][inside[s >> 1::2, s & 1::2]]
        out[s] = np.bincount(v >> (depth - 8), minlength=BINS)
    return out


def histogram_slow(S, depth, win=(0, 0, 0, 0)):
    """the same, pixel by pixel"""
    H, W = S.shape
    x0, y0, w, h = window(W, H, win)
    out = np.zeros((4, BINS), np.uint32)
    for y in range(y0, y0 + h):
        for x in range(x0, x0 + w):
            out[2 * (y & 1) + (x & 1), int(S[y, x]) >> (depth - 8)] += 1
    return out


def pooled(hist, pattern, colour):
    """256 Python integers: the sites of `colour` (0 / 1 / 2 = R / G / B, 3 = all four) added up"""
    hist = np.asarray(hist)
    sites = [s for s, k in enumerate(SITE_COLOUR[pattern]) if colour == 3 or k == colour]
    return [sum(int(hist[s, b]) for s in sites) for b in range(BINS)]


def percentile_bin(hist, pattern, colour, fraction):
    """(ok, bin): the smallest bin whose inclusive cumulative count reaches rank max(1, ceil(fraction N)); (0, -1) for
    a colour without samples"""
    counts = pooled(hist, pattern, colour)
    N = sum(counts)
    if N == 0:
        return 0, -1
    r = max(1, int(math.ceil(fraction * float(N))))
    cum = 0
    for b, n in enumerate(counts):
        cum += n
        if cum >= r:
            return 1, b
    return 1, BINS - 1


def exposure(hist, pattern, depth, black=None, gains=None, fraction=0.99, target=0.9, max_gain=4.0):
    """(ok, factor): doubles, in the order include/mibayer.h gives"""
    black = (0.0, 0.0, 0.0) if black is None else [float(v) for v in black]
    gains = (1.0, 1.0, 1.0) if gains is None else [float(v) for v in gains]
    vmax = float((1 << depth) - 1)
    level, ok = 0.0, True
    for k in range(3):
        have, b = percentile_bin(hist, pattern, k, fraction)
        if not have or not black[k] < vmax:
            ok = False
            continue
        v = float(b + 1) * float(1 << (depth - 8)) - 1.0
        level = max(level, gains[k] * max(v - black[k], 0.0) / (vmax - black[k]))
    if not ok or not level > 0.0:
        return 0, 1.0
    return 1, min(max(target / level, 1.0 / 16), max_gain)
