"""NumPy model of the noise reduction (include/mibayer.h, group `nr`): integers only, bit-exact.  The definition
restated:

  window      the 24 neighbours of the same site at (x + dx, y + dy), dx, dy in {-4, -2, 0, 2, 4}, not both 0; a
              coordinate off the frame is reflected about the edge sample (np.pad mode "reflect"); needs W >= 6, H >= 5
  threshold   17 nodes curve[0 .. 16], each 0 .. T_MAX (255 for 8-bit, min (max, 2047) for deep mosaics); sh = depth - 4,
              s = 1 << sh, k = S >> sh, f = S & (s - 1):  t = (curve[k] (s - f) + curve[k + 1] f + (s >> 1)) >> sh
  filter      n is included when |n - S| <= t; P = sum of n - S over included n > S, N = sum of S - n over included n < S,
              cnt = 1 + the number included, v = P - N, q = (2 |v| + cnt) // (2 cnt), out = S + sign (v) q
  out         a pure function of the source frame

Samples are int64 arrays of native-depth values (mosaic bytes <-> samples: shading_model.unpack / pack)."""
import math

import numpy as np

NODES = 17
OFFSETS = [(dx, dy) for dy in (-4, -2, 0, 2, 4) for dx in (-4, -2, 0, 2, 4) if dx or dy]
MIN_W, MIN_H = 6, 5


def t_max(depth):
    return 255 if depth == 8 else min((1 << depth) - 1, 2047)


def threshold(S, curve, depth):
    """t of every sample"""
    S = np.asarray(S, np.int64)
    c = np.asarray(curve, np.int64)
    if c.shape != (NODES,) or c.min() < 0 or c.max() > t_max(depth):
        raise ValueError("a curve is 17 nodes of 0 .. %d" % t_max(depth))
    sh = depth - 4
    s = 1 << sh
    k, f = S >> sh, S & (s - 1)
    return (c[k] * (s - f) + c[k + 1] * f + (s >> 1)) >> sh


def neighbours(S):
    """(24, H, W): the window of every sample, in the order of OFFSETS"""
    S = np.asarray(S, np.int64)
    h, w = S.shape
    if w < MIN_W or h < MIN_H:
        raise ValueError("noise reduction needs a frame of at least 6 x 5")
    pad = np.pad(S, 4, mode="reflect")
    return np.stack([pad[4 + dy:4 + dy + h, 4 + dx:4 + dx + w] for dx, dy in OFFSETS])


def included(S, curve, depth):
    """(24, H, W) boolean: the neighbours that take part"""
    S = np.asarray(S, np.int64)
    return np.abs(neighbours(S) - S) <= threshold(S, curve, depth)


def denoise(S, curve, depth, y0=0, y1=None):
    """the denoised frame; rows outside [y0, y1) keep their samples"""
    S = np.asarray(S, np.int64)
    n = neighbours(S)
    d = n - S
    inc = np.abs(d) <= threshold(S, curve, depth)
    P = np.where(inc & (d > 0), d, 0).sum(0)
    N = np.where(inc & (d < 0), -d, 0).sum(0)
    cnt = 1 + inc.sum(0)
    v = P - N
    q = (2 * np.abs(v) + cnt) // (2 * cnt)
    out = S + np.sign(v) * q
    rows = np.zeros(S.shape, bool)
    rows[y0:S.shape[0] if y1 is None else y1] = True
    return np.where(rows, out, S)


def reflect(t, n):
    return -t if t < 0 else 2 * (n - 1) - t if t >= n else t


def denoise_slow(S, curve, depth):
    """the definition, pixel by pixel, with Python integers (small frames only)"""
    S = np.asarray(S, np.int64)
    h, w = S.shape
    sh = depth - 4
    s = 1 << sh
    out = S.copy()
    for y in range(h):
        for x in range(w):
            c = int(S[y, x])
            k, f = c >> sh, c & (s - 1)
            t = (int(curve[k]) * (s - f) + int(curve[k + 1]) * f + (s >> 1)) >> sh
            P = N = 0
            cnt = 1
            for dx, dy in OFFSETS:
                nb = int(S[reflect(y + dy, h), reflect(x + dx, w)])
                if abs(nb - c) <= t:
                    cnt += 1
                    if nb > c:
                        P += nb - c
                    else:
                        N += c - nb
            v = P - N
            q = (2 * abs(v) + cnt) // (2 * cnt)
            out[y, x] = c + q if v >= 0 else c - q
    return out


def reciprocal(cnt):
    """ceil (2^32 / (2 cnt)): what the kernel multiplies 2 |v| + cnt by, taking the high 32 bits"""
    return ((1 << 32) + 2 * cnt - 1) // (2 * cnt)


def noise_curve(depth, black=0.0, read_noise=2.0, shot_noise=0.0, strength=1.0):
    """mibayer_nr_curve: IEEE doubles, the same expression"""
    for v in (black, read_noise, shot_noise, strength):
        if not (v >= 0.0) or math.isinf(v):
            raise ValueError("negative or non-finite argument")
    out = []
    for i in range(NODES):
        v = float(i << (depth - 4))
        over = v - black if v - black > 0.0 else 0.0
        t = math.floor(strength * math.sqrt(read_noise * read_noise + shot_noise * over) + 0.5)
        out.append(int(min(t, float(t_max(depth)))))
    return out


def denoise_raw(raw, dst, width, height, stride, bits=0, big_endian=False, curve=None, y0=0, y1=None):
    """the bytes of the frame `dst` after rows [y0, y1) of the frame `raw` were denoised into it: the first `width`
    samples of those rows are written, everything else keeps what `dst` held"""
    import shading_model as shm
    import stats_model as sm
    y1 = height if y1 is None else y1
    S = sm.samples(raw, width, height, stride, bits, big_endian)
    out = denoise(S, curve, bits or 8, y0, y1)
    keep = np.array(np.asarray(dst).view(np.uint8).reshape(-1), copy=True)
    full = shm.pack(out, dst, width, height, stride, bits, big_endian)
    keep[y0 * stride:y1 * stride] = full[y0 * stride:y1 * stride]
    return keep
