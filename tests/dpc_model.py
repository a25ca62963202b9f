"""NumPy model of the defective pixel correction (include/mibayer.h, group `dpc`): integers only, bit-exact.  The
definition restated:

  neighbours  the eight samples of the same site at (x + dx, y + dy), dx, dy in {-2, 0, 2}, not both 0; a coordinate
              off the frame is replaced by the one on the other side of the pixel (x - 2 < 0 -> x + 2, x + 2 >= W ->
              x - 2, likewise y with H); needs W >= 4 and H >= 4
  detect      hot:  S > hi + hot        cold:  S + cold < lo        (-1 = off)
  replace     pairs H, V, D1, D2 in this order; g = |a - b|; the smallest g wins, the first among equals;
              R = (a + b + 1) >> 1
  out         R if the sample is hot, cold or listed, else S; the neighbours are always those of the source

Samples are int64 arrays of native-depth values (mosaic bytes <-> samples: shading_model.unpack / pack)."""
import numpy as np

MAX_DEFECTS = 65536
PAIRS = ("H", "V", "D1", "D2")


def mirror(n):
    """(index of t - 2, index of t + 2) for t in 0 .. n - 1 under the border rule"""
    t = np.arange(n)
    lo = np.where(t - 2 < 0, t + 2, t - 2)
    hi = np.where(t + 2 >= n, t - 2, t + 2)
    return lo, hi


def neighbours(S):
    """the eight neighbours as a dict (dx, dy) -> array, dx, dy in {-1, 0, 1} standing for -2, 0, +2"""
    S = np.asarray(S, np.int64)
    h, w = S.shape
    if w < 4 or h < 4:
        raise ValueError("defective pixel correction needs a frame of at least 4 x 4")
    xl, xr = mirror(w)
    yu, yd = mirror(h)
    xs = {-1: xl, 0: np.arange(w), 1: xr}
    ys = {-1: yu, 0: np.arange(h), 1: yd}
    return {(dx, dy): S[ys[dy]][:, xs[dx]] for dy in (-1, 0, 1) for dx in (-1, 0, 1) if dx or dy}


def replacement(S):
    """(R, winner): the replacement value of every sample and the index into PAIRS of the pair it came from"""
    n = neighbours(S)
    pairs = [(n[(-1, 0)], n[(1, 0)]), (n[(0, -1)], n[(0, 1)]), (n[(-1, -1)], n[(1, 1)]), (n[(1, -1)], n[(-1, 1)])]
    g = np.stack([np.abs(a - b) for a, b in pairs])
    win = np.argmin(g, axis=0)                  # the first of equals
    r = np.stack([(a + b + 1) >> 1 for a, b in pairs])
    return np.take_along_axis(r, win[None], 0)[0], win


def flagged(S, hot=-1, cold=-1):
    """boolean map of the samples the detection flags"""
    S = np.asarray(S, np.int64)
    n = np.stack(list(neighbours(S).values()))
    hi, lo = n.max(0), n.min(0)
    bad = np.zeros(S.shape, bool)
    if hot >= 0:
        bad |= S > hi + hot
    if cold >= 0:
        bad |= S + cold < lo
    return bad


def sort_defects(defects):
    """the library's copy of a list: (n, 2) of (x, y), sorted by (y, x), duplicates dropped"""
    d = np.asarray(defects, np.int64).reshape(-1, 2)
    if not len(d):
        return np.zeros((0, 2), np.uint32)
    keys = np.unique((d[:, 1] << 32) | d[:, 0])
    return np.stack([keys & 0xffffffff, keys >> 32], 1).astype(np.uint32)


def correct(S, hot=-1, cold=-1, defects=None, y0=0, y1=None):
    """the corrected frame; rows outside [y0, y1) keep their samples"""
    S = np.asarray(S, np.int64)
    h, w = S.shape
    bad = flagged(S, hot, cold)
    if defects is not None and len(defects):
        d = np.asarray(defects, np.int64).reshape(-1, 2)
        if (d < 0).any() or (d[:, 0] >= w).any() or (d[:, 1] >= h).any():
            raise ValueError("a listed defect lies outside the frame")
        bad[d[:, 1], d[:, 0]] = True
    rows = np.zeros(S.shape, bool)
    rows[y0:h if y1 is None else y1] = True
    r, _ = replacement(S)
    return np.where(bad & rows, r, S)


def correct_slow(S, hot=-1, cold=-1, defects=None):
    """the definition, pixel by pixel (small frames only)"""
    S = np.asarray(S, np.int64)
    h, w = S.shape
    listed = set() if defects is None else {(int(x), int(y)) for x, y in np.asarray(defects).reshape(-1, 2)}
    out = S.copy()
    for y in range(h):
        yu = y + 2 if y - 2 < 0 else y - 2
        yd = y - 2 if y + 2 >= h else y + 2
        for x in range(w):
            xl = x + 2 if x - 2 < 0 else x - 2
            xr = x - 2 if x + 2 >= w else x + 2
            s = int(S[y, x])
            pairs = [(S[y, xl], S[y, xr]), (S[yu, x], S[yd, x]), (S[yu, xl], S[yd, xr]), (S[yu, xr], S[yd, xl])]
            flat = [int(v) for p in pairs for v in p]
            is_hot = hot >= 0 and s > max(flat) + hot
            is_cold = cold >= 0 and s + cold < min(flat)
            if not (is_hot or is_cold or (x, y) in listed):
                continue
            best = None
            for a, b in pairs:
                g = abs(int(a) - int(b))
                if best is None or g < best[0]:
                    best = (g, (int(a) + int(b) + 1) >> 1)
            out[y, x] = best[1]
    return out


def read_defect_file(path):
    """defect-file of bayer2rgb: text, one `x y` per line, `#` starts a comment, blank lines allowed"""
    out = []
    for line in open(path):
        line = line.split("#", 1)[0].split()
        if line:
            if len(line) != 2:
                raise ValueError("not an `x y` line: %r" % line)
            out.append((int(line[0]), int(line[1])))
    return np.asarray(out, np.uint32).reshape(-1, 2)


def correct_raw(raw, dst, width, height, stride, bits=0, big_endian=False, hot=-1, cold=-1, defects=None, y0=0, y1=None):
    """the bytes of the frame `dst` after rows [y0, y1) of the frame `raw` were corrected into it: the first `width`
    samples of those rows are written, everything else keeps what `dst` held"""
    import shading_model as shm
    import stats_model as sm
    y1 = height if y1 is None else y1
    S = sm.samples(raw, width, height, stride, bits, big_endian)
    out = correct(S, hot, cold, defects, y0, y1)
    keep = np.array(np.asarray(dst).view(np.uint8).reshape(-1), copy=True)
    full = shm.pack(out, dst, width, height, stride, bits, big_endian)
    keep[y0 * stride:y1 * stride] = full[y0 * stride:y1 * stride]
    return keep
