"""NumPy model of the lens shading correction and of its host helpers (include/mibayer.h, group `shading`): the
definition restated, for the CPU and GPU tests to compare the library against.

A sample S, depth, max = 2^depth - 1 and site s = 2 (y & 1) + (x & 1) are those of group `stats` (stats_model.samples).
Cells are cw = 1 << kx by ch = 1 << ky pixels, kx, ky in 2 .. 8; nodes nx = ((W - 1) >> kx) + 2, ny = ((H - 1) >> ky) + 2,
at most 129 per direction; the table is uint16 g[4][ny][nx], site-major, Q12 (4096 = 1.0), entries 0 .. 32767.

Gain at (x, y), g the plane of the pixel's site: i = x >> kx, fx = x & (cw - 1), j = y >> ky, fy = y & (ch - 1),
  G = ((g[j][i] (cw - fx) + g[j][i+1] fx) (ch - fy) + (g[j+1][i] (cw - fx) + g[j+1][i+1] fx) fy + (1 << (kx+ky-1))) >> (kx+ky)
exact in uint32.  Apply, black[4] per site, each <= max: d = S - black[s] (signed),
  out = clamp (black[s] + ((d G + 2048) >> 12), 0, max)
with an arithmetic shift; d G + 2048 fits int32.  A deep sample is written as the 16-bit word in the source's byte order
with the bits above `bits` zero; only the first W samples of a row are written."""
import math

import numpy as np

import stats_model as sm

MAX_NODES = 129
UNITY = 4096
MAX_ENTRY = 32767


def nodes(width, height, kx, ky):
    """(nx, ny); ValueError where the library returns MIBAYER_ERR_ARG"""
    if width < 1 or height < 1 or not (2 <= kx <= 8 and 2 <= ky <= 8):
        raise ValueError("geometry")
    nx, ny = ((width - 1) >> kx) + 2, ((height - 1) >> ky) + 2
    if nx > MAX_NODES or ny > MAX_NODES:
        raise ValueError("more than %d nodes" % MAX_NODES)
    return nx, ny


def gain_map(table, width, height, kx, ky):
    """(H, W) int64 G of every pixel, each from the plane of its site; the intermediate values are checked against
    uint32"""
    nx, ny = nodes(width, height, kx, ky)
    g = np.asarray(table).astype(np.int64).reshape(4, ny, nx)
    assert g.min() >= 0 and g.max() <= MAX_ENTRY
    cw, ch = 1 << kx, 1 << ky
    y, x = np.arange(height)[:, None], np.arange(width)[None, :]
    i, fx, j, fy = x >> kx, x & (cw - 1), y >> ky, y & (ch - 1)
    s = 2 * (y & 1) + (x & 1)
    top = g[s, j, i] * (cw - fx) + g[s, j, i + 1] * fx
    bot = g[s, j + 1, i] * (cw - fx) + g[s, j + 1, i + 1] * fx
    acc = top * (ch - fy) + bot * fy + (1 << (kx + ky - 1))
    assert acc.max() < 1 << 32
    return acc >> (kx + ky)


def apply(S, table, kx, ky, black, depth):
    """(H, W) int64 shaded samples of the (H, W) sample array S"""
    H, W = S.shape
    vmax = (1 << depth) - 1
    black = np.asarray(black, np.int64)
    assert black.shape == (4,) and black.min() >= 0 and black.max() <= vmax
    G = gain_map(table, W, H, kx, ky)
    bl = black[2 * (np.arange(H)[:, None] & 1) + (np.arange(W)[None, :] & 1)]
    acc = (S.astype(np.int64) - bl) * G + 2048
    assert acc.max() < 1 << 31 and acc.min() >= -(1 << 31)
    return np.clip(bl + (acc >> 12), 0, vmax)         # >> on int64 is arithmetic


def apply_slow(S, table, kx, ky, black, depth):
    """the same, pixel by pixel in Python integers"""
    H, W = S.shape
    nx, ny = nodes(W, H, kx, ky)
    g = np.asarray(table).reshape(4, ny, nx)
    cw, ch, vmax = 1 << kx, 1 << ky, (1 << depth) - 1
    out = np.zeros((H, W), np.int64)
    for y in range(H):
        for x in range(W):
            s = 2 * (y & 1) + (x & 1)
            i, fx, j, fy = x >> kx, x & (cw - 1), y >> ky, y & (ch - 1)
            p = g[s]
            G = ((int(p[j, i]) * (cw - fx) + int(p[j, i + 1]) * fx) * (ch - fy)
                 + (int(p[j + 1, i]) * (cw - fx) + int(p[j + 1, i + 1]) * fx) * fy + (1 << (kx + ky - 1))) >> (kx + ky)
            d = int(S[y, x]) - int(black[s])
            out[y, x] = min(max(int(black[s]) + ((d * G + 2048) >> 12), 0), vmax)
    return out


def pack(S, raw, width, height, stride, bits=0, big_endian=False):
    """the bytes of a frame that held `raw` after the first `width` samples of each row were overwritten with S"""
    out = np.array(np.asarray(raw).view(np.uint8).reshape(-1), copy=True)
    rows = out[:height * stride].reshape(height, stride)
    if bits == 0:
        rows[:, :width] = S.astype(np.uint8)
    else:
        hi, lo = (S >> 8).astype(np.uint8), (S & 255).astype(np.uint8)
        rows[:, 0:2 * width:2] = hi if big_endian else lo
        rows[:, 1:2 * width:2] = lo if big_endian else hi
    return out


def shade_raw(raw, table, kx, ky, black, width, height, stride, bits=0, big_endian=False, dst=None):
    """the frame `raw` shaded: bytes of the same layout (in place), or `dst` with the samples written into it"""
    S = sm.samples(raw, width, height, stride, bits, big_endian)
    out = apply(S, table, kx, ky, black, bits or 8)
    return pack(out, raw if dst is None else dst, width, height, stride, bits, big_endian)


def _locate(c, p):
    n = len(c)
    if n == 1 or p <= c[0]:
        lo, t = 0, 0.0
    elif p >= c[n - 1]:
        lo, t = n - 1, 0.0
    else:
        lo = 0
        while c[lo + 1] <= p:
            lo += 1
        t = (p - c[lo]) / (c[lo + 1] - c[lo])
    return lo, min(lo + 1, n - 1), t


def stats_shading(zones, width, height, black, kx, ky, max_gain):
    """(ok, (4, ny, nx) uint16 table) from the (zones_y, zones_x) STATS_DTYPE zones of a flat field, in the order
    include/mibayer.h spells out, in Python floats (IEEE doubles)"""
    zones = np.asarray(zones)
    zones_y, zones_x = zones.shape
    nx, ny = nodes(width, height, kx, ky)
    unity = np.full((4, ny, nx), UNITY, np.uint16)
    if not (width >= 2 and width % 2 == 0 and 1 <= zones_x <= min(64, width // 2)
            and 1 <= zones_y <= min(64, height // 2) and 1.0 <= max_gain <= 7.99):
        raise ValueError("arguments")
    zcw, zch = sm.cell(width, zones_x), sm.cell(height, zones_y)
    ux, uy = -(-width // zcw), -(-height // zch)
    cx = [float(a * zcw + min((a + 1) * zcw, width)) * 0.5 for a in range(ux)]
    cy = [float(b * zch + min((b + 1) * zch, height)) * 0.5 for b in range(uy)]
    black = (0, 0, 0, 0) if black is None else black
    out = unity.copy()
    for s in range(4):
        full = [[int(zones["count"][b, a, s]) > 0 for a in range(ux)] for b in range(uy)]
        if not any(any(r) for r in full):
            return 0, unity
        m = [[float(int(zones["sum"][b, a, s])) / float(int(zones["count"][b, a, s])) - float(black[s])
              if full[b][a] else 0.0 for a in range(ux)] for b in range(uy)]
        filled = [row[:] for row in m]
        for b in range(uy):
            for a in range(ux):
                if not full[b][a]:
                    best = None
                    for b2 in range(uy):
                        for a2 in range(ux):
                            d = (a2 - a) ** 2 + (b2 - b) ** 2
                            if full[b2][a2] and (best is None or d < best[0]):
                                best = (d, m[b2][a2])
                    filled[b][a] = best[1]
        m = filled
        v = np.zeros((ny, nx))
        for j in range(ny):
            b, b1, ty = _locate(cy, float(j << ky))
            for i in range(nx):
                a, a1, tx = _locate(cx, float(i << kx))
                top = m[b][a] + (m[b][a1] - m[b][a]) * tx
                bot = m[b1][a] + (m[b1][a1] - m[b1][a]) * tx
                val = top + (bot - top) * ty
                if not val > 0.0:
                    return 0, unity
                v[j, i] = val
        vmax = float(v.max())
        for j in range(ny):
            for i in range(nx):
                gain = min(max(vmax / float(v[j, i]), 1.0), max_gain)
                out[s, j, i] = int(math.floor(gain * 4096.0 + 0.5))
    return 1, out


MAGIC = b"MISH"


def write_file(path, kx, ky, table, black):
    """the little-endian file bayer2rgb shading-file= names: MISH, u32 version = 1, kx, ky, nx, ny, black[4], the table"""
    table = np.asarray(table, np.uint16)
    _, ny, nx = table.shape
    with open(path, "wb") as f:
        f.write(MAGIC + np.array([1, kx, ky, nx, ny] + list(black), "<u4").tobytes() + table.astype("<u2").tobytes())
