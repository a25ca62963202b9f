"""NumPy model of the mosaic zone statistics and of the grey-world helper (include/mibayer.h, group `stats`): the
definition restated, for the CPU and GPU tests to compare the library against.

A sample S is the byte of an 8-bit mosaic or the 16-bit word in the given byte order masked to `bits`; site
s = 2 (y & 1) + (x & 1); a zone grid of zones_x x zones_y with cells of cw = 2 ceil((W/2) / zones_x) pixels by
ch = 2 ceil((H/2) / zones_y) rows (H/2 not rounded: the last row of an odd height has a zone too), pixel (x, y) in
zone (x // cw, y // ch); per zone and site the sum and the count of the samples with lo <= S <= hi and the number of
those with S > hi."""
import numpy as np

STATS_DTYPE = np.dtype([("sum", np.uint64, 4), ("count", np.uint32, 4), ("clipped", np.uint32, 4)])
# colour (0 = R, 1 = G, 2 = B) of site s per Bayer order: the map rgb2bayer uses
SITE_COLOUR = {"bggr": (2, 1, 1, 0), "gbrg": (1, 2, 0, 1), "grbg": (1, 0, 2, 1), "rggb": (0, 1, 1, 2)}


def cell(size, zones):
    """pixels (rows) of a zone along an axis of `size` pixels cut into `zones` zones"""
    return 2 * -(-((size + 1) // 2) // zones)


def samples(raw, width, height, stride, bits=0, big_endian=False):
    """(height, width) int64 samples of a frame given as bytes with `stride` bytes per row: padding and the bits above
    `bits` dropped"""
    rows = np.asarray(raw).view(np.uint8).reshape(-1)[:height * stride].reshape(height, stride)
    if bits == 0:
        return rows[:, :width].astype(np.int64)
    words = rows[:, :2 * width].reshape(height, width, 2).astype(np.int64)
    v = (words[..., 0] << 8 | words[..., 1]) if big_endian else (words[..., 1] << 8 | words[..., 0])
    return v & ((1 << bits) - 1)


def zone_stats(S, zones_x, zones_y, lo, hi):
    """(zones_y, zones_x) STATS_DTYPE of the (H, W) sample array S"""
    H, W = S.shape
    assert 1 <= zones_x <= min(64, W // 2) and 1 <= zones_y <= min(64, H // 2) and lo <= hi
    cw, ch = cell(W, zones_x), cell(H, zones_y)
    zone = (np.arange(H)[:, None] // ch) * zones_x + np.arange(W)[None, :] // cw
    out = np.zeros((zones_y, zones_x), STATS_DTYPE)
    n = zones_x * zones_y
    for s in range(4):
        v = S[s >> 1::2, s & 1::2].reshape(-1)
        z = zone[s >> 1::2, s & 1::2].reshape(-1)
        inside = (v >= lo) & (v <= hi)
        # float64 weights are exact here: a sum stays far below 2^53
        sums = np.bincount(z[inside], v[inside].astype(np.float64), n)
        out["sum"][..., s] = sums.astype(np.uint64).reshape(zones_y, zones_x)
        out["count"][..., s] = np.bincount(z[inside], minlength=n).reshape(zones_y, zones_x)
        out["clipped"][..., s] = np.bincount(z[v > hi], minlength=n).reshape(zones_y, zones_x)
    return out


def zone_stats_slow(S, zones_x, zones_y, lo, hi):
    """the same, pixel by pixel"""
    H, W = S.shape
    cw, ch = cell(W, zones_x), cell(H, zones_y)
    out = np.zeros((zones_y, zones_x), STATS_DTYPE)
    for y in range(H):
        for x in range(W):
            z = out[y // ch, x // cw]
            s, v = 2 * (y & 1) + (x & 1), int(S[y, x])
            if lo <= v <= hi:
                z["sum"][s] += np.uint64(v)
                z["count"][s] += 1
            elif v > hi:
                z["clipped"][s] += 1
    return out


def grey_world(zones, pattern, black=(0.0, 0.0, 0.0)):
    """(ok, gains): all zones pooled per colour, m_k = S_k / N_k - black_k; gains (m_G / m_R, 1, m_G / m_B) clamped to
    [1/16, 15.99], or (0, unit gains) when a colour has no samples or a mean is not positive"""
    zones = np.asarray(zones).reshape(-1)
    S, N = [0, 0, 0], [0, 0, 0]
    for s, k in enumerate(SITE_COLOUR[pattern]):
        S[k] += int(zones["sum"][:, s].astype(object).sum())
        N[k] += int(zones["count"][:, s].astype(object).sum())
    if 0 in N:
        return 0, (1.0, 1.0, 1.0)
    m = [float(S[k]) / float(N[k]) - float(black[k]) for k in range(3)]
    if min(m) <= 0:
        return 0, (1.0, 1.0, 1.0)
    clamp = lambda g: min(max(g, 1.0 / 16), 15.99)  # noqa: E731
    return 1, (clamp(m[1] / m[0]), 1.0, clamp(m[1] / m[2]))
