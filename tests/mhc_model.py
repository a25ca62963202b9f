"""TEST INFRASTRUCTURE: NumPy model of the Malvar-He-Cutler demosaic (include/mibayer.h, MIBAYER_FLAG_MHC).

Written from the formula, not from the kernel: the samples of highbit_model (8-bit bytes, or 16-bit words masked to
`bits`), reflect-101 borders (np.pad mode="reflect"), the four MHC filters scaled by 16, v = clamp((acc + 8) >> 4,
0, 2^depth - 1) on int32-range sums, then highbit_model.to_output."""
import numpy as np

from highbit_model import PATTERNS, pack, to_output, unpack  # noqa: F401  (pack: re-exported for the tests)

# colour of the top-left 2x2 sites, raster order (the site map of rgb2bayer)
SITES = {"bggr": "BGGR", "gbrg": "GBRG", "grbg": "GRBG", "rggb": "RGGB"}


def _filter(taps):
    k = np.zeros((5, 5), np.int64)
    for (dy, dx), w in taps.items():
        k[dy + 2, dx + 2] = w
    assert k.sum() == 16
    return k


def _sym(base):
    """taps given for one sign expanded over every sign combination of (dy, dx)"""
    out = {}
    for (dy, dx), w in base.items():
        for sy in (1, -1):
            for sx in (1, -1):
                out[(sy * dy, sx * dx)] = w
    return out


F_G = _filter(_sym({(0, 0): 8, (0, 1): 4, (1, 0): 4, (0, 2): -2, (2, 0): -2}))
F_ROW = _filter(_sym({(0, 0): 10, (0, 1): 8, (0, 2): -2, (1, 1): -2, (2, 0): 1}))
F_COL = F_ROW.T.copy()
F_DIAG = _filter(_sym({(0, 0): 12, (1, 1): 4, (0, 2): -3, (2, 0): -3}))


def site_map(pattern, H, W):
    """(H, W) array of 'R' / 'G' / 'B'."""
    if not isinstance(pattern, str):
        pattern = {v: k for k, v in PATTERNS.items()}[int(pattern)]
    s = SITES[pattern]
    tile = np.array([[s[0], s[1]], [s[2], s[3]]])
    return np.tile(tile, ((H + 1) // 2, (W + 1) // 2))[:H, :W]


def correlate(S, k, rows=None):
    """sum over (dy, dx) of k[dy+2, dx+2] * S(y+dy, x+dx), reflect-101 borders; rows: only these output rows"""
    H, W = S.shape
    P = np.pad(S.astype(np.int64), 2, mode="reflect")
    rows = np.arange(H) if rows is None else np.asarray(rows)
    acc = np.zeros((rows.size, W), np.int64)
    for dy in range(5):
        for dx in range(5):
            if k[dy, dx]:
                acc += k[dy, dx] * P[rows + dy, dx:dx + W]
    return acc


def native_rgb(S, pattern, depth, rows=None):
    """(H, W) masked samples -> (H, W, 3) int64 (R, G, B) at the native depth; rows: only these output rows
    (-> (len(rows), W, 3))"""
    S = np.asarray(S).astype(np.int64)
    H, W = S.shape
    if W < 4 or W % 2 or H < 3:
        raise ValueError("outside the defined domain")
    vmax = (1 << depth) - 1

    rows = np.arange(H) if rows is None else np.asarray(rows)

    def f(k):
        return np.clip((correlate(S, k, rows) + 8) >> 4, 0, vmax)

    sites = site_map(pattern, H, W)[rows]
    fg, frow, fcol, fdiag = f(F_G), f(F_ROW), f(F_COL), f(F_DIAG)
    # the colour of the non-green sites of each row: a G site takes it from its left/right neighbours (F_row)
    row_colour = np.where((sites == "R").any(axis=1), "R", "B")[:, None]
    S = S[rows]
    R = np.where(sites == "R", S, np.where(sites == "B", fdiag, np.where(row_colour == "R", frow, fcol)))
    B = np.where(sites == "B", S, np.where(sites == "R", fdiag, np.where(row_colour == "B", frow, fcol)))
    G = np.where(sites == "G", S, fg)
    return np.stack([R, G, B], axis=-1)


def samples(src, width, height, bits, src_big_endian=False, stride=None):
    """Frame bytes -> ((H, W) int64 masked samples, depth); bits 0 / 8 = the 8-bit mosaic."""
    if bits in (0, 8):
        stride = width if stride is None else stride
        raw = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)[:stride * height].reshape(height, stride)
        return raw[:, :width].astype(np.int64), 8
    return unpack(src, width, height, stride, bits, src_big_endian), bits


def bayer2rgb_mhc(src, width, height, pattern, offsets, bits=0, out16=False, src_big_endian=False,
                  dst_big_endian=False, stride=None):
    """Frame bytes -> output rows (bytes): (H, 4W) for the 4-byte formats, (H, 8W) for 16-bit channels."""
    S, depth = samples(src, width, height, bits, src_big_endian, stride)
    return to_output(native_rgb(S, pattern, depth), depth, offsets, out16, dst_big_endian)
