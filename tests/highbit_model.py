"""TEST INFRASTRUCTURE: NumPy model of bayer2rgb on deep samples (include/mibayer.h, MIBAYER_FLAG_SRC_BITS).

The closed form of oracle/bayer2rgb_np.py -- E/O lines with their edge columns, the up()/dn() row maps, the
double-rounded green of merge_bg / merge_gr -- on wide integers:
  input   one 16-bit word per sample (little- or big-endian), masked to its low `bits` bits (bits = 8: an 8-bit mosaic);
  average avg(a, b) = (a + b + 1) >> 1 on the masked values, at the native depth;
  output  16-bit channels: v << (16 - bits), alpha 0xffff, little- or big-endian words;
          8-bit channels (the 4-byte formats): v >> (bits - 8), alpha 255.
It lives under tests/ because oracle/ is frozen; with 8-bit-valued input the native result equals the 8-bit oracle's."""
import numpy as np

PATTERNS = {"bggr": 0, "gbrg": 1, "grbg": 2, "rggb": 3}
# (r, g, b) offsets: bytes of the 4-byte formats, 16-bit channels of the 8-byte ones
LAYOUTS = {
    "RGBx": (0, 1, 2), "RGBA": (0, 1, 2), "BGRx": (2, 1, 0), "BGRA": (2, 1, 0),
    "xRGB": (1, 2, 3), "ARGB": (1, 2, 3), "xBGR": (3, 2, 1), "ABGR": (3, 2, 1),
    "RGBA64": (0, 1, 2), "BGRA64": (2, 1, 0), "ARGB64": (1, 2, 3), "ABGR64": (3, 2, 1),
}


def avg(a, b):
    return (a + b + 1) >> 1


def unpack(buf, width, height, stride=None, bits=16, big_endian=False):
    """Frame bytes (height rows of `stride` bytes, 2 bytes per sample) -> (height, width) int64 masked samples."""
    stride = 2 * width if stride is None else stride
    raw = np.frombuffer(np.ascontiguousarray(buf).tobytes(), np.uint8)[:stride * height].reshape(height, stride)
    words = raw[:, :2 * width].copy().view(">u2" if big_endian else "<u2").astype(np.int64)
    return words & ((1 << bits) - 1)


def pack(samples, stride=None, big_endian=False):
    """(height, width) integer samples -> frame bytes (height, stride) uint8, 16-bit words, padding zero."""
    S = np.asarray(samples)
    H, W = S.shape
    stride = 2 * W if stride is None else stride
    out = np.zeros((H, stride), np.uint8)
    out[:, :2 * W] = np.ascontiguousarray(S.astype(">u2" if big_endian else "<u2")).view(np.uint8).reshape(H, 2 * W)
    return out


def horizontal_lines(S):
    H, W = S.shape
    left = np.empty_like(S)
    right = np.empty_like(S)
    left[:, 1:] = S[:, :-1]
    left[:, 0] = S[:, 1]
    right[:, :-1] = S[:, 1:]
    right[:, -1] = S[:, -2]
    A = avg(left, right)
    E = S.copy()
    O = S.copy()
    E[:, 1::2] = A[:, 1::2]
    O[:, 0::2] = A[:, 0::2]
    E[:, W - 1] = S[:, W - 2]
    O[:, 0] = S[:, 1]
    O[:, W - 2] = S[:, W - 3]
    return E, O


def row_maps(H):
    up = np.arange(H) - 1
    up[0] = 1
    dn = np.arange(H) + 1
    dn[H - 1] = H - 4 if H >= 4 else 1
    return up, dn


def native_rgb(S, pattern, rows=None):
    """(H, W) masked samples -> (H, W, 3) int64 (R, G, B) at the native depth; rows: only these output rows
    (-> (len(rows), W, 3)), from the source rows they need."""
    if isinstance(pattern, str):
        pattern = PATTERNS[pattern]
    H, W = np.shape(S)
    if W < 4 or W % 2 or H < 3:
        raise ValueError("outside the defined domain")
    swap_rb = pattern in (PATTERNS["rggb"], PATTERNS["gbrg"])
    swap_rows = pattern in (PATTERNS["grbg"], PATTERNS["gbrg"])
    rows = np.arange(H) if rows is None else np.asarray(rows)
    up, dn = row_maps(H)
    need = np.unique(np.concatenate([up[rows], rows, dn[rows]]))
    slot = np.zeros(H, np.int64)
    slot[need] = np.arange(need.size)
    E, O = horizontal_lines(np.asarray(S)[need].astype(np.int64))
    u, j, d = slot[up[rows]], slot[rows], slot[dn[rows]]
    VE, VO = avg(E[u], E[d]), avg(O[u], O[d])
    E, O = E[j], O[j]
    even_x = (np.arange(W) % 2 == 0)[None, :]
    g_bg = np.where(even_x, avg(VE, O), O)
    g_gr = np.where(even_x, E, avg(VO, E))
    T = ((rows & 1) ^ int(swap_rows)).astype(bool)[:, None]
    b_prime = np.where(T, VE, E)
    r_prime = np.where(T, O, VO)
    G = np.where(T, g_gr, g_bg)
    R, B = (b_prime, r_prime) if swap_rb else (r_prime, b_prime)
    return np.stack([R, G, B], axis=-1)


def to_output(rgb, bits, offsets, out16, dst_big_endian=False):
    """(H, W, 3) native values -> output rows as bytes: (H, 8W) for 16-bit channels, (H, 4W) for 8-bit ones."""
    r_off, g_off, b_off = LAYOUTS[offsets] if isinstance(offsets, str) else offsets
    H, W, _ = rgb.shape
    if out16:
        out = np.full((H, W, 4), 0xFFFF, np.int64)
        v = rgb << (16 - bits)
        dt = ">u2" if dst_big_endian else "<u2"
    else:
        out = np.full((H, W, 4), 0xFF, np.int64)
        v = rgb >> (bits - 8)
        dt = np.uint8
    out[..., r_off] = v[..., 0]
    out[..., g_off] = v[..., 1]
    out[..., b_off] = v[..., 2]
    return np.ascontiguousarray(out.astype(dt)).view(np.uint8).reshape(H, -1)


def bayer2rgb_highbit(src, width, height, pattern, offsets, bits, out16, src_big_endian=False,
                      dst_big_endian=False, stride=None):
    """Frame bytes -> output rows (bytes).  bits = 0 or 8: an 8-bit mosaic (one byte per sample, stride >= width)."""
    if bits in (0, 8):
        stride = width if stride is None else stride
        raw = np.frombuffer(np.ascontiguousarray(src).tobytes(), np.uint8)[:stride * height].reshape(height, stride)
        S, depth = raw[:, :width].astype(np.int64), 8
    else:
        S, depth = unpack(src, width, height, stride, bits, src_big_endian), bits
    return to_output(native_rgb(S, pattern), depth, offsets, out16, dst_big_endian)
