"""TEST INFRASTRUCTURE: NumPy model of the fused colour stage (include/mibayer.h, MIBAYER_FLAG_COLOUR).

Written from the header's formula, not from the kernel.  The stage has no counterpart in the reference, so this model
is its oracle.  Input is the PLAIN result of the same cfg without the flag as little-endian ARGB64 (highbit_model /
mhc_model); the native-depth channels come back by >> (16 - depth) -- the plain 16-bit output is v << (16 - depth) --
then, per pixel, in exact integers (int64 here):
  1. c = max(c - black[k], 0)
  2. acc_k = m[3k] R + m[3k+1] G + m[3k+2] B;  c'_k = clamp((acc_k + 2048) >> 12, 0, 2^depth - 1)
  3. tone curve (optional): t = c' << (16 - depth), i = t >> 8, f = t & 255,
     o = min((tone[i] (256 - f) + tone[i+1] f + 128) >> 8, 65535); 16-bit channels o, 8-bit channels o >> 8;
     without one the deep path's conversion: c' << (16 - depth) or c' >> (depth - 8)
  4. alpha and layouts as highbit_model.to_output.
The matrix and the tone table are inputs: GPU tests take them from the library's helpers."""
import numpy as np

import highbit_model as hm
import mhc_model as mm

IDENTITY = (4096, 0, 0, 0, 4096, 0, 0, 0, 4096)


def plain_argb64(src, width, height, pattern, bits=0, method="bilinear", src_big_endian=False, stride=None):
    """the same cfg without the flag -> (H, 8W) bytes of little-endian ARGB64, and the native depth"""
    depth = bits or 8
    if method == "mhc":
        rows = mm.bayer2rgb_mhc(src, width, height, pattern, "ARGB64", bits=bits, out16=True,
                                src_big_endian=src_big_endian, stride=stride)
    else:
        rows = hm.bayer2rgb_highbit(src, width, height, pattern, "ARGB64", depth, True,
                                    src_big_endian=src_big_endian, stride=stride)
    return rows, depth


def native_from_argb64(rows, depth):
    """(H, 8W) little-endian ARGB64 bytes -> (H, W, 3) int64 (R, G, B) at the native depth"""
    rows = np.ascontiguousarray(rows)
    H = rows.shape[0]
    px = rows.view("<u2").reshape(H, -1, 4).astype(np.int64)
    return px[..., 1:4] >> (16 - depth)


def stage(rgb, depth, black=(0, 0, 0), matrix=IDENTITY, tone=None, out16=False):
    """(H, W, 3) native values -> (H, W, 3) int64 values at the OUTPUT depth (16-bit or 8-bit channels)"""
    vmax = (1 << depth) - 1
    c = np.maximum(np.asarray(rgb).astype(np.int64) - np.asarray(black, np.int64).reshape(1, 1, 3), 0)
    m = np.asarray(matrix, np.int64).reshape(3, 3)
    acc = (c[..., None, :] * m[None, None, :, :]).sum(axis=-1)          # acc[..., k] = sum_j m[k, j] c[..., j]
    c2 = np.clip((acc + 2048) >> 12, 0, vmax)
    if tone is None:
        return c2 << (16 - depth) if out16 else c2 >> (depth - 8)
    tone = np.asarray(tone, np.int64)
    assert tone.shape == (257,)
    t = c2 << (16 - depth)
    i, f = t >> 8, t & 255
    o = np.minimum((tone[i] * (256 - f) + tone[i + 1] * f + 128) >> 8, 65535)
    return o if out16 else o >> 8


def pack(values, offsets, out16, dst_big_endian=False):
    """(H, W, 3) values at output depth -> output rows as bytes, alpha 0xffff / 0xff"""
    r_off, g_off, b_off = hm.LAYOUTS[offsets] if isinstance(offsets, str) else offsets
    H, W, _ = values.shape
    out = np.full((H, W, 4), 0xFFFF if out16 else 0xFF, np.int64)
    out[..., r_off] = values[..., 0]
    out[..., g_off] = values[..., 1]
    out[..., b_off] = values[..., 2]
    dt = (">u2" if dst_big_endian else "<u2") if out16 else np.uint8
    return np.ascontiguousarray(out.astype(dt)).view(np.uint8).reshape(H, -1)


def colour(plain_rows, depth, offsets, out16, black=(0, 0, 0), matrix=IDENTITY, tone=None, dst_big_endian=False):
    """plain little-endian ARGB64 rows -> the colour context's output rows (bytes)"""
    return pack(stage(native_from_argb64(plain_rows, depth), depth, black, matrix, tone, out16), offsets, out16,
                dst_big_endian)


def bayer2rgb_colour(src, width, height, pattern, offsets, bits=0, out16=False, method="bilinear", black=(0, 0, 0),
                     matrix=IDENTITY, tone=None, src_big_endian=False, dst_big_endian=False, stride=None):
    """Frame bytes -> output rows (bytes) of a MIBAYER_FLAG_COLOUR context"""
    rows, depth = plain_argb64(src, width, height, pattern, bits, method, src_big_endian, stride)
    return colour(rows, depth, offsets, out16, black, matrix, tone, dst_big_endian)
