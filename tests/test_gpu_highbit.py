"""GPU tests of deep samples (include/mibayer.h, MIBAYER_FLAG_SRC_BITS): every entry point of a deep context against
the NumPy model of tests/highbit_model.py, and the full-size reference md5s through the 16-bit path."""
import hashlib
import json
import os

import numpy as np
import pytest

import highbit_model as hm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
LAYOUT8 = ("RGBx", "BGRx", "xRGB", "xBGR")
LAYOUT16 = ("RGBA64", "BGRA64", "ARGB64", "ABGR64")
# output arms: (out16, dst_big_endian)
OUTS = ((False, False), (True, False), (True, True))


def mosaic(rng, w, h, bits, stride=None, big_endian=False, junk=True):
    """random samples of `bits` bits, with random junk above them (must be ignored) -> (samples, frame bytes)"""
    S = rng.integers(0, 1 << bits, (h, w))
    words = S | (rng.integers(0, 1 << 16, (h, w)) & ~((1 << bits) - 1) & 0xFFFF) if junk else S
    buf = hm.pack(words, stride, big_endian)
    if stride and stride > 2 * w:
        buf[:, 2 * w:] = 0x5A                       # padding is not part of the frame
    return S, buf


def expect(buf, w, h, pattern, layout, bits, out16, sbe=False, dbe=False, stride=None):
    return hm.bayer2rgb_highbit(buf, w, h, pattern, layout, bits, out16, sbe, dbe, stride)


def layout_for(out16, k):
    return (LAYOUT16 if out16 else LAYOUT8)[k]


def test_every_depth_order_layout_and_byte_order(gpu_pkg):
    rng = np.random.default_rng(1)
    n = 0
    for bits in (10, 12, 14, 16):
        for sbe in (False, True):
            for pattern in ORDERS:
                w, h = (38, 11) if (n & 1) else (36, 9)      # both row tails: width % 4 == 2 and == 0
                _, buf = mosaic(rng, w, h, bits, big_endian=sbe)
                for out16, dbe in OUTS:
                    for k in range(4):
                        layout = layout_for(out16, k)
                        with gpu_pkg.Context(w, h, pattern, layout, bits=bits, src_big_endian=sbe, out16=out16,
                                             dst_big_endian=dbe, device=0) as ctx:
                            got = ctx.process_host(buf)
                        want = expect(buf, w, h, pattern, layout, bits, out16, sbe, dbe)
                        assert np.array_equal(got, want), (bits, sbe, pattern, out16, dbe, layout)
                n += 1
    # an 8-bit mosaic with 16-bit output (v << 8)
    for pattern in ORDERS:
        src = rng.integers(0, 256, (7, 40), dtype=np.uint8)
        for dbe in (False, True):
            for layout in LAYOUT16:
                with gpu_pkg.Context(38, 7, pattern, layout, out16=True, dst_big_endian=dbe, device=0) as ctx:
                    got = ctx.process_host(src)
                want = expect(src, 38, 7, pattern, layout, 8, True, sbe=False, dbe=dbe, stride=40)
                assert np.array_equal(got, want), (pattern, layout, dbe)


@pytest.mark.parametrize("w,h", [(4, 3), (6, 5), (3838, 2160), (1366, 768)])
def test_edge_geometries_and_padded_strides(gpu_pkg, w, h):
    rng = np.random.default_rng(w * 7 + h)
    for bits, pattern, layout, out16 in ((12, "grbg", "ARGB64", True), (10, "rggb", "BGRx", False),
                                         (16, "gbrg", "ABGR64", True)):
        for sstride, dstride in ((0, 0), (2 * w + 12, (8 if out16 else 4) * w + 24)):
            _, buf = mosaic(rng, w, h, bits, stride=sstride or None)
            with gpu_pkg.Context(w, h, pattern, layout, src_stride=sstride, dst_stride=dstride, bits=bits,
                                 device=0) as ctx:
                got = ctx.process_host(buf)
                row = (8 if out16 else 4) * w
                want = expect(buf, w, h, pattern, layout, bits, out16, stride=sstride or None)
                assert np.array_equal(got[:, :row], want), (bits, pattern, layout, sstride, dstride)
                assert (got[:, row:] == 0xA5).all()          # row padding of the destination untouched
                # device path, with guard bytes before and after the frame
                guard = 4096
                d_src = ctx.device_alloc(ctx.src_bytes)
                d_dst = ctx.device_alloc(ctx.dst_bytes + 2 * guard)
                try:
                    ctx.to_device(d_src, buf)
                    ctx.to_device(d_dst, np.full(ctx.dst_bytes + 2 * guard, 0x3C, np.uint8))
                    ctx.process_device(d_src, d_dst + guard, 1)
                    ctx.sync()
                    out = ctx.from_device(d_dst, ctx.dst_bytes + 2 * guard)
                finally:
                    ctx.device_free(d_src)
                    ctx.device_free(d_dst)
                assert (out[:guard] == 0x3C).all() and (out[-guard:] == 0x3C).all()
                frame = out[guard:-guard].reshape(h, ctx.dst_stride)
                assert np.array_equal(frame[:, :row], want) and (frame[:, row:] == 0x3C).all()


@pytest.mark.parametrize("flags", [0, 1])
def test_ring_submit_wait_order_and_tags(gpu_pkg, flags):
    """1080p at 8 B/px out: the host path cuts it into bands (16.6 MB >= the band threshold)"""
    rng = np.random.default_rng(3 + flags)
    w, h, n = 1920, 1080, 7
    frames = [mosaic(rng, w, h, 12, big_endian=True)[1] for _ in range(3)]
    with gpu_pkg.Context(w, h, "bggr", "ARGB64", bits=12, src_big_endian=True, inflight=3, flags=flags,
                         device=0) as ctx:
        outs = [np.zeros((h, ctx.dst_stride), np.uint8) for _ in range(n)]
        srcs = [np.ascontiguousarray(frames[i % 3]) for i in range(n)]
        got_tags = []
        for i in range(n):
            while ctx.pending() >= 3:
                got_tags.append(ctx.wait())
            ctx.submit(srcs[i], outs[i], tag=100 + i)
        while ctx.pending():
            got_tags.append(ctx.wait())
        assert got_tags == [100 + i for i in range(n)]
    wants = [expect(f, w, h, "bggr", "ARGB64", 12, True, sbe=True) for f in frames]
    for i in range(n):
        assert np.array_equal(outs[i], wants[i % 3]), i


def test_process_device_batch_and_list(gpu_pkg):
    rng = np.random.default_rng(11)
    w, h = 642, 50
    bufs = [mosaic(rng, w, h, 14)[1] for _ in range(18)]
    wants = [expect(b, w, h, "gbrg", "RGBA64", 14, True) for b in bufs]
    with gpu_pkg.Context(w, h, "gbrg", "RGBA64", bits=14, device=0) as ctx:
        # batch, frames padded apart on both sides
        sfb, dfb = ctx.src_bytes + 256, ctx.dst_bytes + 512
        n = 5
        d_src = ctx.device_alloc(n * sfb)
        d_dst = ctx.device_alloc(n * dfb)
        try:
            host = np.zeros((n, sfb), np.uint8)
            for f in range(n):
                host[f, :ctx.src_bytes] = bufs[f].reshape(-1)
            ctx.to_device(d_src, host)
            ctx.process_device(d_src, d_dst, n, src_frame_bytes=sfb, dst_frame_bytes=dfb)
            ctx.sync()
            out = ctx.from_device(d_dst, n * dfb).reshape(n, dfb)
            for f in range(n):
                assert np.array_equal(out[f, :ctx.dst_bytes].reshape(h, -1), wants[f]), f
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_dst)
        # list: 18 separate allocations -> two launches (16 + 2)
        srcs = [ctx.device_alloc(ctx.src_bytes) for _ in bufs]
        dsts = [ctx.device_alloc(ctx.dst_bytes) for _ in bufs]
        try:
            for d, b in zip(srcs, bufs):
                ctx.to_device(d, b)
            ctx.process_device_list(srcs, dsts)
            ctx.sync()
            for f, d in enumerate(dsts):
                assert np.array_equal(ctx.from_device(d, ctx.dst_bytes).reshape(h, -1), wants[f]), f
        finally:
            for d in srcs + dsts:
                ctx.device_free(d)
        # what a deep context does not have
        for call in (lambda: ctx.fill_synthetic(0x1000, 1, 1), lambda: ctx.set_plan(1, 1),
                     lambda: ctx.launch_geometry(1)):
            with pytest.raises(gpu_pkg.MibayerError) as e:
                call()
            assert e.value.status == gpu_pkg.ERR_ARG


def test_two_shard_pool_on_device_0(gpu_pkg):
    rng = np.random.default_rng(21)
    w, h, n = 640, 480, 8
    bufs = [mosaic(rng, w, h, 10)[1] for _ in range(n)]
    outs = [np.zeros((h, 4 * w), np.uint8) for _ in range(n)]
    with gpu_pkg.Pool([0, 0], w, h, "rggb", "xBGR", inflight=2, bits=10) as pool:
        done = []
        for i in range(n):
            while pool.pending() >= pool.capacity:
                done.append(pool.wait())
            pool.submit(bufs[i], outs[i], tag=i + 1)
        while pool.pending():
            done.append(pool.wait())
    assert done == list(range(1, n + 1))
    for i in range(n):
        assert np.array_equal(outs[i], expect(bufs[i], w, h, "rggb", "xBGR", 10, False)), i


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def test_known_md5_through_the_16bit_path(gpu_pkg):
    """every entry of tests/golden/known_md5.json: the 8-bit synthetic mosaic zero-extended to 16-bit words, bits=16,
    16-bit output -> the low byte of every channel (alpha 0xffff -> 0xff) has the reference's md5"""
    with open(os.path.join(ROOT, "tests", "golden", "known_md5.json")) as f:
        entries = json.load(f)["entries"]
    for e in entries:
        w, h = e["width"], e["height"]
        with gpu_pkg.Context(w, h, e["pattern"], e["format"], device=0) as c8:
            d8 = c8.device_alloc(c8.src_bytes)
            try:
                c8.fill_synthetic(d8, 1, e["seed"])
                c8.sync()
                src8 = c8.from_device(d8, c8.src_bytes)
            finally:
                c8.device_free(d8)
        assert md5(src8) == e["md5_input"], e
        words = src8.reshape(h, -1)[:, :w].astype("<u2")
        with gpu_pkg.Context(w, h, e["pattern"], e["format"], bits=16, out16=True, device=0) as ctx:
            d_src = ctx.device_alloc(ctx.src_bytes)
            d_dst = ctx.device_alloc(ctx.dst_bytes)
            try:
                ctx.to_device(d_src, words)
                ctx.process_device(d_src, d_dst, 1)
                ctx.sync()
                out = ctx.from_device(d_dst, ctx.dst_bytes)
            finally:
                ctx.device_free(d_src)
                ctx.device_free(d_dst)
        px = out.reshape(h, w, 4, 2)                        # little-endian words: [..., 0] = low byte
        alpha = 6 - sum(gpu_pkg.FORMATS[e["format"]])
        assert (px[:, :, alpha, 1] == 0xFF).all()
        assert (np.delete(px[..., 1], alpha, axis=2) == 0).all()
        assert md5(px[..., 0]) == e["md5_output"], e


def test_4k_12bit_batch_of_16(gpu_pkg):
    """one launch over 16 4K frames of 12-bit samples -> ARGB64; per frame: every border row and column and a seeded
    sample of rows against the model"""
    rng = np.random.default_rng(4096)
    w, h, n = 3840, 2160, 16
    with gpu_pkg.Context(w, h, "grbg", "ARGB64", bits=12, device=0) as ctx:
        d_src = ctx.device_alloc(n * ctx.src_bytes)
        d_dst = ctx.device_alloc(n * ctx.dst_bytes)
        try:
            samples = []
            for f in range(n):
                S, buf = mosaic(rng, w, h, 12)
                samples.append(S)
                ctx.to_device(d_src + f * ctx.src_bytes, buf)
            ctx.process_device(d_src, d_dst, n)
            ctx.sync()
            rows = np.unique(np.concatenate([[0, 1, 2, h - 3, h - 2, h - 1], rng.integers(0, h, 24)]))
            for f in range(n):
                out = ctx.from_device(d_dst + f * ctx.dst_bytes, ctx.dst_bytes).reshape(h, 8 * w)
                S = samples[f]
                want_rows = hm.to_output(hm.native_rgb(S, "grbg", rows), 12, "ARGB64", True)
                assert np.array_equal(out[rows], want_rows), f
                left = hm.to_output(hm.native_rgb(S[:, :12], "grbg"), 12, "ARGB64", True)[:, :8 * 8]
                right = hm.to_output(hm.native_rgb(S[:, -12:], "grbg"), 12, "ARGB64", True)[:, -8 * 8:]
                assert np.array_equal(out[:, :64], left), f
                assert np.array_equal(out[:, -64:], right), f
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_dst)
