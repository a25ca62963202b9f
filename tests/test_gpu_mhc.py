"""GPU tests of the Malvar-He-Cutler demosaic (include/mibayer.h, MIBAYER_FLAG_MHC): every entry point of an MHC
context, bit-exact against the NumPy model of tests/mhc_model.py."""
import numpy as np
import pytest

import highbit_model as hm
import mhc_model as mm

pytestmark = pytest.mark.gpu

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
LAYOUT8 = ("RGBx", "BGRx", "xRGB", "xBGR")
# output arms: (layout, out16, dst_big_endian)
OUTS = (("BGRx", False, False), ("ARGB64", True, False), ("ARGB64", True, True))


def mosaic8(rng, w, h, stride=None):
    stride = stride or ((w + 3) & ~3)
    buf = rng.integers(0, 256, (h, stride), dtype=np.uint8)
    buf[:, w:] = 0x5A
    return buf


def mosaic16(rng, w, h, bits, stride=None, big_endian=False):
    """random samples of `bits` bits with junk above them (must be ignored) -> frame bytes"""
    S = rng.integers(0, 1 << bits, (h, w))
    words = S | (rng.integers(0, 1 << 16, (h, w)) & ~((1 << bits) - 1) & 0xFFFF)
    buf = hm.pack(words, stride, big_endian)
    if stride and stride > 2 * w:
        buf[:, 2 * w:] = 0x5A
    return buf


def run_device(ctx, buf, guard=4096):
    """process_device of one frame into a buffer with guard bytes on both sides; checks the guards and the row padding,
    returns the frame's rows"""
    d_src = ctx.device_alloc(ctx.src_bytes)
    d_dst = ctx.device_alloc(ctx.dst_bytes + 2 * guard)
    try:
        ctx.to_device(d_src, np.ascontiguousarray(buf))
        ctx.to_device(d_dst, np.full(ctx.dst_bytes + 2 * guard, 0x3C, np.uint8))
        ctx.process_device(d_src, d_dst + guard, 1)
        ctx.sync()
        out = ctx.from_device(d_dst, ctx.dst_bytes + 2 * guard)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    assert (out[:guard] == 0x3C).all() and (out[-guard:] == 0x3C).all()
    return out[guard:-guard].reshape(ctx.height, ctx.dst_stride)


@pytest.mark.parametrize("w,h", [(4, 3), (6, 5), (36, 9), (38, 11)])
def test_8bit_every_order_and_layout(gpu_pkg, w, h):
    rng = np.random.default_rng(w * 31 + h)
    for pattern in ORDERS:
        buf = mosaic8(rng, w, h)
        for layout in LAYOUT8:
            want = mm.bayer2rgb_mhc(buf, w, h, pattern, layout, stride=buf.shape[1])
            with gpu_pkg.Context(w, h, pattern, layout, method="mhc", device=0) as ctx:
                assert ctx.method == "mhc"
                got = ctx.process_host(buf)
                assert np.array_equal(got, want), (pattern, layout, "host")
                assert np.array_equal(run_device(ctx, buf), want), (pattern, layout, "device")


def test_every_depth_byte_order_and_output(gpu_pkg):
    rng = np.random.default_rng(5)
    n = 0
    for bits in (8, 10, 12, 14, 16):
        for sbe in ((False,) if bits == 8 else (False, True)):
            for pattern in ORDERS:
                w, h = (38, 11) if (n & 1) else (36, 9)
                n += 1
                if bits == 8:
                    buf = mosaic8(rng, w, h)
                    stride = buf.shape[1]
                else:
                    buf = mosaic16(rng, w, h, bits, big_endian=sbe)
                    stride = None
                for layout, out16, dbe in OUTS:
                    deep = dict(bits=0 if bits == 8 else bits, src_big_endian=sbe, out16=out16, dst_big_endian=dbe)
                    want = mm.bayer2rgb_mhc(buf, w, h, pattern, layout, stride=stride, **deep)
                    with gpu_pkg.Context(w, h, pattern, layout, method="mhc", device=0, **deep) as ctx:
                        got = ctx.process_host(buf)
                    assert np.array_equal(got, want), (bits, sbe, pattern, layout, out16, dbe)


@pytest.mark.parametrize("w,h", [(3838, 2160), (1366, 768), (4056, 3040)])
def test_large_frames_padded_strides(gpu_pkg, w, h):
    rng = np.random.default_rng(w + h)
    for bits, pattern, layout, out16 in ((0, "rggb", "xRGB", False), (12, "grbg", "ARGB64", True),
                                         (10, "bggr", "BGRx", False)):
        px = 8 if out16 else 4
        sstride = (2 * w if bits else (w + 3) & ~3) + 12
        dstride = px * w + 24
        buf = mosaic16(rng, w, h, bits, stride=sstride) if bits else mosaic8(rng, w, h, stride=sstride)
        want = mm.bayer2rgb_mhc(buf, w, h, pattern, layout, bits=bits, out16=out16, stride=sstride)
        with gpu_pkg.Context(w, h, pattern, layout, src_stride=sstride, dst_stride=dstride, bits=bits, out16=out16,
                             method="mhc", device=0) as ctx:
            got = ctx.process_host(buf)
            assert np.array_equal(got[:, :px * w], want), (bits, layout, "host")
            assert (got[:, px * w:] == 0xA5).all()
            frame = run_device(ctx, buf)
            assert np.array_equal(frame[:, :px * w], want), (bits, layout, "device")
            assert (frame[:, px * w:] == 0x3C).all()


def test_banded_host_path_4k_8bit(gpu_pkg):
    """3840x2160 -> BGRx is 33 MB out: the host path cuts the frame into bands, each uploaded with its halo rows"""
    rng = np.random.default_rng(44)
    w, h = 3840, 2160
    buf = mosaic8(rng, w, h)
    want = mm.bayer2rgb_mhc(buf, w, h, "gbrg", "BGRx", stride=buf.shape[1])
    with gpu_pkg.Context(w, h, "gbrg", "BGRx", method="mhc", device=0) as ctx:
        for _ in range(2):
            assert np.array_equal(ctx.process_host(buf), want)


def test_banded_host_path_1080p_12bit_argb64(gpu_pkg):
    rng = np.random.default_rng(45)
    w, h = 1920, 1080
    buf = mosaic16(rng, w, h, 12)
    want = mm.bayer2rgb_mhc(buf, w, h, "rggb", "ARGB64", bits=12, out16=True)
    with gpu_pkg.Context(w, h, "rggb", "ARGB64", bits=12, method="mhc", device=0) as ctx:
        assert np.array_equal(ctx.process_host(buf), want)


@pytest.mark.parametrize("flags", [0, 1])
def test_ring_submit_wait_order_and_tags(gpu_pkg, flags):
    """inflight=3, with and without MIBAYER_FLAG_HIPGRAPH (the host path of an MHC context runs without graphs)"""
    rng = np.random.default_rng(3 + flags)
    w, h, n = 1920, 1080, 7
    frames = [mosaic16(rng, w, h, 12, big_endian=True) for _ in range(3)]
    with gpu_pkg.Context(w, h, "bggr", "ARGB64", bits=12, src_big_endian=True, inflight=3, flags=flags,
                         method="mhc", device=0) as ctx:
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
    wants = [mm.bayer2rgb_mhc(f, w, h, "bggr", "ARGB64", bits=12, out16=True, src_big_endian=True) for f in frames]
    for i in range(n):
        assert np.array_equal(outs[i], wants[i % 3]), i


@pytest.mark.parametrize("bits", [0, 14])
def test_process_device_batch_and_list(gpu_pkg, bits):
    rng = np.random.default_rng(11 + bits)
    w, h = 642, 50
    layout = "RGBA64" if bits else "RGBx"
    bufs = [mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h) for _ in range(18)]
    wants = [mm.bayer2rgb_mhc(b, w, h, "gbrg", layout, bits=bits, out16=bool(bits), stride=b.shape[1]) for b in bufs]
    with gpu_pkg.Context(w, h, "gbrg", layout, bits=bits, method="mhc", device=0) as ctx:
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
        for call in (lambda: ctx.set_plan(1, 1), lambda: ctx.launch_geometry(1)):
            with pytest.raises(gpu_pkg.MibayerError) as e:
                call()
            assert e.value.status == gpu_pkg.ERR_ARG
        assert ctx.variant_name.startswith("mhc")


def test_fill_synthetic_follows_the_source_depth(gpu_pkg):
    """an 8-bit MHC mosaic takes the synthetic generator (the bilinear context's bytes); a deep one refuses it"""
    w, h = 640, 480
    with gpu_pkg.Context(w, h, "bggr", "BGRx", device=0) as ref, \
            gpu_pkg.Context(w, h, "bggr", "BGRx", method="mhc", device=0) as ctx:
        d_a, d_b, d_out = ref.device_alloc(ref.src_bytes), ctx.device_alloc(ctx.src_bytes), ctx.device_alloc(ctx.dst_bytes)
        try:
            ref.fill_synthetic(d_a, 1, 9)
            ref.sync()
            ctx.fill_synthetic(d_b, 1, 9)
            ctx.process_device(d_b, d_out, 1)
            ctx.sync()
            src = ref.from_device(d_a, ref.src_bytes)
            assert np.array_equal(ctx.from_device(d_b, ctx.src_bytes), src)
            want = mm.bayer2rgb_mhc(src, w, h, "bggr", "BGRx", stride=ctx.src_stride)
            assert np.array_equal(ctx.from_device(d_out, ctx.dst_bytes).reshape(h, -1), want)
        finally:
            ref.device_free(d_a)
            ctx.device_free(d_b)
            ctx.device_free(d_out)
    with gpu_pkg.Context(w, h, "bggr", "BGRx", bits=12, method="mhc", device=0) as ctx:
        with pytest.raises(gpu_pkg.MibayerError) as e:
            ctx.fill_synthetic(0x1000, 1, 1)
        assert e.value.status == gpu_pkg.ERR_ARG


def test_two_shard_pool_on_device_0(gpu_pkg):
    rng = np.random.default_rng(21)
    w, h, n = 640, 480, 8
    for bits, layout, out16 in ((0, "xBGR", False), (10, "ABGR64", True)):
        bufs = [mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h) for _ in range(n)]
        px = 8 if out16 else 4
        outs = [np.zeros((h, px * w), np.uint8) for _ in range(n)]
        with gpu_pkg.Pool([0, 0], w, h, "rggb", layout, inflight=2, bits=bits, method="mhc") as pool:
            done = []
            for i in range(n):
                while pool.pending() >= pool.capacity:
                    done.append(pool.wait())
                pool.submit(bufs[i], outs[i], tag=i + 1)
            while pool.pending():
                done.append(pool.wait())
        assert done == list(range(1, n + 1))
        for i in range(n):
            want = mm.bayer2rgb_mhc(bufs[i], w, h, "rggb", layout, bits=bits, out16=out16)
            assert np.array_equal(outs[i], want), (bits, i)


@pytest.mark.parametrize("bits,layout", [(0, "BGRx"), (12, "ARGB64")])
def test_4k_batch_of_16(gpu_pkg, bits, layout):
    """one launch over 16 4K frames; per frame every border row and column and a seeded sample of rows"""
    rng = np.random.default_rng(4096 + bits)
    w, h, n = 3840, 2160, 16
    out16 = bits != 0
    px = 8 if out16 else 4
    depth = bits or 8
    with gpu_pkg.Context(w, h, "grbg", layout, bits=bits, method="mhc", device=0) as ctx:
        d_src = ctx.device_alloc(n * ctx.src_bytes)
        d_dst = ctx.device_alloc(n * ctx.dst_bytes)
        try:
            samples = []
            for f in range(n):
                buf = mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h)
                samples.append(mm.samples(buf, w, h, bits, stride=ctx.src_stride)[0])
                ctx.to_device(d_src + f * ctx.src_bytes, buf)
            ctx.process_device(d_src, d_dst, n)
            ctx.sync()
            rows = np.unique(np.concatenate([[0, 1, 2, 15, 16, 17, h - 3, h - 2, h - 1], rng.integers(0, h, 24)]))
            for f in range(n):
                out = ctx.from_device(d_dst + f * ctx.dst_bytes, ctx.dst_bytes).reshape(h, px * w)
                S = samples[f]
                want_rows = hm.to_output(mm.native_rgb(S, "grbg", depth, rows), depth, layout, out16)
                assert np.array_equal(out[rows], want_rows), f
                left = hm.to_output(mm.native_rgb(S[:, :12], "grbg", depth), depth, layout, out16)[:, :8 * px]
                right = hm.to_output(mm.native_rgb(S[:, -12:], "grbg", depth), depth, layout, out16)[:, -8 * px:]
                assert np.array_equal(out[:, :8 * px], left), f
                assert np.array_equal(out[:, -8 * px:], right), f
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_dst)
