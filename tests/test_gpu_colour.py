"""GPU tests of the fused colour stage (include/mibayer.h, MIBAYER_FLAG_COLOUR): every entry point of a colour context,
bit-exact against the NumPy model of tests/colour_model.py.  The matrix and the tone table come from the library's own
helpers (mibayer_colour_matrix / mibayer_colour_tone), so the model and the kernel multiply with the same integers."""
import ctypes
import threading

import numpy as np
import pytest

import colour_model as cm
import highbit_model as hm
import mhc_model as mm

pytestmark = pytest.mark.gpu

ORDERS = ("bggr", "gbrg", "grbg", "rggb")
LAYOUT8 = ("RGBx", "BGRx", "xRGB", "xBGR")
METHODS = ("bilinear", "mhc")
# output arms: (layout, out16, dst_big_endian)
OUTS = (("BGRx", False, False), ("ARGB64", True, False), ("ARGB64", True, True))
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)      # rows sum to 1


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


def make_colour(pkg, depth, curve="srgb", gains=(1.9, 1.0, 1.6), ccm=CCM, black=None):
    """a stage that exercises every step: black level at 1/16 of the range, gains, a CCM with negative entries, a curve"""
    black = (1 << depth) // 16 if black is None else black
    tone = {None: None, "srgb": pkg.TONE_SRGB, "linear": pkg.TONE_LINEAR, "gamma": pkg.TONE_GAMMA}[curve]
    return pkg.Colour.make(black=black, gains=gains, ccm=ccm, curve=tone)


def model_kw(col):
    return dict(black=tuple(col.black[:]), matrix=tuple(col.matrix[:]), tone=col.tone_table())


def run_device(ctx, buf, guard=4096):
    """process_device of one frame into a buffer with guard bytes on both sides; checks the guards, returns the rows"""
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


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("w,h", [(4, 3), (6, 5), (36, 9), (38, 20), (258, 33)])
def test_8bit_every_order_and_layout(gpu_pkg, method, w, h):
    rng = np.random.default_rng(w * 31 + h)
    col = make_colour(gpu_pkg, 8)
    for pattern in ORDERS:
        buf = mosaic8(rng, w, h)
        for layout in LAYOUT8:
            want = cm.bayer2rgb_colour(buf, w, h, pattern, layout, method=method, stride=buf.shape[1], **model_kw(col))
            with gpu_pkg.Context(w, h, pattern, layout, method=method, colour=col, device=0) as ctx:
                assert ctx.colour and ctx.method == method and ctx.variant_name.startswith("colour_" + method)
                got = ctx.process_host(buf)
                assert np.array_equal(got, want), (pattern, layout, "host")
                assert np.array_equal(run_device(ctx, buf), want), (pattern, layout, "device")


@pytest.mark.parametrize("method", METHODS)
@pytest.mark.parametrize("curve", [None, "srgb"])
def test_every_depth_byte_order_and_output(gpu_pkg, method, curve):
    rng = np.random.default_rng(5)
    n = 0
    for bits in (8, 10, 12, 14, 16):
        col = make_colour(gpu_pkg, bits, curve)
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
                    want = cm.bayer2rgb_colour(buf, w, h, pattern, layout, method=method, stride=stride,
                                               **deep, **model_kw(col))
                    with gpu_pkg.Context(w, h, pattern, layout, method=method, colour=col, device=0, **deep) as ctx:
                        got = ctx.process_host(buf)
                    assert np.array_equal(got, want), (bits, sbe, pattern, layout, out16, dbe)


@pytest.mark.parametrize("method", METHODS)
def test_identities_against_a_context_without_the_flag(gpu_pkg, method):
    """identity stage == the plain context's bytes (the 8-bit bilinear one is the production kernel); a linear tone
    curve on top leaves 16-bit output unchanged; and the plain context is what the parent computed (the models)"""
    rng = np.random.default_rng(77)
    w, h = 258, 37
    linear = gpu_pkg.Colour.make(curve=gpu_pkg.TONE_LINEAR)
    for bits, layout, out16 in ((0, "BGRx", False), (0, "RGBA64", True), (12, "xRGB", False), (12, "ARGB64", True),
                                (16, "ABGR64", True)):
        buf = mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h)
        with gpu_pkg.Context(w, h, "gbrg", layout, bits=bits, out16=out16, method=method, device=0) as plain:
            assert not plain.colour
            want = plain.process_host(buf)
        if method == "mhc":
            model = mm.bayer2rgb_mhc(buf, w, h, "gbrg", layout, bits=bits, out16=out16, stride=buf.shape[1])
        else:
            model = hm.bayer2rgb_highbit(buf, w, h, "gbrg", layout, bits or 8, out16, stride=buf.shape[1])
        assert np.array_equal(want, model), (bits, layout, "plain context")
        with gpu_pkg.Context(w, h, "gbrg", layout, bits=bits, out16=out16, method=method, colour=True, device=0) as ctx:
            got = ctx.get_colour()
            assert got.has_tone == 0 and got.matrix[:] == list(cm.IDENTITY) and got.black[:] == [0, 0, 0]
            assert np.array_equal(ctx.process_host(buf), want), (bits, layout, "identity")
            if out16:
                ctx.set_colour(linear)
                assert np.array_equal(ctx.process_host(buf), want), (bits, layout, "linear tone")


@pytest.mark.parametrize("w,h", [(3838, 2160), (4056, 3040)])
def test_large_frames_padded_strides_and_guards(gpu_pkg, w, h):
    rng = np.random.default_rng(w + h)
    for bits, pattern, layout, out16, method in ((0, "rggb", "xRGB", False, "bilinear"),
                                                 (12, "grbg", "ARGB64", True, "mhc"),
                                                 (10, "bggr", "BGRx", False, "bilinear")):
        col = make_colour(gpu_pkg, bits or 8)
        px = 8 if out16 else 4
        sstride = (2 * w if bits else (w + 3) & ~3) + 12
        dstride = px * w + 24
        buf = mosaic16(rng, w, h, bits, stride=sstride) if bits else mosaic8(rng, w, h, stride=sstride)
        want = cm.bayer2rgb_colour(buf, w, h, pattern, layout, bits=bits, out16=out16, method=method, stride=sstride,
                                   **model_kw(col))
        with gpu_pkg.Context(w, h, pattern, layout, src_stride=sstride, dst_stride=dstride, bits=bits, out16=out16,
                             method=method, colour=col, device=0) as ctx:
            got = ctx.process_host(buf)
            assert np.array_equal(got[:, :px * w], want), (bits, layout, "host")
            assert (got[:, px * w:] == 0xA5).all()
            frame = run_device(ctx, buf)
            assert np.array_equal(frame[:, :px * w], want), (bits, layout, "device")
            assert (frame[:, px * w:] == 0x3C).all()


@pytest.mark.parametrize("method", METHODS)
def test_banded_host_path_4k(gpu_pkg, method):
    """3840x2160 -> BGRx is 33 MB out: the host path cuts the frame into bands, each uploaded with its halo rows"""
    rng = np.random.default_rng(44)
    w, h = 3840, 2160
    col = make_colour(gpu_pkg, 8)
    buf = mosaic8(rng, w, h)
    want = cm.bayer2rgb_colour(buf, w, h, "gbrg", "BGRx", method=method, stride=buf.shape[1], **model_kw(col))
    with gpu_pkg.Context(w, h, "gbrg", "BGRx", method=method, colour=col, device=0) as ctx:
        for _ in range(2):
            assert np.array_equal(ctx.process_host(buf), want)


@pytest.mark.parametrize("flags", [0, 1])
def test_set_colour_between_frames_in_submission_order(gpu_pkg, flags):
    """frames queued before mibayer_set_colour keep the old parameters, tone table included; the next one has the new
    ones.  inflight=3, with and without MIBAYER_FLAG_HIPGRAPH (the host path of a colour context runs without graphs)"""
    rng = np.random.default_rng(3 + flags)
    w, h, n = 1920, 1080, 8
    cols = [make_colour(gpu_pkg, 12, "srgb"), make_colour(gpu_pkg, 12, "gamma", gains=(1.0, 1.3, 2.5), black=0),
            make_colour(gpu_pkg, 12, None, gains=(2.0, 1.0, 1.0), ccm=None)]
    frames = [mosaic16(rng, w, h, 12, big_endian=True) for _ in range(2)]
    with gpu_pkg.Context(w, h, "bggr", "ARGB64", bits=12, src_big_endian=True, inflight=3, flags=flags,
                         method="mhc", colour=True, device=0) as ctx:
        outs = [np.zeros((h, ctx.dst_stride), np.uint8) for _ in range(n)]
        srcs = [np.ascontiguousarray(frames[i % 2]) for i in range(n)]
        got_tags = []
        for i in range(n):
            while ctx.pending() >= 3:
                got_tags.append(ctx.wait())
            ctx.set_colour(cols[i % 3])                 # while up to two earlier frames are still in flight
            ctx.submit(srcs[i], outs[i], tag=100 + i)
        while ctx.pending():
            got_tags.append(ctx.wait())
        assert got_tags == [100 + i for i in range(n)]
    plain = [cm.plain_argb64(f, w, h, "bggr", 12, "mhc", src_big_endian=True)[0] for f in frames]
    for i in range(n):
        want = cm.colour(plain[i % 2], 12, "ARGB64", True, **model_kw(cols[i % 3]))
        assert np.array_equal(outs[i], want), i


@pytest.mark.parametrize("bits,method", [(0, "bilinear"), (14, "mhc"), (10, "bilinear")])
def test_process_device_batch_and_list(gpu_pkg, bits, method):
    rng = np.random.default_rng(11 + bits)
    w, h = 642, 50
    layout = "RGBA64" if bits else "RGBx"
    col = make_colour(gpu_pkg, bits or 8)
    bufs = [mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h) for _ in range(18)]
    wants = [cm.bayer2rgb_colour(b, w, h, "gbrg", layout, bits=bits, out16=bool(bits), method=method,
                                 stride=b.shape[1], **model_kw(col)) for b in bufs]
    with gpu_pkg.Context(w, h, "gbrg", layout, bits=bits, method=method, colour=col, device=0) as ctx:
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


BAD_STAGES = (("black", 0, -1), ("black", 2, 65536), ("matrix", 4, 65536), ("matrix", 8, -65536), ("tone", 256, 65537),
              ("tone", 0, 1 << 31), ("has_tone", None, 2), ("has_tone", None, -1), ("struct_size", None, 8))


def bad_stage(pkg, field, index, value):
    bad = pkg.Colour.make(black=3, gains=(2, 1, 1), curve=pkg.TONE_SRGB)
    if index is None:
        setattr(bad, field, value)
    else:
        getattr(bad, field)[index] = value
    return bad


def test_set_get_colour_argument_errors(gpu_pkg):
    """ERR_ARG on a context without the flag and on out-of-range values; a refused set leaves the stage as it was; the
    plan entry points refuse a colour context"""
    pkg = gpu_pkg
    L = pkg.lib()
    col = pkg.Colour()
    with pkg.Context(64, 48, device=0) as plain, pkg.Context(64, 48, method="mhc", device=0) as mhc:
        for ctx in (plain, mhc):
            assert L.mibayer_set_colour(ctx._h, ctypes.byref(col)) == pkg.ERR_ARG
            assert L.mibayer_get_colour(ctx._h, ctypes.byref(col)) == pkg.ERR_ARG
    with pkg.Context(64, 48, colour=True, device=0) as ctx:
        assert L.mibayer_set_colour(ctx._h, None) == pkg.ERR_ARG and L.mibayer_get_colour(ctx._h, None) == pkg.ERR_ARG
        good = pkg.Colour.make(black=3, gains=(2, 1, 1), curve=pkg.TONE_SRGB)
        ctx.set_colour(good)
        for field, index, value in BAD_STAGES:
            bad = bad_stage(pkg, field, index, value)
            assert L.mibayer_set_colour(ctx._h, ctypes.byref(bad)) == pkg.ERR_ARG, (field, index, value)
            assert bytes(ctx.get_colour()) == bytes(good), (field, index, value)
        # the edges of the ranges are inside; without a curve the table is not looked at
        edge = pkg.Colour(black=(0, 65535, 1), matrix=(65535, -65535, 0, 0, 4096, 0, 0, 0, 4096), tone=[65536] * 257)
        ctx.set_colour(edge)
        assert bytes(ctx.get_colour()) == bytes(edge)
        junk = pkg.Colour()
        junk.tone[7] = 1 << 30
        ctx.set_colour(junk)
        for call in (lambda: ctx.set_plan(1, 1), lambda: ctx.set_plan_for(1, 1, 1), lambda: ctx.launch_geometry(1),
                     lambda: ctx.autotune(0x1000, 0x2000, 1), lambda: ctx.autotune_list([0x1000], [0x2000])):
            with pytest.raises(pkg.MibayerError) as e:
                call()
            assert e.value.status == pkg.ERR_ARG
    # a pool: the same ranges, refused at once and without effect on the frames that follow
    w, h = 66, 20
    buf = mosaic8(np.random.default_rng(9), w, h)
    with pkg.Pool([0, 0], w, h, "bggr", "BGRx", inflight=2, colour=good) as pool:
        for field, index, value in BAD_STAGES:
            bad = bad_stage(pkg, field, index, value)
            assert L.mibayer_pool_set_colour(pool._h, ctypes.byref(bad)) == pkg.ERR_ARG, (field, index, value)
        assert L.mibayer_pool_set_colour(pool._h, None) == pkg.ERR_ARG
        out = np.zeros((h, 4 * w), np.uint8)
        pool.submit(buf, out, tag=1)
        assert pool.wait() == 1
    assert np.array_equal(out, cm.bayer2rgb_colour(buf, w, h, "bggr", "BGRx", stride=buf.shape[1], **model_kw(good)))


def test_a_banded_frame_never_mixes_two_stages(gpu_pkg):
    """a 4K host-path frame is launched band by band; another thread keeps switching the stage meanwhile.  Every frame
    must come out wholly in one of the two stages (it takes one copy when it is accepted)"""
    rng = np.random.default_rng(46)
    w, h = 3840, 2160
    cols = [make_colour(gpu_pkg, 8, None, gains=(2.0, 1.0, 1.0), ccm=None, black=0),
            make_colour(gpu_pkg, 8, "srgb", gains=(1.0, 1.0, 2.0), ccm=None, black=8)]
    buf = mosaic8(rng, w, h)
    plain = cm.plain_argb64(buf, w, h, "rggb", 0, "bilinear", stride=buf.shape[1])[0]
    wants = [cm.colour(plain, 8, "BGRx", False, **model_kw(c)) for c in cols]
    assert not np.array_equal(wants[0][:16], wants[1][:16]) and not np.array_equal(wants[0][-16:], wants[1][-16:])
    stop = threading.Event()
    with gpu_pkg.Context(w, h, "rggb", "BGRx", colour=cols[0], device=0) as ctx:
        def switch():
            k = 0
            while not stop.is_set():
                k ^= 1
                ctx.set_colour(cols[k])
        t = threading.Thread(target=switch)
        t.start()
        try:
            outs = [ctx.process_host(buf).copy() for _ in range(12)]
        finally:
            stop.set()
            t.join()
    for i, out in enumerate(outs):
        assert np.array_equal(out, wants[0]) or np.array_equal(out, wants[1]), i


def test_pool_set_colour_with_frames_still_queued(gpu_pkg):
    """The stage changes before EVERY submit while earlier frames are still in flight or waiting in a shard's helper
    thread (pageable buffers: the helpers submit on their own time).  Frame i must come out with the stage the pool held
    when it was submitted."""
    rng = np.random.default_rng(22)
    w, h, n = 1920, 1080, 12
    for bits, layout, out16, method in ((0, "xBGR", False, "bilinear"), (12, "ABGR64", True, "mhc")):
        d = bits or 8
        cols = [make_colour(gpu_pkg, d), make_colour(gpu_pkg, d, None, gains=(1.0, 2.0, 1.0)),
                make_colour(gpu_pkg, d, "gamma", gains=(1.5, 1.0, 1.0), ccm=None, black=0)]
        bufs = [mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h) for _ in range(3)]
        px = 8 if out16 else 4
        outs = [np.zeros((h, px * w), np.uint8) for _ in range(n)]
        with gpu_pkg.Pool([0, 0], w, h, "rggb", layout, inflight=2, bits=bits, method=method, colour=True) as pool:
            done = []
            for i in range(n):
                while pool.pending() >= pool.capacity:
                    done.append(pool.wait())
                if i >= 2:                              # frames 0 and 1: the identity a new pool holds
                    pool.set_colour(cols[i % 3])
                pool.submit(bufs[i % 3], outs[i], tag=i + 1)
            while pool.pending():
                done.append(pool.wait())
        assert done == list(range(1, n + 1))
        plain = [cm.plain_argb64(b, w, h, "rggb", bits, method)[0] for b in bufs]
        for i in range(n):
            kw = model_kw(cols[i % 3]) if i >= 2 else {}
            want = cm.colour(plain[i % 3], d, layout, out16, **kw)
            assert np.array_equal(outs[i], want), (bits, i)


def test_two_shard_pool_on_device_0(gpu_pkg):
    rng = np.random.default_rng(21)
    w, h, n = 640, 480, 8
    for bits, layout, out16, method in ((0, "xBGR", False, "bilinear"), (10, "ABGR64", True, "mhc")):
        cols = [make_colour(gpu_pkg, bits or 8), make_colour(gpu_pkg, bits or 8, None, gains=(1.0, 2.0, 1.0))]
        bufs = [mosaic16(rng, w, h, bits) if bits else mosaic8(rng, w, h) for _ in range(n)]
        px = 8 if out16 else 4
        outs = [np.zeros((h, px * w), np.uint8) for _ in range(n)]
        with gpu_pkg.Pool([0, 0], w, h, "rggb", layout, inflight=2, bits=bits, method=method, colour=cols[0]) as pool:
            done = []
            for i in range(n):
                while pool.pending() >= pool.capacity:
                    done.append(pool.wait())
                if i == n // 2:
                    pool.set_colour(cols[1])            # with frames of the first half still in flight
                pool.submit(bufs[i], outs[i], tag=i + 1)
            while pool.pending():
                done.append(pool.wait())
        assert done == list(range(1, n + 1))
        for i in range(n):
            want = cm.bayer2rgb_colour(bufs[i], w, h, "rggb", layout, bits=bits, out16=out16, method=method,
                                       **model_kw(cols[i >= n // 2]))
            assert np.array_equal(outs[i], want), (bits, i)
    with gpu_pkg.Pool([0, 0], w, h, "rggb", "BGRx", inflight=2) as pool:
        with pytest.raises(gpu_pkg.MibayerError) as e:
            pool.set_colour(cols[0])
        assert e.value.status == gpu_pkg.ERR_ARG
