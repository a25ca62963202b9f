"""GPU tests of the mosaic zone statistics (include/mibayer.h, group `stats`): mosaic_stats_kernel through
mibayer_stats_device, the host path (mibayer_set_stats / mibayer_frame_stats) and the pool, bit-exact against the
NumPy model of tests/stats_model.py -- every value is an integer sum, whatever the order of the kernel's atomics."""
import numpy as np
import pytest

import stats_model as sm

pytestmark = pytest.mark.gpu

WIDTHS = (4, 6, 66, 258, 266, 1026)     # one lane; a half dword; a 2-column tail; past one wave / one workgroup strip
HEIGHTS = (3, 5, 18, 37)                # odd rows, less than / more than one group of rows in flight


def same(got, want):
    for f in ("sum", "count", "clipped"):
        assert np.array_equal(got[f], want[f]), (f, got[f].reshape(-1, 4)[:4], want[f].reshape(-1, 4)[:4])


def frame8(rng, W, H, stride=None, pad=0xFF):
    stride = stride or (W + 3) & ~3
    raw = np.full((H, stride), pad, np.uint8)
    raw[:, :W] = rng.integers(0, 256, (H, W))
    return raw


def frame16(rng, W, H, bits, big_endian, stride=None):
    """words with junk above `bits`, in the given byte order, 0xFF in the row padding"""
    stride = stride or 2 * W
    words = rng.integers(0, 1 << 16, (H, W)).astype(np.uint16)
    words[0, :2] = ((1 << bits) - 1, 0xFFFF << bits & 0xFFFF)          # max and 0 under junk
    raw = np.full((H, stride), 0xFF, np.uint8)
    raw[:, :2 * W] = words.astype(">u2" if big_endian else "<u2").view(np.uint8).reshape(H, 2 * W)
    return raw


@pytest.mark.parametrize("W", WIDTHS)
def test_8bit_geometries(gpu_pkg, W):
    rng = np.random.default_rng(W)
    for H in HEIGHTS:
        raw = frame8(rng, W, H)
        S = sm.samples(raw, W, H, raw.shape[1])
        with gpu_pkg.Context(W, H, "rggb", "RGBx", device=0) as ctx:
            for zx, zy in ((1, 1), (3, 5)):
                zx, zy = min(zx, W // 2), min(zy, H // 2)
                got = ctx.stats_batch_via_device(raw[None], zx, zy, 16, 239)[0]
                same(got, sm.zone_stats(S, zx, zy, 16, 239))


def test_64x64_zones_with_empty_trailing_ones(gpu_pkg):
    W, H = 258, 130
    raw = frame8(np.random.default_rng(1), W, H)
    with gpu_pkg.Context(W, H, device=0) as ctx:
        got = ctx.stats_batch_via_device(raw[None], 64, 64, 1, 254)[0]
    want = sm.zone_stats(sm.samples(raw, W, H, raw.shape[1]), 64, 64, 1, 254)
    same(got, want)
    assert sm.cell(W, 64) == 6 and not got["count"][:, 43:].any() and not got["count"][33:].any()


def test_padded_stride_and_offset_base(gpu_pkg):
    W, H, stride = 266, 18, 320
    rng = np.random.default_rng(2)
    raw = frame8(rng, W, H, stride)
    want = sm.zone_stats(sm.samples(raw, W, H, stride), 3, 5, 0, 200)
    with gpu_pkg.Context(W, H, src_stride=stride, device=0) as ctx:
        same(ctx.stats_batch_via_device(raw[None], 3, 5, 0, 200)[0], want)
        # the frame at 4 mod 16 inside an allocation
        d_buf = ctx.device_alloc(raw.size + 16)
        d_stats = ctx.device_alloc(15 * 64)
        try:
            assert d_buf % 16 == 0
            ctx.to_device(d_buf + 4, raw)
            ctx.stats_device(d_buf + 4, d_stats, 3, 5, 0, 200)
            ctx.sync()
            same(ctx.from_device(d_stats, 15 * 64).view(sm.STATS_DTYPE).reshape(5, 3), want)
        finally:
            ctx.device_free(d_buf)
            ctx.device_free(d_stats)


@pytest.mark.parametrize("bits", (10, 12, 16))
@pytest.mark.parametrize("big_endian", (False, True))
def test_deep_samples(gpu_pkg, bits, big_endian):
    rng = np.random.default_rng(bits + big_endian)
    vmax = (1 << bits) - 1
    for W, H, stride in ((6, 5, 0), (130, 18, 0), (258, 37, 544)):
        raw = frame16(rng, W, H, bits, big_endian, stride or None)
        S = sm.samples(raw, W, H, raw.shape[1], bits, big_endian)
        with gpu_pkg.Context(W, H, "grbg", "ARGB64", src_stride=stride, device=0, bits=bits,
                             src_big_endian=big_endian) as ctx:
            for zx, zy, lo, hi in ((1, 1, 0, vmax), (3, 2, vmax // 16, vmax - vmax // 16)):
                same(ctx.stats_batch_via_device(raw[None], zx, zy, lo, hi)[0], sm.zone_stats(S, zx, zy, lo, hi))


@pytest.mark.parametrize("lo,hi", [(0, 255), (0, 0), (77, 77), (255, 255)])
def test_range_extremes(gpu_pkg, lo, hi):
    W, H = 66, 18
    raw = frame8(np.random.default_rng(3), W, H)
    raw[0, :3] = (0, 77, 255)
    with gpu_pkg.Context(W, H, device=0) as ctx:
        got = ctx.stats_batch_via_device(raw[None], 3, 3, lo, hi)[0]
    same(got, sm.zone_stats(sm.samples(raw, W, H, raw.shape[1]), 3, 3, lo, hi))


def test_sums_need_64_bits(gpu_pkg):
    """520 x 520 samples of 0xFFFF: 67 600 per site, x 65 535 > 2^32"""
    W = H = 520
    raw = np.full((H, 2 * W), 0xFF, np.uint8)
    with gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=16) as ctx:
        got = ctx.stats_batch_via_device(raw[None], 1, 1, 0, 65535)[0]
    assert got["sum"][0, 0].tolist() == [67600 * 65535] * 4 and 67600 * 65535 > 1 << 32
    assert got["count"][0, 0].tolist() == [67600] * 4 and not got["clipped"].any()


def test_batch_junk_prefill_and_repeat(gpu_pkg):
    W, H, n = 258, 37, 3
    rng = np.random.default_rng(4)
    raw = np.stack([frame8(rng, W, H) for _ in range(n)])
    pitch = raw[0].size + 64            # a frame pitch larger than the frame
    padded = np.full((n, pitch), 0xFF, np.uint8)
    padded[:, :raw[0].size] = raw.reshape(n, -1)
    want = np.stack([sm.zone_stats(sm.samples(raw[f], W, H, raw.shape[2]), 4, 3, 10, 250) for f in range(n)])
    with gpu_pkg.Context(W, H, device=0) as ctx:
        same(ctx.stats_batch_via_device(padded, 4, 3, 10, 250, src_frame_bytes=pitch), want)   # d_stats held 0xA5 junk
        d_src, d_stats = ctx.device_alloc(n * pitch), ctx.device_alloc(n * 12 * 64)
        try:
            ctx.to_device(d_src, padded)
            for _ in range(2):          # the second call zeroes again: the same zones, not doubled
                ctx.stats_device(d_src, d_stats, 4, 3, 10, 250, n, pitch)
            ctx.sync()
            same(ctx.from_device(d_stats, n * 12 * 64).view(sm.STATS_DTYPE).reshape(n, 3, 4), want)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_stats)


def test_argument_errors(gpu_pkg):
    L = gpu_pkg.lib()
    W, H = 66, 18

    def rc(ctx, d_src, d_stats, zx=1, zy=1, lo=0, hi=255, n=1, pitch=None):
        return L.mibayer_stats_device(ctx._h, d_src, pitch or ctx.src_bytes, n, zx, zy, lo, hi, d_stats, ctx.stream)

    with gpu_pkg.Context(W, H, device=0) as ctx, gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=10) as deep, \
            gpu_pkg.Context(W, H, "bggr", "ARGB", device=0, flags=gpu_pkg.FLAG_RGB2BAYER) as inv:
        d_src, d_stats = ctx.device_alloc(4 * W * H * 2), ctx.device_alloc(64 * 64 * 64)
        try:
            E = gpu_pkg.ERR_ARG
            assert rc(ctx, d_src, d_stats) == gpu_pkg.OK
            assert rc(inv, d_src, d_stats) == E
            assert rc(ctx, d_src, d_stats, lo=5, hi=4) == E
            assert rc(ctx, d_src, d_stats, hi=256) == E and rc(deep, d_src, d_stats, hi=1024) == E
            assert rc(deep, d_src, d_stats, hi=1023) == gpu_pkg.OK
            for zx, zy in ((0, 1), (1, 0), (0, 0), (65, 1), (1, 65), (34, 1), (1, 10), (-1, 1)):
                assert rc(ctx, d_src, d_stats, zx, zy) == E, (zx, zy)
            assert rc(ctx, d_src, d_stats, 33, 9) == gpu_pkg.OK
            assert rc(ctx, d_src + 2, d_stats) == E and rc(ctx, d_src, d_stats + 4) == E
            assert rc(ctx, None, d_stats) == E and rc(ctx, d_src, None) == E and rc(ctx, d_src, d_stats, n=-1) == E
            assert rc(ctx, d_src, d_stats, n=2, pitch=ctx.src_bytes - 4) == gpu_pkg.ERR_GEOMETRY
            assert rc(ctx, d_src, d_stats, n=2, pitch=ctx.src_bytes + 2) == gpu_pkg.ERR_GEOMETRY
            ctx.sync(), deep.sync()
            # the host-path setters check the same things
            assert L.mibayer_set_stats(inv._h, 1, 1, 0, 255) == E and L.mibayer_set_stats(ctx._h, 1, 1, 9, 8) == E
            assert L.mibayer_set_stats(ctx._h, 34, 1, 0, 255) == E and L.mibayer_set_stats(ctx._h, 1, 1, 0, 256) == E
            out = np.zeros(1, sm.STATS_DTYPE)
            assert L.mibayer_frame_stats(ctx._h, out.ctypes.data, 1) == gpu_pkg.ERR_EMPTY
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_stats)


def test_host_path_sync_and_ring(gpu_pkg, oracle):
    W, H = 258, 37
    rng = np.random.default_rng(5)
    raws = [frame8(rng, W, H) for _ in range(5)]
    wants = [sm.zone_stats(sm.samples(r, W, H, r.shape[1]), 4, 3, 8, 247) for r in raws]
    with gpu_pkg.Context(W, H, "gbrg", "BGRx", device=0, inflight=3) as ctx:
        plain = [ctx.process_host(r).copy() for r in raws]
        with pytest.raises(gpu_pkg.MibayerError):
            ctx.frame_stats()           # statistics are off: MIBAYER_ERR_EMPTY
        ctx.set_stats(4, 3, 8, 247)
        for r, p, w in zip(raws, plain, wants):
            assert np.array_equal(ctx.process_host(r), p)      # the converted bytes do not change
            same(ctx.frame_stats(), w)
        # a 3-deep ring: the zones of each frame, in order
        dsts = [np.zeros_like(plain[0]) for _ in raws]
        got = []
        for i in range(len(raws) + 3):
            if i >= 3:
                assert ctx.wait() == i - 3 + 1
                got.append(ctx.frame_stats())
            if i < len(raws):
                ctx.submit(raws[i].reshape(-1), dsts[i], tag=i + 1)
        for g, w, d, p in zip(got, wants, dsts, plain):
            same(g, w)
            assert np.array_equal(d, p)
        # another grid for the frames accepted from now on; off again
        ctx.set_stats(1, 1, 0, 255)
        ctx.process_host(raws[0])
        same(ctx.frame_stats(), sm.zone_stats(sm.samples(raws[0], W, H, raws[0].shape[1]), 1, 1, 0, 255))
        ctx.set_stats(0, 0)
        ctx.process_host(raws[0])
        assert gpu_pkg.lib().mibayer_frame_stats(ctx._h, np.zeros(1, sm.STATS_DTYPE).ctypes.data, 1) == gpu_pkg.ERR_EMPTY


def test_host_path_bands_count_each_row_once(gpu_pkg):
    """3840 x 2160 synchronous: the frame is uploaded and launched in bands with halo rows"""
    W, H = 3840, 2160
    raw = frame8(np.random.default_rng(6), W, H)
    with gpu_pkg.Context(W, H, "rggb", "RGBx", device=0) as ctx, \
            gpu_pkg.Context(W, H, "rggb", "RGBx", device=0, flags=gpu_pkg.FLAG_HIPGRAPH) as graph:
        plain = ctx.process_host(raw).copy()
        for c in (ctx, graph):
            c.set_stats(32, 32, 16, 239)
            assert np.array_equal(c.process_host(raw), plain)
            got = c.frame_stats()
            same(got, sm.zone_stats(sm.samples(raw, W, H, W), 32, 32, 16, 239))
            assert int(got["count"].sum()) + int(got["clipped"].sum()) + int((raw < 16).sum()) == W * H


def test_colour_context_host_stats(gpu_pkg):
    """a COLOUR + MHC deep context: the statistics are those of the mosaic, whatever the stage does"""
    W, H, bits = 130, 18, 12
    raw = frame16(np.random.default_rng(7), W, H, bits, False)
    col = gpu_pkg.Colour.make(black=64, gains=(2.0, 1.0, 1.5))
    with gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=bits, method="mhc", colour=col) as ctx:
        plain = ctx.process_host(raw.reshape(-1)).copy()
        ctx.set_stats(2, 2, 64, 3839)
        assert np.array_equal(ctx.process_host(raw.reshape(-1)), plain)
        same(ctx.frame_stats(), sm.zone_stats(sm.samples(raw, W, H, 2 * W, bits), 2, 2, 64, 3839))


def test_pool_two_shards_in_submission_order(gpu_pkg):
    W, H, n = 258, 37, 7
    rng = np.random.default_rng(8)
    raws = [frame8(rng, W, H) for _ in range(n)]
    wants = [sm.zone_stats(sm.samples(r, W, H, r.shape[1]), 3, 2, 1, 254) for r in raws]
    with gpu_pkg.Context(W, H, device=0) as ctx:
        plain = [ctx.process_host(r).copy() for r in raws]
    with gpu_pkg.Pool([0, 0], W, H, inflight=2) as pool:
        with pytest.raises(gpu_pkg.MibayerError):
            pool.set_stats(200, 1, 0, 255)
        pool.set_stats(3, 2, 1, 254)
        dsts = [np.zeros_like(plain[0]) for _ in raws]
        done = 0
        for i in range(n):
            if pool.pending() == pool.capacity:
                assert pool.wait() == done + 1
                same(pool.frame_stats(), wants[done])
                done += 1
            pool.submit(raws[i].reshape(-1), dsts[i], tag=i + 1)
        while pool.pending():
            assert pool.wait() == done + 1
            same(pool.frame_stats(), wants[done])
            done += 1
        assert done == n and all(np.array_equal(d, p) for d, p in zip(dsts, plain))
        # off again: the next frame has none
        pool.set_stats(0, 0)
        pool.submit(raws[0].reshape(-1), dsts[0], tag=1)
        pool.wait()
        with pytest.raises(gpu_pkg.MibayerError):
            pool.frame_stats()


def test_pool_failover_redo_keeps_the_zones(gpu_pkg):
    W, H, n = 66, 18, 6
    rng = np.random.default_rng(9)
    raws = [frame8(rng, W, H) for _ in range(n)]
    wants = [sm.zone_stats(sm.samples(r, W, H, r.shape[1]), 2, 2, 0, 255) for r in raws]
    with gpu_pkg.Pool([0, 0], W, H, inflight=2) as pool:
        pool.set_stats(2, 2, 0, 255)
        pool.inject_fault(1, 0)         # shard 1 reports a device error for its first frame: redone on shard 0
        dsts = [np.zeros((H, 4 * W), np.uint8) for _ in raws]
        done = 0

        def collect():
            nonlocal done
            assert pool.wait() == done + 1
            same(pool.frame_stats(), wants[done])
            done += 1

        for i in range(n):
            while True:
                # the capacity shrinks with the dropped shard, and the survivor's ring may be full before the pool is
                if pool.pending() >= gpu_pkg.lib().mibayer_pool_capacity(pool._h):
                    collect()
                    continue
                try:
                    pool.submit(raws[i].reshape(-1), dsts[i], tag=i + 1)
                    break
                except gpu_pkg.MibayerError as e:
                    assert e.status == gpu_pkg.ERR_BUSY
                    collect()
        while pool.pending():
            collect()
        assert done == n and pool.alive() == 1
