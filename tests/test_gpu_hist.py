"""GPU tests of the mosaic histogram (include/mibayer.h, group `hist`): mosaic_hist_kernel through mibayer_hist_device,
the host path (mibayer_set_hist / mibayer_frame_hist) and the pool, bit-exact against the NumPy model of
tests/hist_model.py -- every value is an integer count, whatever the order of the kernel's atomics.

The kernel's boundaries (csrc/mibayer_internal.h, mosaic_hist_kernel): a lane reads one dword = 4 columns of an 8-bit
mosaic or 2 of a deep one; a wave spans 64 dwords = 256 / 128 columns; a workgroup 256 dwords = 1024 / 512 columns;
the row loop is kHistAhead = 8 deep; a workgroup walks kHistMinRows = 16 rows of a small launch, more (up to
kHistMaxRows = 256) once the launch has kHistSpread = 512 workgroups."""
import numpy as np
import pytest

import hist_model as hm
from test_gpu_stats import frame8, frame16

pytestmark = pytest.mark.gpu

# W = 4, 6: one lane, whole and half a dword; 254, 258: either side of a wave (258 % 4 == 2); 1022, 1026, 1030: either
# side of a workgroup's strip
WIDTHS8 = (4, 6, 254, 256, 258, 1022, 1024, 1026, 1030)
WIDTHS16 = (4, 6, 126, 128, 130, 510, 512, 514)
# 3, 4, 5: the smallest; 7, 8, 9: either side of the row loop; 15, 16, 17, 33: either side of one and two workgroups' rows
HEIGHTS = (3, 4, 5, 7, 8, 9, 15, 16, 17, 33)


def same(got, want):
    assert got.shape == want.shape and got.dtype == want.dtype
    assert np.array_equal(got, want), np.argwhere(got != want)[:8]


def windows(W, H):
    """the whole frame; 2 x 1 and 2 x 2 at the origin and at the last even column / last row; x0 = 2 (mod 4); a window
    ending on the last row; an odd y0"""
    wins = [(0, 0, 0, 0), (0, 0, 2, 1), (W - 2, H - 1, 2, 1), (0, H - 1, W, 1)]
    if H >= 2:
        wins += [(0, 0, 2, 2), (W - 2, H - 2, 2, 2), (0, 1, W, H - 1)]
    if W >= 6 and H >= 3:
        wins += [(2, 1, W - 4, H - 2), (2, H - 3, 4, 3)]
    return wins


@pytest.mark.parametrize("W", WIDTHS8)
def test_8bit_geometries_and_windows(gpu_pkg, W):
    rng = np.random.default_rng(W)
    for H in HEIGHTS:
        raw = frame8(rng, W, H)
        S = hm.samples(raw, W, H, raw.shape[1])
        with gpu_pkg.Context(W, H, "rggb", "RGBx", device=0) as ctx:
            for win in windows(W, H) if H in (3, 5, 9, 17) else [(0, 0, 0, 0)]:
                same(ctx.hist_batch_via_device(raw[None], win)[0], hm.histogram(S, 8, win))


@pytest.mark.parametrize("bits,big_endian", [(10, False), (12, False), (16, False), (12, True)])
def test_deep_samples(gpu_pkg, bits, big_endian):
    rng = np.random.default_rng(bits + big_endian)
    for W in WIDTHS16:
        for H in (3, 5, 9, 17):
            stride = 2 * W + 8 if W == 130 else 0        # 0xFF in the padding (frame16)
            raw = frame16(rng, W, H, bits, big_endian, stride or None)      # junk above `bits`
            S = hm.samples(raw, W, H, raw.shape[1], bits, big_endian)
            with gpu_pkg.Context(W, H, "grbg", "ARGB64", src_stride=stride, device=0, bits=bits,
                                 src_big_endian=big_endian) as ctx:
                for win in windows(W, H) if H == 5 else [(0, 0, 0, 0)]:
                    same(ctx.hist_batch_via_device(raw[None], win)[0], hm.histogram(S, bits, win))


def test_rows_per_workgroup_above_the_minimum(gpu_pkg):
    """5 strips x 2100 rows: 2100 * 5 / 512 = 20 rows per workgroup, and 2100 = 105 * 20 exactly; 2110: a short last one"""
    W = 4100
    rng = np.random.default_rng(11)
    for H in (2100, 2110):
        raw = frame8(rng, W, H)
        with gpu_pkg.Context(W, H, device=0) as ctx:
            same(ctx.hist_batch_via_device(raw[None])[0], hm.histogram(hm.samples(raw, W, H, W), 8))


def test_rows_per_workgroup_at_the_maximum(gpu_pkg):
    """8 strips x 1030 rows x 16 frames / 512 = 257: every workgroup walks 256 rows, the last of a frame 6"""
    W, H, n = 8192, 1030, 16
    base = frame8(np.random.default_rng(12), W, H)
    raw = np.stack([base ^ np.uint8(17 * f) for f in range(n)])
    with gpu_pkg.Context(W, H, device=0) as ctx:
        got = ctx.hist_batch_via_device(raw)
    for f in range(n):
        same(got[f], hm.histogram(raw[f].astype(np.int64), 8))


@pytest.mark.parametrize("kind", ["constant", "per-site", "ramp"])
def test_contents(gpu_pkg, kind):
    W, H = 1030, 37
    raw = np.zeros((H, (W + 3) & ~3), np.uint8)
    if kind == "constant":              # one bin per site takes everything: the contention worst case
        raw[:] = 200
    elif kind == "per-site":            # a site mix-up moves a count
        for s in range(4):
            raw[s >> 1::2, s & 1::2] = 10 + 50 * s
    else:                               # all 256 bins
        raw[:] = (np.arange(raw.shape[1])[None, :] + 3 * np.arange(H)[:, None]) & 0xFF
    raw[:, W:] = 0xEE
    with gpu_pkg.Context(W, H, device=0) as ctx:
        got = ctx.hist_batch_via_device(raw[None])[0]
    same(got, hm.histogram(hm.samples(raw, W, H, raw.shape[1]), 8))
    if kind == "constant":
        assert got[:, 200].tolist() == [515 * 19, 515 * 19, 515 * 18, 515 * 18] and int(got.sum()) == W * H
    if kind == "per-site":
        assert [int(got[s, 10 + 50 * s]) for s in range(4)] == [515 * 19, 515 * 19, 515 * 18, 515 * 18]
    if kind == "ramp":
        assert (got.sum(axis=0) > 0).all()


def test_constant_deep_frame(gpu_pkg):
    W, H, bits = 514, 17, 12
    raw = np.full((H, W), 0xFFFF, np.uint16).view(np.uint8)             # 4095 under junk: the last bin
    with gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=bits) as ctx:
        got = ctx.hist_batch_via_device(raw[None])[0]
    assert got[:, 255].tolist() == [257 * 9, 257 * 9, 257 * 8, 257 * 8] and int(got.sum()) == W * H


def test_padded_stride_offset_base_and_pitched_batch(gpu_pkg):
    W, H, stride, n = 266, 18, 320, 3
    rng = np.random.default_rng(2)
    raws = [frame8(rng, W, H, stride, pad=0x5A) for _ in range(n)]
    wants = np.stack([hm.histogram(hm.samples(r, W, H, stride), 8, (2, 1, 262, 16)) for r in raws])
    pitch = raws[0].size + 64
    padded = np.full((n, pitch), 0xFF, np.uint8)
    padded[:, :raws[0].size] = np.stack(raws).reshape(n, -1)
    with gpu_pkg.Context(W, H, src_stride=stride, device=0) as ctx:
        same(ctx.hist_batch_via_device(padded, (2, 1, 262, 16), src_frame_bytes=pitch), wants)
        # the batch at 4 mod 16 inside its allocation
        same(ctx.hist_batch_via_device(padded, (2, 1, 262, 16), src_frame_bytes=pitch, src_offset=4), wants)
        d_src, d_hist = ctx.device_alloc(n * pitch), ctx.device_alloc(n * 4096)
        try:
            ctx.to_device(d_src, padded)
            for _ in range(2):          # the second call zeroes again: the same counts, not doubled
                ctx.hist_device(d_src, d_hist, (2, 1, 262, 16), n, pitch)
            ctx.sync()
            same(ctx.from_device(d_hist, n * 4096).view(np.uint32).reshape(n, 4, 256), wants)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_hist)


@pytest.mark.parametrize("kind", ["mhc", "colour", "rgb24", "planar"])
def test_other_contexts(gpu_pkg, kind):
    W, H = 130, 18
    raw = frame8(np.random.default_rng(3), W, H)
    kw = {"mhc": dict(fmt="RGBx", method="mhc"), "colour": dict(fmt="RGBx", colour=gpu_pkg.Colour.make(black=16)),
          "rgb24": dict(fmt="RGB"), "planar": dict(fmt="GBR")}[kind]
    fmt = kw.pop("fmt")
    with gpu_pkg.Context(W, H, "gbrg", fmt, device=0, **kw) as ctx:
        same(ctx.hist_batch_via_device(raw[None], (2, 1, 124, 15))[0],
             hm.histogram(hm.samples(raw, W, H, raw.shape[1]), 8, (2, 1, 124, 15)))


def test_argument_errors(gpu_pkg):
    L = gpu_pkg.lib()
    W, H = 66, 19

    def rc(ctx, d_src, d_hist, win=(0, 0, 0, 0), n=1, pitch=None):
        return L.mibayer_hist_device(ctx._h, d_src, pitch or ctx.src_bytes, n, *win, d_hist, ctx.stream)

    with gpu_pkg.Context(W, H, device=0) as ctx, \
            gpu_pkg.Context(W, H, "bggr", "ARGB", device=0, flags=gpu_pkg.FLAG_RGB2BAYER) as inv:
        d_src, d_hist = ctx.device_alloc(4 * W * H * 2), ctx.device_alloc(2 * 4096)
        try:
            E = gpu_pkg.ERR_ARG
            assert rc(ctx, d_src, d_hist) == gpu_pkg.OK and rc(inv, d_src, d_hist) == E
            for win in ((1, 0, 2, 1), (0, 0, 3, 1), (0, 0, 0, 1), (0, 0, 2, 0), (-2, 0, 2, 1), (0, -1, 2, 1),
                        (66, 0, 2, 1), (0, 19, 2, 1), (2, 0, 66, 1), (0, 1, 2, 19), (0, 0, 68, 19), (0, 0, 66, 20)):
                assert rc(ctx, d_src, d_hist, win) == E, win
            for win in ((64, 18, 2, 1), (0, 0, 66, 19), (2, 1, 64, 18)):
                assert rc(ctx, d_src, d_hist, win) == gpu_pkg.OK, win
            assert rc(ctx, d_src + 2, d_hist) == E and rc(ctx, d_src, d_hist + 2) == E
            assert rc(ctx, None, d_hist) == E and rc(ctx, d_src, None) == E and rc(ctx, d_src, d_hist, n=-1) == E
            assert rc(ctx, d_src, d_hist, n=0) == gpu_pkg.OK
            assert rc(ctx, d_src, d_hist, n=2, pitch=ctx.src_bytes - 4) == gpu_pkg.ERR_GEOMETRY
            assert rc(ctx, d_src, d_hist, n=2, pitch=ctx.src_bytes + 2) == gpu_pkg.ERR_GEOMETRY
            ctx.sync()
            assert L.mibayer_set_hist(inv._h, 1, 0, 0, 0, 0) == E and L.mibayer_set_hist(ctx._h, 1, 1, 0, 2, 1) == E
            assert L.mibayer_set_hist(ctx._h, 1, 0, 0, 68, 1) == E
            assert L.mibayer_set_hist(ctx._h, 0, 1, 1, 1, 1) == gpu_pkg.OK      # off: the window is not looked at
            assert L.mibayer_frame_hist(ctx._h, np.zeros((4, 256), np.uint32).ctypes.data) == gpu_pkg.ERR_EMPTY
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_hist)


def test_host_path_sync_ring_and_stats_together(gpu_pkg):
    import stats_model as sm
    from test_gpu_stats import same as same_zones
    W, H = 258, 37
    rng = np.random.default_rng(5)
    raws = [frame8(rng, W, H) for _ in range(5)]
    win = (2, 1, 254, 35)
    wants = [hm.histogram(hm.samples(r, W, H, r.shape[1]), 8, win) for r in raws]
    with gpu_pkg.Context(W, H, "gbrg", "BGRx", device=0, inflight=3) as ctx:
        plain = [ctx.process_host(r).copy() for r in raws]
        with pytest.raises(gpu_pkg.MibayerError):
            ctx.frame_hist()            # histograms are off: MIBAYER_ERR_EMPTY
        ctx.set_hist(True, win)
        for r, p, w in zip(raws, plain, wants):
            assert np.array_equal(ctx.process_host(r), p)      # the converted bytes do not change
            same(ctx.frame_hist(), w)
        # a 3-deep ring: the histogram of each frame, in order
        dsts = [np.zeros_like(plain[0]) for _ in raws]
        got = []
        for i in range(len(raws) + 3):
            if i >= 3:
                assert ctx.wait() == i - 3 + 1
                got.append(ctx.frame_hist())
            if i < len(raws):
                ctx.submit(raws[i].reshape(-1), dsts[i], tag=i + 1)
        for g, w, d, p in zip(got, wants, dsts, plain):
            same(g, w)
            assert np.array_equal(d, p)
        # statistics as well, and the whole frame from now on
        ctx.set_stats(4, 3, 8, 247)
        ctx.set_hist(True)
        assert np.array_equal(ctx.process_host(raws[1]), plain[1])
        same(ctx.frame_hist(), hm.histogram(hm.samples(raws[1], W, H, raws[1].shape[1]), 8))
        same_zones(ctx.frame_stats(), sm.zone_stats(sm.samples(raws[1], W, H, raws[1].shape[1]), 4, 3, 8, 247))
        # histograms off again, statistics still on
        ctx.set_hist(False)
        assert np.array_equal(ctx.process_host(raws[2]), plain[2])
        assert gpu_pkg.lib().mibayer_frame_hist(ctx._h, np.zeros((4, 256), np.uint32).ctypes.data) == gpu_pkg.ERR_EMPTY
        same_zones(ctx.frame_stats(), sm.zone_stats(sm.samples(raws[2], W, H, raws[2].shape[1]), 4, 3, 8, 247))


def test_host_path_bands_count_each_row_once(gpu_pkg):
    """2048 x 2048 BGRx = 16 MiB of output, synchronous: uploaded and launched in bands with halo rows"""
    W = H = 2048
    raw = frame8(np.random.default_rng(6), W, H)
    want = hm.histogram(hm.samples(raw, W, H, W), 8)
    with gpu_pkg.Context(W, H, "rggb", "BGRx", device=0) as ctx, \
            gpu_pkg.Context(W, H, "rggb", "BGRx", device=0, flags=gpu_pkg.FLAG_HIPGRAPH) as graph:
        plain = ctx.process_host(raw).copy()
        for c in (ctx, graph):
            c.set_hist(True)
            assert np.array_equal(c.process_host(raw), plain)
            got = c.frame_hist()
            same(got, want)
            assert int(got.sum()) == W * H


def test_pool_two_shards_in_submission_order(gpu_pkg):
    W, H, n = 258, 37, 7
    rng = np.random.default_rng(8)
    raws = [frame8(rng, W, H) for _ in range(n)]
    wants = [hm.histogram(hm.samples(r, W, H, r.shape[1]), 8) for r in raws]
    with gpu_pkg.Context(W, H, device=0) as ctx:
        plain = [ctx.process_host(r).copy() for r in raws]
    with gpu_pkg.Pool([0, 0], W, H, inflight=2) as pool:
        with pytest.raises(gpu_pkg.MibayerError):
            pool.set_hist(True, (1, 0, 2, 1))
        pool.set_hist(True)
        dsts = [np.zeros_like(plain[0]) for _ in raws]
        done = 0
        for i in range(n):
            if pool.pending() == pool.capacity:
                assert pool.wait() == done + 1
                same(pool.frame_hist(), wants[done])
                done += 1
            pool.submit(raws[i].reshape(-1), dsts[i], tag=i + 1)
        while pool.pending():
            assert pool.wait() == done + 1
            same(pool.frame_hist(), wants[done])
            done += 1
        assert done == n and all(np.array_equal(d, p) for d, p in zip(dsts, plain))
        with pytest.raises(gpu_pkg.MibayerError):
            pool.frame_stats()          # zones were never asked for
        # a window and zones together, then off again: the next frame has none
        pool.set_stats(1, 1, 0, 255)
        pool.set_hist(True, (2, 1, 4, 3))
        pool.submit(raws[0].reshape(-1), dsts[0], tag=1)
        pool.wait()
        same(pool.frame_hist(), hm.histogram(hm.samples(raws[0], W, H, raws[0].shape[1]), 8, (2, 1, 4, 3)))
        assert int(pool.frame_stats()["count"].sum()) == W * H
        pool.set_hist(False)
        pool.submit(raws[0].reshape(-1), dsts[0], tag=1)
        pool.wait()
        with pytest.raises(gpu_pkg.MibayerError):
            pool.frame_hist()
        assert int(pool.frame_stats()["count"].sum()) == W * H


def test_pool_failover_redo_keeps_the_histograms(gpu_pkg):
    W, H, n = 66, 18, 6
    rng = np.random.default_rng(9)
    raws = [frame8(rng, W, H) for _ in range(n)]
    wants = [hm.histogram(hm.samples(r, W, H, r.shape[1]), 8) for r in raws]
    with gpu_pkg.Pool([0, 0], W, H, inflight=2) as pool:
        pool.set_hist(True)
        pool.inject_fault(1, 0)         # shard 1 reports a device error for its first frame: redone on shard 0
        dsts = [np.zeros((H, 4 * W), np.uint8) for _ in raws]
        done = 0

        def collect():
            nonlocal done
            assert pool.wait() == done + 1
            same(pool.frame_hist(), wants[done])
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
