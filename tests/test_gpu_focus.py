"""GPU tests of the mosaic focus statistics (include/mibayer.h, group `focus`): mosaic_focus_kernel through
mibayer_focus_device, byte for byte against the NumPy model of tests/focus_model.py -- every value is an integer sum,
whatever the order of the kernel's atomics.  Context.focus_batch_via_device puts guards around the mosaic and the zones
and checks that all of them, and the mosaic, come back untouched: every test here is a test of "read-only" too."""
import numpy as np
import pytest

import focus_cases as fc
import focus_model as fm

pytestmark = pytest.mark.gpu

# one lane; a half dword; three dwords; past a wave; past a workgroup strip, without and with a 2-column tail; past four
WIDTHS8 = (4, 6, 10, 66, 258, 266, 1026, 1030)
# three dwords; past a wave (64 dwords = 128 px); one strip and two dwords; two strips and two / six dwords
WIDTHS16 = (6, 130, 258, 514, 518)
# no rv at all (3, 4); one / two rows of rv; some rows; odd; past one segment of 64 rows; two zone rows of > 1 segment
HEIGHTS = (3, 4, 5, 6, 18, 37, 70, 133)


def same(got, want):
    assert got.shape == want.shape
    for f in ("h", "v", "nh", "nv"):
        assert np.array_equal(got[f], want[f]), (f, np.argwhere(got[f] != want[f])[:4].tolist())


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


def grids(W, H):
    return ((1, 1), (min(3, W // 2), min(5, H // 2)))


@pytest.mark.parametrize("W", WIDTHS8)
def test_8bit_geometries(gpu_pkg, W):
    rng = np.random.default_rng(W)
    for H in HEIGHTS:
        raw = frame8(rng, W, H)
        S = fm.samples(raw, W, H, raw.shape[1])
        with gpu_pkg.Context(W, H, "rggb", "RGBx", device=0) as ctx:
            for zx, zy in grids(W, H):
                for thr in (0, 64, 510):
                    got = ctx.focus_batch_via_device(raw[None], zx, zy, thr)[0]
                    same(got, fm.zone_focus(S, zx, zy, thr, 255))
            nh, nv = fm.counts_at_zero(W, H)
            got = ctx.focus_batch_via_device(raw[None], 1, 1, 0)[0]
            assert got["nh"][0, 0].tolist() == nh and got["nv"][0, 0].tolist() == nv


@pytest.mark.parametrize("bits", (10, 12, 16))
@pytest.mark.parametrize("big_endian", (False, True))
def test_deep_geometries(gpu_pkg, bits, big_endian):
    rng = np.random.default_rng(bits + big_endian)
    vmax = (1 << bits) - 1
    for W in WIDTHS16:
        for H in HEIGHTS if W in (6, 518) else (5, 37, 70):
            raw = frame16(rng, W, H, bits, big_endian)
            S = fm.samples(raw, W, H, raw.shape[1], bits, big_endian)
            with gpu_pkg.Context(W, H, "grbg", "ARGB64", device=0, bits=bits, src_big_endian=big_endian) as ctx:
                for zx, zy in grids(W, H):
                    for thr in (0, vmax // 4, 2 * vmax):
                        got = ctx.focus_batch_via_device(raw[None], zx, zy, thr)[0]
                        same(got, fm.zone_focus(S, zx, zy, thr, vmax))


def test_64x64_zones_with_empty_trailing_ones(gpu_pkg):
    W, H = 258, 130
    raw = frame8(np.random.default_rng(1), W, H)
    S = fm.samples(raw, W, H, raw.shape[1])
    with gpu_pkg.Context(W, H, device=0) as ctx:
        for thr in (0, 100):
            got = ctx.focus_batch_via_device(raw[None], 64, 64, thr)[0]
            same(got, fm.zone_focus(S, 64, 64, thr, 255))
    assert fm.cell(W, 64) == 6 and fm.cell(H, 64) == 4
    for f in ("h", "v", "nh", "nv"):
        assert not got[f][:, 43:].any() and not got[f][33:].any()


def test_padded_stride_and_offset_base(gpu_pkg):
    """0xFF in the row padding, which the last dword's neighbour load may touch but never count; the frame at 4 mod 16"""
    rng = np.random.default_rng(2)
    for W, H, stride in ((266, 18, 320), (258, 37, 264)):
        raw = frame8(rng, W, H, stride)
        want = fm.zone_focus(fm.samples(raw, W, H, stride), 3, 5, 32, 255)
        with gpu_pkg.Context(W, H, src_stride=stride, device=0) as ctx:
            same(ctx.focus_batch_via_device(raw[None], 3, 5, 32)[0], want)
            same(ctx.focus_batch_via_device(raw[None], 3, 5, 32, src_offset=4)[0], want)
    W, H, bits, stride = 130, 18, 12, 272
    raw = frame16(rng, W, H, bits, True, stride)
    want = fm.zone_focus(fm.samples(raw, W, H, stride, bits, True), 3, 5, 500, 4095)
    with gpu_pkg.Context(W, H, "gbrg", "ARGB64", src_stride=stride, device=0, bits=bits, src_big_endian=True) as ctx:
        same(ctx.focus_batch_via_device(raw[None], 3, 5, 500, src_offset=4)[0], want)


@pytest.mark.parametrize("deep", (False, True))
def test_batch_with_poisoned_gaps(gpu_pkg, deep):
    """three frames of different content, a frame pitch larger than the frame and gaps that would change the sums: no
    halo row comes from a neighbouring frame or from a gap.  The first and last rows of each frame are bright on dark,
    so a row borrowed across a frame seam would show."""
    W, H, n = 258, 37, 3
    rng = np.random.default_rng(4 + deep)
    if deep:
        raws = [frame16(rng, W, H, 12, False) for _ in range(n)]
        S = [fm.samples(r, W, H, r.shape[1], 12, False) for r in raws]
        vmax, kw = 4095, dict(pattern="bggr", fmt="ARGB64", bits=12)
    else:
        raws = [frame8(rng, W, H) for _ in range(n)]
        for f, r in enumerate(raws):
            r[:2, :W] = 255 - 100 * f
            r[-2:, :W] = 40 * f
        S = [fm.samples(r, W, H, r.shape[1]) for r in raws]
        vmax, kw = 255, dict(pattern="bggr", fmt="RGBx")
    pitch = raws[0].size + 3 * raws[0].shape[1] + 64
    padded = np.full((n, pitch), 0xEE, np.uint8)
    padded[:, :raws[0].size] = np.stack(raws).reshape(n, -1)
    for zx, zy, thr in ((1, 1, 0), (4, 3, vmax // 8)):
        want = np.stack([fm.zone_focus(s, zx, zy, thr, vmax) for s in S])
        with gpu_pkg.Context(W, H, device=0, **kw) as ctx:
            same(ctx.focus_batch_via_device(padded, zx, zy, thr, src_frame_bytes=pitch), want)
    # the second call zeroes again: the same zones, not doubled
    with gpu_pkg.Context(W, H, device=0, **kw) as ctx:
        d_src, d_focus = ctx.device_alloc(n * pitch), ctx.device_alloc(n * 12 * 96)
        try:
            ctx.to_device(d_src, padded)
            for _ in range(2):
                ctx.focus_device(d_src, d_focus, 4, 3, vmax // 8, n, pitch)
            ctx.sync()
            same(ctx.from_device(d_focus, n * 12 * 96).view(fm.FOCUS_DTYPE).reshape(n, 3, 4), want)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_focus)


@pytest.mark.parametrize("bits", (0, 10, 16))
def test_extreme_frame(gpu_pkg, bits):
    """0 / max alternating at same-site distance: |r| = 2 max wherever it is defined, the largest sums a segment holds"""
    W, H = 266, 133
    vmax = (1 << bits) - 1 if bits else 255
    y, x = np.mgrid[0:H, 0:W]
    S = (((x >> 1) + (y >> 1)) & 1) * vmax
    if bits:
        raw = S.astype("<u2").view(np.uint8).reshape(H, 2 * W)
        kw = dict(pattern="rggb", fmt="ARGB64", bits=bits)
    else:
        raw = np.zeros((H, (W + 3) & ~3), np.uint8)
        raw[:, :W] = S
        kw = dict(pattern="rggb", fmt="RGBx")
    nh, nv = fm.counts_at_zero(W, H)
    with gpu_pkg.Context(W, H, device=0, **kw) as ctx:
        for zx, zy in ((1, 1), (3, 2)):
            for thr in (0, 2 * vmax):
                got = ctx.focus_batch_via_device(np.ascontiguousarray(raw)[None], zx, zy, thr)[0]
                same(got, fm.zone_focus(S, zx, zy, thr, vmax))
                assert got["nh"].reshape(-1, 4).sum(0).tolist() == nh and got["nv"].reshape(-1, 4).sum(0).tolist() == nv
                assert np.array_equal(got["h"], got["nh"].astype(np.uint64) * np.uint64(2 * vmax))


def test_sums_need_64_bits(gpu_pkg):
    """520 x 520 of 0 / 65535 alternating in one zone: 66 564 responses of 131 070 per site and direction > 2^32"""
    W = H = 520
    y, x = np.mgrid[0:H, 0:W]
    S = (((x >> 1) + (y >> 1)) & 1) * 65535
    raw = np.ascontiguousarray(S.astype("<u2").view(np.uint8).reshape(H, 2 * W))
    with gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=16) as ctx:
        got = ctx.focus_batch_via_device(raw[None], 1, 1, 1)[0]
    n = 260 * 258
    assert got["nh"][0, 0].tolist() == [n] * 4 == got["nv"][0, 0].tolist()
    assert got["h"][0, 0].tolist() == [n * 131070] * 4 == got["v"][0, 0].tolist() and n * 131070 > 1 << 32


def test_every_bayer2rgb_context_is_accepted(gpu_pkg):
    W, H = 66, 18
    rng = np.random.default_rng(6)
    raw8 = frame8(rng, W, H)
    want8 = fm.zone_focus(fm.samples(raw8, W, H, raw8.shape[1]), 3, 2, 40, 255)
    raw12 = frame16(rng, W, H, 12, False)
    want12 = fm.zone_focus(fm.samples(raw12, W, H, 2 * W, 12), 3, 2, 400, 4095)
    col = gpu_pkg.Colour.make(black=4, gains=(2.0, 1.0, 1.5))
    for kw in (dict(fmt="RGBx", method="mhc"), dict(fmt="BGRx", colour=col), dict(fmt="RGB"), dict(fmt="BGR", method="mhc"),
               dict(fmt="GBR"), dict(fmt="ARGB64")):
        with gpu_pkg.Context(W, H, "gbrg", device=0, **kw) as ctx:
            same(ctx.focus_batch_via_device(raw8[None], 3, 2, 40)[0], want8)
    for kw in (dict(fmt="ARGB64", method="mhc", colour=col), dict(fmt="RGBx"), dict(fmt="RGB"), dict(fmt="GBR")):
        with gpu_pkg.Context(W, H, "gbrg", device=0, bits=12, **kw) as ctx:
            same(ctx.focus_batch_via_device(raw12[None], 3, 2, 400)[0], want12)


def test_argument_errors(gpu_pkg):
    L = gpu_pkg.lib()
    W, H = 66, 18

    def rc(ctx, d_src, d_focus, zx=1, zy=1, thr=0, n=1, pitch=None):
        return L.mibayer_focus_device(ctx._h, d_src, pitch or ctx.src_bytes, n, zx, zy, thr, d_focus, ctx.stream)

    with gpu_pkg.Context(W, H, device=0) as ctx, gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=10) as deep, \
            gpu_pkg.Context(W, H, "bggr", "ARGB", device=0, flags=gpu_pkg.FLAG_RGB2BAYER) as inv:
        d_src, d_focus = ctx.device_alloc(4 * W * H * 2), ctx.device_alloc(64 * 64 * 96)
        try:
            E = gpu_pkg.ERR_ARG
            assert rc(ctx, d_src, d_focus) == gpu_pkg.OK
            assert rc(inv, d_src, d_focus) == E
            assert rc(ctx, d_src, d_focus, thr=510) == gpu_pkg.OK and rc(ctx, d_src, d_focus, thr=511) == E
            assert rc(deep, d_src, d_focus, thr=2046) == gpu_pkg.OK and rc(deep, d_src, d_focus, thr=2047) == E
            assert rc(ctx, d_src, d_focus, thr=0xFFFFFFFF) == E
            for zx, zy in ((0, 1), (1, 0), (0, 0), (65, 1), (1, 65), (34, 1), (1, 10), (-1, 1)):
                assert rc(ctx, d_src, d_focus, zx, zy) == E, (zx, zy)
            assert rc(ctx, d_src, d_focus, 33, 9) == gpu_pkg.OK
            assert rc(ctx, d_src + 2, d_focus) == E and rc(ctx, d_src, d_focus + 4) == E
            assert rc(ctx, None, d_focus) == E and rc(ctx, d_src, None) == E and rc(ctx, d_src, d_focus, n=-1) == E
            assert rc(ctx, d_src, d_focus, n=0) == gpu_pkg.OK
            assert rc(ctx, d_src, d_focus, n=2, pitch=ctx.src_bytes - 4) == gpu_pkg.ERR_GEOMETRY
            assert rc(ctx, d_src, d_focus, n=2, pitch=ctx.src_bytes + 2) == gpu_pkg.ERR_GEOMETRY
            ctx.sync(), deep.sync()
            # the host-path setters check the same things
            assert L.mibayer_set_focus(inv._h, 1, 1, 0) == E and L.mibayer_set_focus(inv._h, 0, 0, 0) == E
            assert L.mibayer_set_focus(ctx._h, 34, 1, 0) == E and L.mibayer_set_focus(ctx._h, 1, 1, 511) == E
            assert L.mibayer_set_focus(ctx._h, 0, 1, 0) == E
            out = np.zeros(1, fm.FOCUS_DTYPE)
            assert L.mibayer_frame_focus(ctx._h, out.ctypes.data, 1) == gpu_pkg.ERR_EMPTY
            assert L.mibayer_frame_focus(ctx._h, None, 1) == E
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_focus)


@pytest.mark.parametrize("case", fc.CASES, ids=lambda c: "%dx%d_%d%s_%dx%d" % (c.W, c.H, c.bits, "be" if c.big_endian else "",
                                                                               c.zones_x, c.zones_y))
def test_case_table(gpu_pkg, case):
    """the table of tests/focus_cases.py (what it reaches: tests/test_focus_cases.py), at its threshold, one below and
    one above it, and at 0"""
    raw = fc.frame(case)
    thr = fc.threshold(case)
    kw = dict(pattern="grbg", fmt="ARGB64", bits=case.bits, src_big_endian=case.big_endian) if case.bits else {}
    with gpu_pkg.Context(case.W, case.H, device=0, **kw) as ctx:
        for t in (thr, thr - 1, thr + 1, 0):
            same(ctx.focus_batch_via_device(raw[None], case.zones_x, case.zones_y, t)[0], fc.expected(case, raw, t))
