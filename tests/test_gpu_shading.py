"""GPU tests of the lens shading correction (include/mibayer.h, group `shading`): mosaic_shade_kernel through
mibayer_shade_device and through the host path, bit-exact against tests/shading_model.py.

The kernel (csrc/mibayer_kernels.hip): a lane owns one dword of a row -- 4 samples of an 8-bit mosaic, 2 of a deep one; a
wave spans 64 dwords, a workgroup 256 = one strip; a row whose width is 2 mod 4 ends in a half dword that is stored as 16
bits.  A workgroup walks kShadeMinRows = 16 rows of a small launch and up to kShadeMaxRows = 64 of a large one
(tests/shading_cases.py restates the rule; section E runs the long ones), cell row by cell row, kShadeAhead = 8 rows at a
time, and reads a new row of nodes at every cell-row seam.  Widths: one lane (4), a tail only behind it (6), past a wave (258),
past a strip with a tail (1030; 518 for 16-bit samples).  Heights: the smallest, an odd one, one past two segments (37),
and one that ends exactly on a cell-row seam."""
import numpy as np
import pytest

import band_cases as bc
import shading_cases as shc
import shading_model as shm
import stats_model as sm
import strip_cases as sc
import test_gpu_band_seams as bs
import tile_cases as tc

pytestmark = pytest.mark.gpu

GRIDS = [(2, 2), (8, 8), (2, 8), (5, 3)]
WIDTHS8 = (4, 6, 258, 1030)
WIDEST_K2 = 510                 # cells of 4 pixels: the widest frame of 2 mod 4 that 129 nodes cover (1030 asks for 259)
DEEP_GRIDS = [(8, 8), (5, 3), (3, 8), (4, 2)]   # ... and 518 asks for 131
SRC_FILL, DST_FILL, GUARD = 0x5A, 0xC3, 64


def seam_height(ky):
    """a height that ends exactly on a cell-row seam, at least 40 rows or one cell"""
    ch = 1 << ky
    return max(ch, 40 // ch * ch)


site_planes = shc.site_planes


def run_device(ctx, frames, pitch=None, offset=0, in_place=False):
    """frames: (n, src_bytes) bytes -> (n, src_bytes) bytes after ONE mibayer_shade_device launch, and the bytes the
    destination held before.  Source and destination are surrounded by guards and sit `offset` bytes into their
    allocations, `pitch` bytes apart; everything outside the frames must stay as it was, and so must the source of an
    out-of-place launch"""
    frames = np.ascontiguousarray(frames, np.uint8)
    n, nb = frames.shape
    assert nb == ctx.src_bytes
    pitch = pitch or nb
    total = offset + n * pitch + GUARD
    src = np.full(total, SRC_FILL, np.uint8)
    for f in range(n):
        src[offset + f * pitch:offset + f * pitch + nb] = frames[f]
    # an out-of-place destination holds a sentinel everywhere: the row padding must keep it
    before = src.copy() if in_place else np.full(total, DST_FILL, np.uint8)
    d_src = ctx.device_alloc(total)
    d_dst = d_src if in_place else ctx.device_alloc(total)
    try:
        ctx.to_device(d_src, src)
        if not in_place:
            ctx.to_device(d_dst, before)
        ctx.shade_device(d_src + offset, None if in_place else d_dst + offset, n, pitch, pitch)
        ctx.sync()
        out = ctx.from_device(d_dst, total)
        if not in_place:
            assert np.array_equal(ctx.from_device(d_src, total), src), "the source of an out-of-place launch changed"
    finally:
        ctx.device_free(d_src)
        if not in_place:
            ctx.device_free(d_dst)
    keep = np.ones(total, bool)
    for f in range(n):
        keep[offset + f * pitch:offset + f * pitch + nb] = False
    assert np.array_equal(out[keep], before[keep]), "bytes outside the frames were written"
    pick = lambda a: np.stack([a[offset + f * pitch:offset + f * pitch + nb] for f in range(n)])  # noqa: E731
    return pick(out), pick(before)


def check(pkg, ctx, frames, table, kx, ky, black, bits=0, sbe=False, where="", segment_of=None, **kw):
    """one launch in place and one out of place, each against the model.  `segment_of`: row -> (ya, yb) of the
    workgroups that walk it, for the message"""
    w, h, stride = ctx.width, ctx.height, ctx.src_stride
    ctx.set_shading(pkg.Shading(kx, ky, table, black))
    for in_place in (False, True):
        got, before = run_device(ctx, frames, in_place=in_place, **kw)
        for f in range(len(frames)):
            want = shm.shade_raw(frames[f], table, kx, ky, black, w, h, stride, bits, sbe, dst=before[f])
            if not np.array_equal(got[f], want):
                bad = np.argwhere(got[f].reshape(h, stride) != want.reshape(h, stride))
                seg = " in the segment of rows %d .. %d" % segment_of(bad[0][0]) if segment_of else ""
                raise AssertionError("%s %dx%d k=(%d,%d) %s frame %d: %d bytes differ, first at row %d byte %d%s (got %d, want %d)"
                                     % (where, w, h, kx, ky, "in place" if in_place else "out of place", f, len(bad), bad[0][0],
                                        bad[0][1], seg, got[f].reshape(h, stride)[tuple(bad[0])],
                                        want.reshape(h, stride)[tuple(bad[0])]))


# -- A. widths, heights, grids ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kx,ky", GRIDS)
def test_every_width_and_height_8bit(gpu_pkg, kx, ky):
    """rows carry 4 bytes of padding: the half dword of a width of 2 mod 4 and the padding behind it keep the
    destination's sentinel"""
    rng = np.random.default_rng([1, kx, ky])
    for w in WIDTHS8 if kx > 2 else WIDTHS8[:3] + (WIDEST_K2,):
        for h in (3, 5, 37, seam_height(ky)):
            stride = ((w + 3) & ~3) + 4
            with gpu_pkg.Context(w, h, sc.ORDERS[(w + h) % 4], "RGBx", src_stride=stride, device=0) as ctx:
                frame = sc.random_frame(rng, w, h, 0, stride).reshape(1, -1)
                check(gpu_pkg, ctx, frame, site_planes(w, h, kx, ky), kx, ky, (16, 9, 12, 20), where="8-bit")


@pytest.mark.parametrize("sbe", [False, True], ids=["le", "be"])
@pytest.mark.parametrize("bits", [10, 12, 14, 16])
def test_deep_mosaics_both_byte_orders(gpu_pkg, bits, sbe):
    """16-bit words with junk above `bits`: the output has those bits zero, in the source's byte order"""
    rng = np.random.default_rng([2, bits, sbe])
    vmax = (1 << bits) - 1
    for i, (w, h) in enumerate([(518, 37), (6, 5), (4, 3), (518, 40)]):
        kx, ky = (DEEP_GRIDS if w > 500 else GRIDS)[(i + bits // 2) % 4]
        with gpu_pkg.Context(w, h, sc.ORDERS[i], "RGBx", bits=bits, src_big_endian=sbe, device=0) as ctx:
            frame = sc.random_frame(rng, w, h, bits, None, sbe).reshape(1, -1)
            check(gpu_pkg, ctx, frame, site_planes(w, h, kx, ky, rng), kx, ky, (vmax // 16, vmax // 20, vmax // 18, vmax // 14),
                  bits, sbe, where="%d-bit %s" % (bits, "BE" if sbe else "LE"))


# -- B. addressing -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_random_table_padded_stride_odd_base_and_frame_pitch(gpu_pkg, bits):
    """a random table; rows with 12 bytes of padding; the base pointer at 4 mod 16; 3 frames 20 bytes further apart than
    a frame is long"""
    rng = np.random.default_rng([3, bits])
    w, h, kx, ky = (1030, 37, 5, 3) if bits == 0 else (518, 21, 3, 2)
    stride = sc.src_row_bytes(w, bits) + 12
    nx, ny = shm.nodes(w, h, kx, ky)
    table = rng.integers(0, shm.MAX_ENTRY + 1, (4, ny, nx)).astype(np.uint16)
    vmax = (1 << (bits or 8)) - 1
    with gpu_pkg.Context(w, h, "grbg", "RGBx", src_stride=stride, bits=bits, device=0) as ctx:
        frames = np.stack([sc.random_frame(rng, w, h, bits, stride).reshape(-1) for _ in range(3)])
        check(gpu_pkg, ctx, frames, table, kx, ky, tuple(rng.integers(0, vmax + 1, 4)), bits, where="random table",
              pitch=ctx.src_bytes + 20, offset=4)


def test_errors_follow_the_header(gpu_pkg):
    pkg = gpu_pkg
    L = pkg.lib()
    with pkg.Context(64, 48, device=0) as ctx:
        d = ctx.device_alloc(4 * ctx.src_bytes)
        try:
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d, ctx.src_bytes, 1, None) == pkg.ERR_EMPTY
            assert ctx.get_shading() is None
            nx, ny = pkg.shading_nodes(64, 48, 4, 4)
            table = np.full((4, ny, nx), 5000, np.uint16)
            ctx.set_shading(pkg.Shading(4, 4, table, (1, 2, 3, 4)))
            kx, ky, black, got = ctx.get_shading()
            assert (kx, ky, black) == (4, 4, (1, 2, 3, 4)) and np.array_equal(got, table)
            s = ctx.stream
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d, ctx.src_bytes, 0, s) == pkg.OK
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d, ctx.src_bytes, -1, s) == pkg.ERR_ARG
            assert L.mibayer_shade_device(ctx._h, None, ctx.src_bytes, d, ctx.src_bytes, 1, s) == pkg.ERR_ARG
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, None, ctx.src_bytes, 1, s) == pkg.ERR_ARG
            assert L.mibayer_shade_device(ctx._h, d + 2, ctx.src_bytes, d, ctx.src_bytes, 1, s) == pkg.ERR_ARG
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d + 1, ctx.src_bytes, 1, s) == pkg.ERR_ARG
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes - 4, d, ctx.src_bytes, 2, s) == pkg.ERR_GEOMETRY
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d, ctx.src_bytes + 2, 2, s) == pkg.ERR_GEOMETRY
            # in place with two pitches: a frame's stores would land in another frame's unread samples
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d, ctx.src_bytes + 4, 2, s) == pkg.ERR_GEOMETRY
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes + 4, d, ctx.src_bytes + 4, 2, s) == pkg.OK
            assert L.mibayer_shade_device(ctx._h, d, ctx.src_bytes, d, ctx.src_bytes + 4, 1, s) == pkg.OK
            # the rules of mibayer_set_shading
            bad = table.copy()
            bad[3, ny - 1, nx - 1] = 32768
            for sh in (pkg.Shading(4, 4, bad), pkg.Shading(4, 4, table, (0, 0, 256, 0)), pkg.Shading(1, 4, table),
                       pkg.Shading(4, 9, table), pkg.Shading(4, 4, None)):
                assert L.mibayer_set_shading(ctx._h, sh) == pkg.ERR_ARG
            short = pkg.Shading(4, 4, table)
            short.struct_size -= 4
            assert L.mibayer_set_shading(ctx._h, short) == pkg.ERR_ARG
            assert ctx.get_shading()[2] == (1, 2, 3, 4)         # a refused table leaves the one set before
            ctx.set_shading(None)
            assert ctx.get_shading() is None
            ctx.sync()
        finally:
            ctx.device_free(d)
    with pkg.Context(64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER, device=0) as inv:
        assert L.mibayer_set_shading(inv._h, pkg.Shading(4, 4, table)) == pkg.ERR_ARG
        assert L.mibayer_set_shading(inv._h, None) == pkg.ERR_ARG
    # a frame of more than 129 nodes under the smallest cells
    with pkg.Context(516, 8, device=0) as wide:
        nx, ny = 130, 3
        assert L.mibayer_set_shading(wide._h, pkg.Shading(2, 2, np.full((4, ny, nx), 4096, np.uint16))) == pkg.ERR_ARG
        nx, ny = pkg.shading_nodes(516, 8, 3, 2)
        wide.set_shading(pkg.Shading(3, 2, np.full((4, ny, nx), 4096, np.uint16)))


# -- C. extremes ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 16])
def test_extreme_values(gpu_pkg, bits):
    """gain 0 and 32767, S = 0 and max, black = 0 and max, the largest cells: G fills uint32 and d G + 2048 fills int32"""
    rng = np.random.default_rng([4, bits])
    w, h, kx, ky = 262, 259, 8, 8
    vmax = (1 << (bits or 8)) - 1
    nx, ny = shm.nodes(w, h, kx, ky)
    with gpu_pkg.Context(w, h, "rggb", "RGBx", bits=bits, device=0) as ctx:
        S = rng.choice([0, vmax], (h, w))
        frame = sc.frame_bytes(S, bits, rng).reshape(1, -1)
        for gain in (0, 32767):
            for black in (0, vmax):
                check(gpu_pkg, ctx, frame, np.full((4, ny, nx), gain, np.uint16), kx, ky, (black,) * 4, bits,
                      where="gain %d black %d" % (gain, black))
        # every node at an extreme of its own, every site its own black level
        table = rng.choice([0, 32767], (4, ny, nx)).astype(np.uint16)
        check(gpu_pkg, ctx, frame, table, kx, ky, (0, vmax, vmax, 0), bits, where="mixed extremes")


def test_unity_table_is_the_identity(gpu_pkg):
    rng = np.random.default_rng(5)
    w, h, kx, ky = 258, 37, 5, 3
    nx, ny = shm.nodes(w, h, kx, ky)
    with gpu_pkg.Context(w, h, "bggr", "RGBx", bits=10, device=0) as ctx:
        frame = sc.random_frame(rng, w, h, 10).reshape(1, -1)
        ctx.set_shading(gpu_pkg.Shading(kx, ky, np.full((4, ny, nx), 4096, np.uint16), (0, 1023, 77, 500)))
        got, _ = run_device(ctx, frame, in_place=True)
        S = sm.samples(frame[0], w, h, ctx.src_stride, 10)
        assert np.array_equal(sm.samples(got[0], w, h, ctx.src_stride, 16), S)      # the junk above 10 bits is gone


# -- D. host path ----------------------------------------------------------------------------------------------------------------

DEEP_12_TO_16 = bc.Family("deep_12_to_16", "strip", sc.STRIP_ROWS, sc.Arm("deep_12_to_16", "bilinear", 12, True, False), 1, False)
HOST_FAMILIES = {"tile_8_bilinear": lambda: bc.family(tc.NT_NAMES[0]), "deep_12_to_argb64": lambda: DEEP_12_TO_16,
                 "mhc_8_to_8": lambda: bc.family("mhc_8_to_8")}
HOST_SIZE = (266, 52)           # strip families: bands of 16, 16, 16 and 4 rows; cells of 8 rows cut every band


def host_case(fam, w, h):
    if fam is DEEP_12_TO_16:
        return sc.Case(w, h, "grbg", "ARGB64", True, False)
    return bc.rotate(fam, 2, w, h)


@pytest.mark.parametrize("name", sorted(HOST_FAMILIES))
def test_host_path_shades_every_row_once(gpu_pkg, gpu_lab_pkg, oracle, name):
    """a frame banded by its destination stride (tests/test_gpu_band_seams.py) and the same frame with two in flight
    (never banded): the bytes are the demosaic model's on the model-shaded mosaic, mibayer_frame_stats counts shaded
    samples, and with the table taken away again the bytes are those from before"""
    pkg = gpu_pkg
    fam = HOST_FAMILIES[name]()
    w, h = HOST_SIZE
    case = host_case(fam, w, h)
    bits = 0 if fam.kind == "tile" else fam.arm.bits
    sbe = fam.kind == "strip" and case.sbe
    depth = bits or 8
    kx, ky = 5, 3
    rng = np.random.default_rng([6, sorted(HOST_FAMILIES).index(name)])
    sstride, _ = bc.strides(fam, w, h)
    buf = bs.random_frame(fam, case, rng, sstride)
    table = site_planes(w, h, kx, ky, rng)
    black = (1 << depth) // 16
    blacks = (black, black + 3, black + 1, black + 2)
    shaded = shm.shade_raw(buf, table, kx, ky, blacks, w, h, sstride, bits, sbe).reshape(h, sstride)
    want_plain = bs.expect(pkg, oracle, fam, buf, case)
    want = bs.expect(pkg, oracle, fam, shaded, case)
    assert not np.array_equal(want, want_plain)
    S_shaded = sm.samples(shaded, w, h, sstride, bits, sbe)
    zx, zy = bc.stats_grid(h)
    lo, hi = 0, (1 << depth) - 1
    # the frame really is banded: the model's count (4 for the strip families, 2 for the 1024 x 32 tiles), and the
    # library's own count where it says it (the lab build, the same sources)
    nb = bc.expected_bands(fam, case)
    assert nb == (4 if fam.kind == "strip" else bc.host_bands(bc.PRODUCT_WANT, bc.BAND_MIN_BYTES, h, fam.unit)) and nb >= 2
    with bs.open_banded(gpu_lab_pkg, fam, case) as lab:
        assert lab.host_bands == nb, (name, lab.host_bands, nb)
    with bs.open_banded(pkg, fam, case) as ctx:
        before = bs.convert_alone(ctx, buf).copy()
        assert not bs.problems(before, want_plain)
        ctx.set_shading(pkg.Shading(kx, ky, table, blacks))
        ctx.set_stats(zx, zy, lo, hi)
        for again in range(2):
            got = bs.convert_alone(ctx, buf)
            bad = bs.problems(got, want)
            assert not bad, "%s banded, frame %d: %s" % (name, again, "\n".join(bad))
            zones, want_zones = ctx.frame_stats(), sm.zone_stats(S_shaded, zx, zy, lo, hi)
            for field in ("sum", "count", "clipped"):
                assert np.array_equal(zones[field], want_zones[field]), (name, field)
        ctx.set_stats(0, 0)
        ctx.set_shading(None)
        assert np.array_equal(bs.convert_alone(ctx, buf), before), "the bytes without a table are not those from before"
    with bs.open_banded(pkg, fam, case, inflight=2) as ctx:
        ctx.set_shading(pkg.Shading(kx, ky, table, blacks))
        outs = [bs.host_frame(ctx) for _ in range(2)]
        src = np.ascontiguousarray(buf).reshape(-1)
        for i, o in enumerate(outs):
            ctx.submit(src, o, tag=i + 1)
        assert [ctx.wait(), ctx.wait()] == [1, 2]
        for o in outs:
            bad = bs.problems(o, want)
            assert not bad, "%s two in flight: %s" % (name, "\n".join(bad))


def test_hipgraph_context_shades_without_graphs(gpu_pkg, oracle):
    pkg = gpu_pkg
    w, h, kx, ky = 258, 37, 4, 4
    rng = np.random.default_rng(8)
    buf = sc.random_frame(rng, w, h, 0)
    table = site_planes(w, h, kx, ky)
    shaded = shm.shade_raw(buf, table, kx, ky, (4, 4, 4, 4), w, h, buf.shape[1]).reshape(buf.shape)
    r, g, b = pkg.FORMATS["BGRx"]
    with pkg.Context(w, h, "gbrg", "BGRx", flags=pkg.FLAG_HIPGRAPH, inflight=2, device=0) as ctx:
        plain = ctx.process_host(buf).copy()
        assert np.array_equal(plain, oracle.bayer2rgb(buf, w, "gbrg", r, g, b))
        ctx.set_shading(pkg.Shading(kx, ky, table, (4, 4, 4, 4)))
        assert np.array_equal(ctx.process_host(buf), oracle.bayer2rgb(shaded, w, "gbrg", r, g, b))
        ctx.set_shading(None)
        assert np.array_equal(ctx.process_host(buf), plain)


@pytest.mark.parametrize("bits", [0, 12])
def test_two_shard_pool_gives_the_same_bytes(gpu_pkg, oracle, bits):
    """two shards on one device, six frames under three tables in turn (the last: none): every frame comes back shaded
    with the table the pool held when it was submitted, whichever shard converted it"""
    pkg = gpu_pkg
    w, h, kx, ky = 258, 37, 5, 3
    rng = np.random.default_rng([7, bits])
    fmt = "ARGB64" if bits else "RGBx"
    deep = dict(bits=bits, out16=True) if bits else {}
    tables = [site_planes(w, h, kx, ky), site_planes(w, h, kx, ky, rng)[::-1].copy(), None]
    blacks = (3, 5, 7, 9)
    bufs = [sc.random_frame(rng, w, h, bits) for _ in range(6)]

    def model(buf, table):
        src = buf if table is None else shm.shade_raw(buf, table, kx, ky, blacks, w, h, buf.shape[1], bits).reshape(buf.shape)
        if bits:
            return sc.expect(DEEP_12_TO_16.arm, src, sc.Case(w, h, "rggb", fmt, False, False))
        r, g, b = pkg.FORMATS[fmt]
        return oracle.bayer2rgb(src, w, "rggb", r, g, b)

    with pkg.Pool([0, 0], w, h, "rggb", fmt, inflight=2, **deep) as pool:
        outs = []
        for i, buf in enumerate(bufs):
            if i % 2 == 0:
                t = tables[i // 2]
                pool.set_shading(None if t is None else pkg.Shading(kx, ky, t, blacks))
            if pool.pending() == pool.capacity:
                pool.wait()
            outs.append(np.full(model(bufs[0], None).shape, 0xA5, np.uint8))
            pool.submit(np.ascontiguousarray(buf).reshape(-1), outs[-1], tag=i + 1)
        while pool.pending():
            pool.wait()
    for i, (buf, out) in enumerate(zip(bufs, outs)):
        assert np.array_equal(out, model(buf, tables[i // 2])), "frame %d" % i


def test_pool_refuses_what_a_context_refuses(gpu_pkg):
    """mibayer_pool_set_shading restates the context's rules on the pool's resolved configuration"""
    pkg = gpu_pkg
    L = pkg.lib()
    w, h = 64, 48
    nx, ny = pkg.shading_nodes(w, h, 4, 4)
    table = np.full((4, ny, nx), 5000, np.uint16)
    bad = table.copy()
    bad[3, ny - 1, nx - 1] = 32768
    short = pkg.Shading(4, 4, table)
    short.struct_size -= 4
    with pkg.Pool([0, 0], w, h, "rggb", "RGBx", inflight=2) as pool:
        for sh in (pkg.Shading(4, 4, bad), pkg.Shading(4, 4, table, (0, 256, 0, 0)), pkg.Shading(1, 4, table),
                   pkg.Shading(4, 9, table), pkg.Shading(4, 4, None), short):
            assert L.mibayer_pool_set_shading(pool._h, sh) == pkg.ERR_ARG
        pool.set_shading(pkg.Shading(4, 4, table, (0, 255, 0, 0)))
        pool.set_shading(None)
    with pkg.Pool([0, 0], w, h, "rggb", "ARGB64", inflight=2, bits=10, out16=True) as deep:
        assert L.mibayer_pool_set_shading(deep._h, pkg.Shading(4, 4, table, (0, 1024, 0, 0))) == pkg.ERR_ARG
        deep.set_shading(pkg.Shading(4, 4, table, (0, 1023, 0, 0)))
    with pkg.Pool([0], 516, 8, "rggb", "RGBx") as wide:        # 130 nodes under cells of 4
        assert L.mibayer_pool_set_shading(wide._h, pkg.Shading(2, 2, np.full((4, 3, 130), 4096, np.uint16))) == pkg.ERR_ARG
    with pkg.Pool([0, 0], w, h, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER) as inv:
        assert L.mibayer_pool_set_shading(inv._h, pkg.Shading(4, 4, table)) == pkg.ERR_ARG
        assert L.mibayer_pool_set_shading(inv._h, None) == pkg.OK       # off is what it is already


# -- E. segments longer than the minimum ---------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", shc.LONG_CASES, ids=shc.case_id)
def test_segments_longer_than_the_minimum(gpu_pkg, case):
    """long batches of narrow frames, whose workgroups walk 18 .. 64 rows and start inside a cell row
    (tests/test_shading_cases.py: which rows and phases, and that these tables show a wrong weight or stale nodes): ONE
    launch for the whole batch, in place and out of place, every frame random and every frame compared; four black
    levels; frames 20 bytes further apart than they are long, the base pointer at 4 mod 16"""
    rng = np.random.default_rng([9, case.w, case.h, case.ky])
    vmax = (1 << (case.bits or 8)) - 1
    stride = sc.src_row_bytes(case.w, case.bits) + 4
    with gpu_pkg.Context(case.w, case.h, sc.ORDERS[(case.w + case.h) % 4], "RGBx", src_stride=stride, bits=case.bits,
                         src_big_endian=case.sbe, device=0) as ctx:
        table = site_planes(case.w, case.h, case.kx, case.ky, rng)
        frames = np.stack([sc.random_frame(rng, case.w, case.h, case.bits, stride, case.sbe).reshape(-1)
                           for _ in range(case.nframes)])
        check(gpu_pkg, ctx, frames, table, case.kx, case.ky, (vmax // 16, vmax // 20, vmax // 18, vmax // 14), case.bits,
              case.sbe, where=shc.case_id(case), segment_of=lambda row: shc.segment_of(case, row),
              pitch=ctx.src_bytes + 20, offset=4)
