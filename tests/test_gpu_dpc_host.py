"""GPU tests of the defective pixel correction on the host path (csrc/mibayer_abi.hip: a second mosaic per ring slot,
the pass in front of the shading pass, rows two behind the upload in a banded frame): the bytes are the demosaic model's
on the model-corrected (and then model-shaded) mosaic, byte for byte.  The device path is tests/test_gpu_dpc.py."""
import numpy as np
import pytest

import band_cases as bc
import dpc_model as dm
import hist_model as hm
import shading_model as shm
import stats_model as sm
import strip_cases as sc
import test_gpu_band_seams as bs
from test_gpu_shading import DEEP_12_TO_16, HOST_FAMILIES, HOST_SIZE, host_case, site_planes

pytestmark = pytest.mark.gpu

KX, KY = 5, 3
LAB_SIZE = (266, 116)           # 15 units of 8 rows, 8 of 16: every band count from 1 to 8 cuts it (last band: 4 rows)


def fam_format(fam, case):
    bits = 0 if fam.kind == "tile" else fam.arm.bits
    return bits, fam.kind == "strip" and case.sbe


def thresholds(bits):
    vmax = (1 << (bits or 8)) - 1
    return vmax // 6, vmax // 7


def cut_defects(w, h, cuts, rng):
    """listed defects two rows on either side of every row in `cuts`, on the first and last two rows, and a few anywhere:
    unsorted, with duplicates"""
    rows = sorted({y for c in list(cuts) + [0, h] for y in (c - 2, c - 1, c, c + 1) if 0 <= y < h})
    xs = [0, 1, 2, 3, w // 2, w // 2 + 1, w - 4, w - 3, w - 2, w - 1]
    lst = [(x, y) for y in rows for x in xs] + [(int(rng.integers(0, w)), int(rng.integers(0, h))) for _ in range(40)]
    lst = np.array(lst + lst[:7], np.uint32)
    return lst[rng.permutation(len(lst))]


def model_mosaic(buf, w, h, sstride, bits, sbe, dpc=None, shade=None):
    """the mosaic everything behind the passes reads: corrected, then shaded"""
    out = np.ascontiguousarray(buf).reshape(-1)
    if dpc is not None:
        hot, cold, lst = dpc
        out = dm.correct_raw(out, out, w, h, sstride, bits, sbe, hot, cold, lst)
    if shade is not None:
        table, blacks = shade
        out = shm.shade_raw(out, table, KX, KY, blacks, w, h, sstride, bits, sbe)
    return out.reshape(h, sstride)


def shading_of(w, h, bits, rng):
    black = (1 << (bits or 8)) // 16
    return site_planes(w, h, KX, KY, rng), (black, black + 3, black + 1, black + 2)


# -- A. product build: banded by the frame's bytes, and two frames in flight -----------------------------------------------

@pytest.mark.parametrize("with_shading", [False, True], ids=["dpc", "dpc_then_shading"])
@pytest.mark.parametrize("name", sorted(HOST_FAMILIES))
def test_host_path_corrects_every_row_once(gpu_pkg, gpu_lab_pkg, oracle, name, with_shading):
    """process_host (banded: the frame has the link to itself) and submit / wait with two in flight (never banded): the
    same bytes, those of the models; mibayer_frame_stats and mibayer_frame_hist see corrected samples; with the correction
    taken away again the bytes are those from before, and the default equals an explicit `off`"""
    pkg = gpu_pkg
    fam = HOST_FAMILIES[name]()
    w, h = HOST_SIZE
    case = host_case(fam, w, h)
    bits, sbe = fam_format(fam, case)
    depth = bits or 8
    rng = np.random.default_rng([11, sorted(HOST_FAMILIES).index(name), with_shading])
    sstride, _ = bc.strides(fam, w, h)
    buf = bs.random_frame(fam, case, rng, sstride)
    nb = bc.expected_bands(fam, case)
    assert nb >= 2
    hot, cold = thresholds(bits)
    lst = cut_defects(w, h, [y0 for y0, _ in bc.band_rows(nb, h, fam.unit)[1:]], rng)
    shade = shading_of(w, h, bits, rng) if with_shading else None
    mosaic = model_mosaic(buf, w, h, sstride, bits, sbe, (hot, cold, lst), shade)
    want_plain = bs.expect(pkg, oracle, fam, buf, case)
    want = bs.expect(pkg, oracle, fam, mosaic, case)
    assert not np.array_equal(want, want_plain)
    S = sm.samples(mosaic, w, h, sstride, bits, sbe)
    assert 0.01 < dm.flagged(sm.samples(buf, w, h, sstride, bits, sbe), hot, cold).mean() < 0.99
    zx, zy = bc.stats_grid(h)
    lo, hi = 0, (1 << depth) - 1
    win = (2, 3, w - 6, h - 7)
    with bs.open_banded(gpu_lab_pkg, fam, case) as lab:
        assert lab.host_bands == nb, (name, lab.host_bands, nb)
    with bs.open_banded(pkg, fam, case) as ctx:
        before = bs.convert_alone(ctx, buf).copy()
        assert not bs.problems(before, want_plain)
        ctx.set_dpc(pkg.Dpc(-1, -1, None))              # on, and the identity: every sample is copied
        assert np.array_equal(bs.convert_alone(ctx, buf), before)
        ctx.set_dpc(pkg.Dpc(hot, cold, lst))
        if shade:
            ctx.set_shading(pkg.Shading(KX, KY, *shade))
        ctx.set_stats(zx, zy, lo, hi)
        ctx.set_hist(True, win)
        for again in range(2):
            got = bs.convert_alone(ctx, buf)
            bad = bs.problems(got, want)
            assert not bad, "%s banded, frame %d: %s" % (name, again, "\n".join(bad))
            zones, want_zones = ctx.frame_stats(), sm.zone_stats(S, zx, zy, lo, hi)
            for field in ("sum", "count", "clipped"):
                assert np.array_equal(zones[field], want_zones[field]), (name, field)
            assert np.array_equal(ctx.frame_hist(), hm.histogram(S, depth, win)), name
        ctx.set_stats(0, 0)
        ctx.set_hist(False)
        ctx.set_shading(None)
        ctx.set_dpc(None)
        assert ctx.get_dpc() is None
        assert np.array_equal(bs.convert_alone(ctx, buf), before), "the bytes with the correction off are not those from before"
    with bs.open_banded(pkg, fam, case, inflight=2) as ctx:
        ctx.set_dpc(pkg.Dpc(hot, cold, lst))
        if shade:
            ctx.set_shading(pkg.Shading(KX, KY, *shade))
        outs = [bs.host_frame(ctx) for _ in range(2)]
        src = np.ascontiguousarray(buf).reshape(-1)
        for i, o in enumerate(outs):
            ctx.submit(src, o, tag=i + 1)
        assert [ctx.wait(), ctx.wait()] == [1, 2]
        for o in outs:
            bad = bs.problems(o, want)
            assert not bad, "%s two in flight: %s" % (name, "\n".join(bad))


# -- B. lab build: every band count ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("want", range(1, 9), ids=lambda n: "want%d" % n)
@pytest.mark.parametrize("name", sorted(HOST_FAMILIES))
def test_every_band_count_with_defects_on_every_cut(gpu_lab_pkg, oracle, monkeypatch, name, want):
    """MIBAYER_HOST_BANDS = 1 .. 8 on a frame of 116 rows: listed defects two rows on either side of every band cut, random
    samples everywhere (a sixth of them flagged).  A row is corrected when the rows two below it are on the device: the
    bilinear families (halo 1) correct row ranges with odd ends, MHC (halo 2) even ones"""
    pkg = gpu_lab_pkg
    fam = HOST_FAMILIES[name]()
    w, h = LAB_SIZE
    case = host_case(fam, w, h)
    bits, sbe = fam_format(fam, case)
    bs.set_wanted(monkeypatch, want)
    rng = np.random.default_rng([12, sorted(HOST_FAMILIES).index(name), want])
    sstride, _ = bc.strides(fam, w, h)
    buf = bs.random_frame(fam, case, rng, sstride)
    nb = bc.expected_bands(fam, case, want)
    assert nb <= want and (nb == want or want not in (1, 2, 4, 8)), (name, want, nb)
    rows = bc.band_rows(nb, h, fam.unit)
    cuts = [y0 for y0, _ in rows[1:]]
    # ... and the rows at which the correction's own ranges end: the band's end + halo
    lst = cut_defects(w, h, cuts + [y1 + fam.halo for _, y1 in rows[:-1]], rng)
    hot, cold = thresholds(bits)
    shade = shading_of(w, h, bits, rng) if want % 2 else None
    mosaic = model_mosaic(buf, w, h, sstride, bits, sbe, (hot, cold, lst), shade)
    expect = bs.expect(pkg, oracle, fam, mosaic, case)
    with bs.open_banded(pkg, fam, case) as ctx:
        assert ctx.host_bands == nb
        ctx.set_dpc(pkg.Dpc(hot, cold, lst))
        if shade:
            ctx.set_shading(pkg.Shading(KX, KY, *shade))
        got = bs.convert_alone(ctx, buf)
    bad = bs.problems(got, expect)
    assert not bad, "%s in %d bands %s: %s" % (name, nb, rows, "\n".join(bad))


# -- C. set and cleared between frames in flight ------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_set_and_cleared_between_frames_in_flight(gpu_pkg, oracle, bits):
    """three frames in flight through one context: the first accepted with one set of parameters, the second with the
    correction off, the third with another list -- each keeps what it was accepted with"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng([13, bits])
    fmt = "ARGB64" if bits else "BGRx"
    deep = dict(bits=bits, out16=True) if bits else {}
    hot, cold = thresholds(bits)
    sets = [(hot, cold, cut_defects(w, h, [16, 32], rng)), None, (-1, cold // 2, cut_defects(w, h, [7], rng)), (hot, -1, None)]
    bufs = [sc.random_frame(rng, w, h, bits) for _ in sets]

    def model(buf, dpc):
        src = model_mosaic(buf, w, h, buf.shape[1], bits, False, dpc)
        if bits:
            return sc.expect(DEEP_12_TO_16.arm, src, sc.Case(w, h, "rggb", fmt, False, False))
        r, g, b = pkg.FORMATS[fmt]
        return oracle.bayer2rgb(src, w, "rggb", r, g, b)

    with pkg.Context(w, h, "rggb", fmt, inflight=4, device=0, **deep) as ctx:
        outs = []
        for i, (buf, dpc) in enumerate(zip(bufs, sets)):
            ctx.set_dpc(None if dpc is None else pkg.Dpc(*dpc))
            outs.append(np.full(model(bufs[0], None).shape, 0xA5, np.uint8))
            ctx.submit(np.ascontiguousarray(buf).reshape(-1), outs[-1], tag=i + 1)
        ctx.set_dpc(None)
        assert [ctx.wait() for _ in sets] == [1, 2, 3, 4]
    for i, (buf, dpc, out) in enumerate(zip(bufs, sets, outs)):
        assert np.array_equal(out, model(buf, dpc)), "frame %d" % i


def test_hipgraph_context_corrects_without_graphs_and_off_is_the_default(gpu_pkg, oracle):
    """a MIBAYER_FLAG_HIPGRAPH context launches without graphs while the correction is set; with it off -- never set, or
    set and taken away -- the bytes and the host path's own counters are the same"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng(14)
    buf = sc.random_frame(rng, w, h, 0)
    lst = cut_defects(w, h, [16], rng)
    fixed = model_mosaic(buf, w, h, buf.shape[1], 0, False, (30, 30, lst))
    r, g, b = pkg.FORMATS["BGRx"]
    counters = []
    for explicit in (False, True):
        with pkg.Context(w, h, "gbrg", "BGRx", flags=pkg.FLAG_HIPGRAPH, inflight=2, device=0) as ctx:
            if explicit:
                ctx.set_dpc(pkg.Dpc(30, 30, lst))
                assert np.array_equal(ctx.process_host(buf), oracle.bayer2rgb(fixed, w, "gbrg", r, g, b))
                ctx.set_dpc(None)
                before = ctx.host_stats()
            else:
                before = ctx.host_stats()
            plain = [ctx.process_host(buf).copy() for _ in range(3)]
            after = ctx.host_stats()
            assert all(np.array_equal(p, oracle.bayer2rgb(buf, w, "gbrg", r, g, b)) for p in plain)
            counters.append({k: after[k] - before[k] for k in ("submits", "waits")})
    assert counters[0] == counters[1] and counters[0]["submits"] >= 3, counters


# -- D. the pool ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_two_shard_pool_gives_the_same_bytes(gpu_pkg, oracle, bits):
    """two shards on one device, six frames under three settings in turn (the last: off): every frame comes back corrected
    with what the pool held when it was submitted, whichever shard converted it"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng([15, bits])
    fmt = "ARGB64" if bits else "RGBx"
    deep = dict(bits=bits, out16=True) if bits else {}
    hot, cold = thresholds(bits)
    sets = [(hot, cold, cut_defects(w, h, [16], rng)), (-1, -1, cut_defects(w, h, [20, 33], rng)), None]
    bufs = [sc.random_frame(rng, w, h, bits) for _ in range(6)]

    def model(buf, dpc):
        src = model_mosaic(buf, w, h, buf.shape[1], bits, False, dpc)
        if bits:
            return sc.expect(DEEP_12_TO_16.arm, src, sc.Case(w, h, "rggb", fmt, False, False))
        r, g, b = pkg.FORMATS[fmt]
        return oracle.bayer2rgb(src, w, "rggb", r, g, b)

    with pkg.Pool([0, 0], w, h, "rggb", fmt, inflight=2, **deep) as pool:
        outs = []
        for i, buf in enumerate(bufs):
            if i % 2 == 0:
                d = sets[i // 2]
                pool.set_dpc(None if d is None else pkg.Dpc(*d))
            if pool.pending() == pool.capacity:
                pool.wait()
            outs.append(np.full(model(bufs[0], None).shape, 0xA5, np.uint8))
            pool.submit(np.ascontiguousarray(buf).reshape(-1), outs[-1], tag=i + 1)
        while pool.pending():
            pool.wait()
    for i, (buf, out) in enumerate(zip(bufs, outs)):
        assert np.array_equal(out, model(buf, sets[i // 2])), "frame %d" % i


def test_pool_refuses_what_a_context_refuses(gpu_pkg):
    pkg = gpu_pkg
    L = pkg.lib()
    short = pkg.Dpc(4, 4)
    short.struct_size -= 4
    with pkg.Pool([0, 0], 64, 48, "rggb", "RGBx", inflight=2) as pool:
        for bad in (pkg.Dpc(256, 4), pkg.Dpc(4, -2), pkg.Dpc(4, 4, [(64, 0)]), pkg.Dpc(4, 4, [(0, 48)]), short):
            assert L.mibayer_pool_set_dpc(pool._h, bad) == pkg.ERR_ARG
        pool.set_dpc(pkg.Dpc(255, 0, [(63, 47)]))
        pool.set_dpc(None)
    with pkg.Pool([0], 64, 3, "rggb", "RGBx") as flat:
        assert L.mibayer_pool_set_dpc(flat._h, pkg.Dpc(4, 4)) == pkg.ERR_GEOMETRY
    with pkg.Pool([0, 0], 64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER) as inv:
        assert L.mibayer_pool_set_dpc(inv._h, pkg.Dpc(4, 4)) == pkg.ERR_ARG
        assert L.mibayer_pool_set_dpc(inv._h, None) == pkg.OK       # off is what it is already
