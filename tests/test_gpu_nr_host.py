"""GPU tests of the noise reduction on the host path (csrc/mibayer_abi.hip: one more mosaic per ring slot, the pass
between the defect pass and the shading pass, rows four behind the defect pass in a banded frame): the bytes are the
demosaic model's on the mosaic the models corrected, denoised and shaded in that order, byte for byte.  The device path
is tests/test_gpu_nr.py."""
import itertools

import numpy as np
import pytest

import band_cases as bc
import dpc_model as dm
import nr_cases as nc
import nr_model as nm
import shading_model as shm
import strip_cases as sc
import test_gpu_band_seams as bs
from test_gpu_dpc_host import KX, KY, LAB_SIZE, cut_defects, fam_format, shading_of, thresholds
from test_gpu_shading import DEEP_12_TO_16, HOST_FAMILIES, HOST_SIZE, host_case

pytestmark = pytest.mark.gpu

COMBOS = list(itertools.product((False, True), repeat=3))       # (dpc, nr, shading)


def curve_of(bits):
    """rising with the level, a sixth of the range in the middle: about a third of a random frame's neighbours are in"""
    depth = bits or 8
    t = min(nm.t_max(depth), ((1 << depth) - 1) // 6)
    return [t * (8 + i) // 16 for i in range(17)]


def model_mosaic(buf, w, h, sstride, bits, sbe, dpc=None, curve=None, shade=None):
    """the mosaic everything behind the passes reads: corrected, then denoised, then shaded"""
    out = np.ascontiguousarray(buf).reshape(-1)
    if dpc is not None:
        hot, cold, lst = dpc
        out = dm.correct_raw(out, out, w, h, sstride, bits, sbe, hot, cold, lst)
    if curve is not None:
        out = nm.denoise_raw(out, out, w, h, sstride, bits, sbe, curve)
    if shade is not None:
        table, blacks = shade
        out = shm.shade_raw(out, table, KX, KY, blacks, w, h, sstride, bits, sbe)
    return out.reshape(h, sstride)


def apply(pkg, ctx, dpc, curve, shade):
    ctx.set_dpc(None if dpc is None else pkg.Dpc(*dpc))
    ctx.set_nr(None if curve is None else pkg.Nr(curve))
    ctx.set_shading(None if shade is None else pkg.Shading(KX, KY, *shade))


def all_combinations(pkg, oracle, ctx, fam, case, buf, sstride, bits, sbe, dpc, curve, shade, where):
    """the eight on / off combinations on one context, one after the other; returns the bytes with everything off"""
    w, h = case.w, case.h
    wants = {}
    for use_dpc, use_nr, use_shade in COMBOS:
        mosaic = model_mosaic(buf, w, h, sstride, bits, sbe, dpc if use_dpc else None, curve if use_nr else None,
                              shade if use_shade else None)
        want = bs.expect(pkg, oracle, fam, mosaic, case)
        apply(pkg, ctx, dpc if use_dpc else None, curve if use_nr else None, shade if use_shade else None)
        got = bs.convert_alone(ctx, buf)
        bad = bs.problems(got, want)
        assert not bad, "%s dpc=%d nr=%d shading=%d: %s" % (where, use_dpc, use_nr, use_shade, "\n".join(bad))
        wants[(use_dpc, use_nr, use_shade)] = want
    assert len({v.tobytes() for v in wants.values()}) == len(COMBOS), "two combinations expect the same bytes"
    return wants[(False, False, False)]


# -- A. product build: banded by the frame's bytes, and two frames in flight -----------------------------------------------

@pytest.mark.parametrize("name", sorted(HOST_FAMILIES))
def test_host_path_denoises_every_row_once(gpu_pkg, gpu_lab_pkg, oracle, name):
    """process_host (banded: the frame has the link to itself) under all eight combinations of the three passes, and
    submit / wait with two in flight (never banded) under all three: the bytes of the models; with the curve taken away
    again the bytes are those of a context that never had one, and a zero curve gives them too"""
    pkg = gpu_pkg
    fam = HOST_FAMILIES[name]()
    w, h = HOST_SIZE
    case = host_case(fam, w, h)
    bits, sbe = fam_format(fam, case)
    rng = np.random.default_rng([21, sorted(HOST_FAMILIES).index(name)])
    sstride, _ = bc.strides(fam, w, h)
    buf = bs.random_frame(fam, case, rng, sstride)
    nb = bc.expected_bands(fam, case)
    assert nb >= 2
    rows = bc.band_rows(nb, h, fam.unit)
    hot, cold = thresholds(bits)
    dpc = (hot, cold, cut_defects(w, h, [y0 for y0, _ in rows[1:]] + nc.row_cuts(rows, h, fam.halo), rng))
    curve, shade = curve_of(bits), shading_of(w, h, bits, rng)
    with bs.open_banded(gpu_lab_pkg, fam, case) as lab:
        assert lab.host_bands == nb, (name, lab.host_bands, nb)
    with bs.open_banded(pkg, fam, case) as never:
        before = bs.convert_alone(never, buf).copy()
    with bs.open_banded(pkg, fam, case) as ctx:
        plain = all_combinations(pkg, oracle, ctx, fam, case, buf, sstride, bits, sbe, dpc, curve, shade, name + " banded")
        assert not bs.problems(before, plain)
        apply(pkg, ctx, None, [0] * 17, None)           # on, and the identity: every sample is copied
        assert np.array_equal(bs.convert_alone(ctx, buf), before)
        apply(pkg, ctx, None, None, None)
        assert ctx.get_nr() is None
        assert np.array_equal(bs.convert_alone(ctx, buf), before), "the bytes with the curve off are not those from before"
    want = bs.expect(pkg, oracle, fam, model_mosaic(buf, w, h, sstride, bits, sbe, dpc, curve, shade), case)
    with bs.open_banded(pkg, fam, case, inflight=2) as ctx:
        apply(pkg, ctx, dpc, curve, shade)
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
def test_every_band_count_under_all_eight_combinations(gpu_lab_pkg, oracle, monkeypatch, name, want):
    """MIBAYER_HOST_BANDS = 1 .. 8 on a frame of 116 rows of random samples (a third of the neighbours included), listed
    defects around every band cut and around every row at which the noise reduction's own launches end.  A row is denoised
    when the rows four below it have had the defect pass, which itself runs two rows behind the upload"""
    pkg = gpu_lab_pkg
    fam = HOST_FAMILIES[name]()
    w, h = LAB_SIZE
    case = host_case(fam, w, h)
    bits, sbe = fam_format(fam, case)
    bs.set_wanted(monkeypatch, want)
    rng = np.random.default_rng([22, sorted(HOST_FAMILIES).index(name), want])
    sstride, _ = bc.strides(fam, w, h)
    buf = bs.random_frame(fam, case, rng, sstride)
    nb = bc.expected_bands(fam, case, want)
    rows = bc.band_rows(nb, h, fam.unit)
    cuts = nc.row_cuts(rows, h, fam.halo)
    assert len(cuts) == nb - 1
    hot, cold = thresholds(bits)
    dpc = (hot, cold, cut_defects(w, h, [y0 for y0, _ in rows[1:]] + cuts + [y + 4 for y in cuts if y + 4 < h], rng))
    curve, shade = curve_of(bits), shading_of(w, h, bits, rng)
    share = nm.included(bs_samples(buf, w, h, sstride, bits, sbe), curve, bits or 8).mean()
    assert 0.1 < share < 0.9, share
    with bs.open_banded(pkg, fam, case) as ctx:
        assert ctx.host_bands == nb
        all_combinations(pkg, oracle, ctx, fam, case, buf, sstride, bits, sbe, dpc, curve, shade,
                         "%s in %d bands %s" % (name, nb, rows))


def bs_samples(buf, w, h, sstride, bits, sbe):
    import stats_model as sm
    return sm.samples(np.ascontiguousarray(buf).reshape(-1), w, h, sstride, bits, sbe)


# -- C. changed between frames in flight ----------------------------------------------------------------------------------------

def small_model(pkg, oracle, buf, w, h, bits, fmt, curve):
    src = model_mosaic(buf, w, h, buf.shape[1], bits, False, None, curve)
    if bits:
        return sc.expect(DEEP_12_TO_16.arm, src, sc.Case(w, h, "rggb", fmt, False, False))
    r, g, b = pkg.FORMATS[fmt]
    return oracle.bayer2rgb(src, w, "rggb", r, g, b)


@pytest.mark.parametrize("bits", [0, 12])
def test_curve_changed_between_frames_in_flight(gpu_pkg, oracle, bits):
    """four frames in flight through one context: each accepted under another curve (the second under none) keeps the one
    it was accepted with"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng([23, bits])
    fmt = "ARGB64" if bits else "BGRx"
    deep = dict(bits=bits, out16=True) if bits else {}
    base = curve_of(bits)
    curves = [base, None, base[::-1], [base[8] // 2] * 17]
    bufs = [sc.random_frame(rng, w, h, bits) for _ in curves]
    with pkg.Context(w, h, "rggb", fmt, inflight=4, device=0, **deep) as ctx:
        outs = []
        for i, (buf, curve) in enumerate(zip(bufs, curves)):
            ctx.set_nr(None if curve is None else pkg.Nr(curve))
            outs.append(np.full(small_model(pkg, oracle, bufs[0], w, h, bits, fmt, None).shape, 0xA5, np.uint8))
            ctx.submit(np.ascontiguousarray(buf).reshape(-1), outs[-1], tag=i + 1)
        ctx.set_nr(None)
        assert [ctx.wait() for _ in curves] == [1, 2, 3, 4]
    models = [small_model(pkg, oracle, buf, w, h, bits, fmt, curve) for buf, curve in zip(bufs, curves)]
    for i, (out, want) in enumerate(zip(outs, models)):
        assert np.array_equal(out, want), "frame %d" % i
    assert not np.array_equal(models[0], small_model(pkg, oracle, bufs[0], w, h, bits, fmt, None))


def test_hipgraph_context_denoises_without_graphs_and_off_is_the_default(gpu_pkg, oracle):
    """a MIBAYER_FLAG_HIPGRAPH context launches without graphs while a curve is set; with it off -- never set, or set and
    taken away -- the bytes and the host path's own counters are the same"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng(24)
    buf = sc.random_frame(rng, w, h, 0)
    curve = curve_of(0)
    clean = model_mosaic(buf, w, h, buf.shape[1], 0, False, None, curve)
    r, g, b = pkg.FORMATS["BGRx"]
    counters = []
    for explicit in (False, True):
        with pkg.Context(w, h, "gbrg", "BGRx", flags=pkg.FLAG_HIPGRAPH, inflight=2, device=0) as ctx:
            if explicit:
                ctx.set_nr(pkg.Nr(curve))
                assert np.array_equal(ctx.process_host(buf), oracle.bayer2rgb(clean, w, "gbrg", r, g, b))
                ctx.set_nr(None)
            before = ctx.host_stats()
            plain = [ctx.process_host(buf).copy() for _ in range(3)]
            after = ctx.host_stats()
            assert all(np.array_equal(p, oracle.bayer2rgb(buf, w, "gbrg", r, g, b)) for p in plain)
            counters.append({k: after[k] - before[k] for k in ("submits", "waits")})
    assert counters[0] == counters[1] and counters[0]["submits"] >= 3, counters


# -- D. the pool ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_two_shard_pool_gives_the_same_bytes(gpu_pkg, oracle, bits):
    """two shards on one device, six frames under three curves in turn (the last: off): every frame comes back denoised
    with what the pool held when it was submitted, whichever shard converted it"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng([25, bits])
    fmt = "ARGB64" if bits else "RGBx"
    deep = dict(bits=bits, out16=True) if bits else {}
    base = curve_of(bits)
    curves = [base, base[::-1], None]
    bufs = [sc.random_frame(rng, w, h, bits) for _ in range(6)]
    with pkg.Pool([0, 0], w, h, "rggb", fmt, inflight=2, **deep) as pool:
        outs = []
        for i, buf in enumerate(bufs):
            if i % 2 == 0:
                c = curves[i // 2]
                pool.set_nr(None if c is None else pkg.Nr(c))
            if pool.pending() == pool.capacity:
                pool.wait()
            outs.append(np.full(small_model(pkg, oracle, bufs[0], w, h, bits, fmt, None).shape, 0xA5, np.uint8))
            pool.submit(np.ascontiguousarray(buf).reshape(-1), outs[-1], tag=i + 1)
        while pool.pending():
            pool.wait()
    for i, (buf, out) in enumerate(zip(bufs, outs)):
        assert np.array_equal(out, small_model(pkg, oracle, buf, w, h, bits, fmt, curves[i // 2])), "frame %d" % i


def test_pool_refuses_what_a_context_refuses(gpu_pkg):
    pkg = gpu_pkg
    L = pkg.lib()
    short, high = pkg.Nr(4), pkg.Nr(4)
    short.struct_size -= 4
    high.curve[3] = 256
    with pkg.Pool([0, 0], 64, 48, "rggb", "RGBx", inflight=2) as pool:
        for bad in (short, high):
            assert L.mibayer_pool_set_nr(pool._h, bad) == pkg.ERR_ARG
        pool.set_nr(pkg.Nr(255))
        pool.set_nr(None)
    with pkg.Pool([0], 64, 4, "rggb", "RGBx") as flat:
        assert L.mibayer_pool_set_nr(flat._h, pkg.Nr(4)) == pkg.ERR_GEOMETRY
    with pkg.Pool([0, 0], 64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER) as inv:
        assert L.mibayer_pool_set_nr(inv._h, pkg.Nr(4)) == pkg.ERR_ARG
        assert L.mibayer_pool_set_nr(inv._h, None) == pkg.OK        # off is what it is already
