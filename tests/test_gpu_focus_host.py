"""GPU tests of the focus statistics on the host path (csrc/mibayer_abi.hip: mibayer_set_focus / mibayer_frame_focus,
one launch per frame behind the last band, the zones downloaded behind the frame) and through the pool: the zones are
the model's on the mosaic the models corrected, denoised and shaded, byte for byte, and nothing else changes.  The device
path is tests/test_gpu_focus.py."""
import numpy as np
import pytest

import band_cases as bc
import focus_model as fm
import nr_cases as nc
import stats_model as sm
import strip_cases as sc
import test_gpu_band_seams as bs
from test_gpu_dpc_host import cut_defects, fam_format, shading_of, thresholds
from test_gpu_nr_host import COMBOS, apply, curve_of, model_mosaic
from test_gpu_shading import HOST_FAMILIES, host_case

pytestmark = pytest.mark.gpu

SIZES = [(258, 37), (266, 70)]


def same(got, want, what=""):
    assert got.shape == want.shape
    for f in ("h", "v", "nh", "nv"):
        assert np.array_equal(got[f], want[f]), (what, f, np.argwhere(got[f] != want[f])[:4].tolist())


def focus_is_empty(pkg, ctx):
    out = np.zeros(1, fm.FOCUS_DTYPE)
    fn = pkg.lib().mibayer_pool_frame_focus if isinstance(ctx, pkg.Pool) else pkg.lib().mibayer_frame_focus
    return fn(ctx._h, out.ctypes.data, 1) == pkg.ERR_EMPTY


def frame_of(rng, w, h, bits):
    return sc.random_frame(rng, w, h, bits)


def model(buf, w, h, bits, zx, zy, thr):
    buf = np.ascontiguousarray(buf)
    vmax = (1 << (bits or 8)) - 1
    return fm.zone_focus(sm.samples(buf.reshape(-1), w, h, buf.shape[1], bits, False), zx, zy, thr, vmax)


# -- A. lab build: every band count, all eight combinations of the passes, with zones and a histogram ---------------------

@pytest.mark.parametrize("want", range(1, 9), ids=lambda n: "want%d" % n)
@pytest.mark.parametrize("size", SIZES, ids=lambda s: "%dx%d" % s)
@pytest.mark.parametrize("name", sorted(HOST_FAMILIES))
def test_every_band_count_under_all_eight_combinations(gpu_lab_pkg, monkeypatch, name, size, want):
    """MIBAYER_HOST_BANDS = 1 .. 8: the focus zones are taken once, behind the last band, on the mosaic the demosaic read
    -- the model applied to the model-corrected mosaic under every on / off combination of the defect, noise reduction and
    shading passes.  Zone statistics and a histogram are on as well: they, and the converted frame, are byte for byte
    those of the same frame with focus off"""
    pkg = gpu_lab_pkg
    fam = HOST_FAMILIES[name]()
    w, h = size
    case = host_case(fam, w, h)
    bits, sbe = fam_format(fam, case)
    vmax = (1 << (bits or 8)) - 1
    bs.set_wanted(monkeypatch, want)
    rng = np.random.default_rng([31, sorted(HOST_FAMILIES).index(name), w, want])
    sstride, _ = bc.strides(fam, w, h)
    buf = bs.random_frame(fam, case, rng, sstride)
    nb = bc.expected_bands(fam, case, want)
    rows = bc.band_rows(nb, h, fam.unit)
    hot, cold = thresholds(bits)
    dpc = (hot, cold, cut_defects(w, h, [y0 for y0, _ in rows[1:]] + nc.row_cuts(rows, h, fam.halo), rng))
    curve, shade = curve_of(bits), shading_of(w, h, bits, rng)
    zx, zy, thr = 3, 5, vmax // 8
    wants = {}
    with bs.open_banded(pkg, fam, case) as ctx:
        assert ctx.host_bands == nb
        ctx.set_stats(3, 2, vmax // 16, vmax - vmax // 16)
        ctx.set_hist(True)
        for combo in COMBOS:
            use_dpc, use_nr, use_shade = combo
            mosaic = model_mosaic(buf, w, h, sstride, bits, sbe, dpc if use_dpc else None, curve if use_nr else None,
                                  shade if use_shade else None)
            wants[combo] = fm.zone_focus(sm.samples(mosaic, w, h, sstride, bits, sbe), zx, zy, thr, vmax)
            apply(pkg, ctx, dpc if use_dpc else None, curve if use_nr else None, shade if use_shade else None)
            ctx.set_focus(0, 0)
            off = bs.convert_alone(ctx, buf).copy()
            zones_off, hist_off = ctx.frame_stats(), ctx.frame_hist()
            assert focus_is_empty(pkg, ctx)
            ctx.set_focus(zx, zy, thr)
            on = bs.convert_alone(ctx, buf)
            where = "%s %dx%d in %d bands dpc=%d nr=%d shading=%d" % ((name, w, h, nb) + combo)
            assert np.array_equal(on, off), where
            assert ctx.frame_stats().tobytes() == zones_off.tobytes() and np.array_equal(ctx.frame_hist(), hist_off), where
            same(ctx.frame_focus(), wants[combo], where)
    assert len({v.tobytes() for v in wants.values()}) == len(COMBOS), "two combinations expect the same zones"


# -- B. frames in flight ------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_grid_changed_between_frames_in_flight(gpu_pkg, bits):
    """four frames in flight through one context, each accepted under another grid and threshold (the third under none):
    each keeps what it was accepted with, and the converted bytes are those of a context that never measured"""
    pkg = gpu_pkg
    w, h = 258, 37
    vmax = (1 << (bits or 8)) - 1
    rng = np.random.default_rng([32, bits])
    fmt = "ARGB64" if bits else "BGRx"
    deep = dict(bits=bits, out16=True) if bits else {}
    grids = [(3, 5, vmax // 8), (1, 1, 0), None, (64, 18, 2 * vmax)]
    bufs = [frame_of(rng, w, h, bits) for _ in grids]
    with pkg.Context(w, h, "rggb", fmt, device=0, **deep) as never:
        plain = [never.process_host(np.ascontiguousarray(b).reshape(-1)).copy() for b in bufs]
    with pkg.Context(w, h, "rggb", fmt, inflight=4, device=0, **deep) as ctx:
        assert focus_is_empty(pkg, ctx)          # before the first frame
        outs = []
        for i, (buf, g) in enumerate(zip(bufs, grids)):
            ctx.set_focus(*(g or (0, 0)))
            outs.append(np.full_like(plain[0], 0xA5))
            ctx.submit(np.ascontiguousarray(buf).reshape(-1), outs[-1], tag=i + 1)
        ctx.set_focus(0, 0)
        for i, (buf, g) in enumerate(zip(bufs, grids)):
            assert ctx.wait() == i + 1
            if g is None:
                assert focus_is_empty(pkg, ctx)
                continue
            ctx._fzones = (g[1], g[0])
            same(ctx.frame_focus(), model(buf, w, h, bits, *g), "frame %d" % i)
            wrong = np.zeros(2, fm.FOCUS_DTYPE)
            assert pkg.lib().mibayer_frame_focus(ctx._h, wrong.ctypes.data, g[0] * g[1] + 1) == pkg.ERR_ARG
        for o, p in zip(outs, plain):
            assert np.array_equal(o, p)


def test_two_frames_in_flight_with_every_measurement(gpu_pkg):
    """zones, histogram and focus zones together, two in flight: each frame's own"""
    pkg = gpu_pkg
    w, h = 266, 70
    rng = np.random.default_rng(33)
    bufs = [frame_of(rng, w, h, 0) for _ in range(5)]
    with pkg.Context(w, h, "gbrg", "RGBx", inflight=2, device=0) as ctx:
        ctx.set_stats(4, 3, 8, 247)
        ctx.set_hist(True)
        ctx.set_focus(5, 2, 40)
        outs = [np.zeros((h, 4 * w), np.uint8) for _ in bufs]
        done = 0
        for i in range(len(bufs) + 2):
            if i >= 2:
                assert ctx.wait() == done + 1
                S = sm.samples(bufs[done], w, h, bufs[done].shape[1])
                same(ctx.frame_focus(), fm.zone_focus(S, 5, 2, 40, 255), "frame %d" % done)
                assert ctx.frame_stats().tobytes() == sm.zone_stats(S, 4, 3, 8, 247).tobytes()
                assert int(ctx.frame_hist().sum()) == w * h
                done += 1
            if i < len(bufs):
                ctx.submit(bufs[i].reshape(-1), outs[i], tag=i + 1)


def test_hipgraph_context_measures_without_graphs_and_off_is_the_default(gpu_pkg):
    """a MIBAYER_FLAG_HIPGRAPH context launches without graphs while focus is on; with it off -- never set, or set and
    taken away -- the bytes and the host path's own counters are the same"""
    pkg = gpu_pkg
    w, h = 258, 37
    rng = np.random.default_rng(34)
    buf = frame_of(rng, w, h, 0)
    counters, frames = [], []
    for explicit in (False, True):
        with pkg.Context(w, h, "gbrg", "BGRx", flags=pkg.FLAG_HIPGRAPH, inflight=2, device=0) as ctx:
            if explicit:
                ctx.set_focus(3, 5, 30)
                frames.append(ctx.process_host(buf).copy())
                same(ctx.frame_focus(), model(buf, w, h, 0, 3, 5, 30))
                ctx.set_focus(0, 0)
            before = ctx.host_stats()
            plain = [ctx.process_host(buf).copy() for _ in range(3)]
            after = ctx.host_stats()
            assert focus_is_empty(pkg, ctx)
            frames += plain
            counters.append({k: after[k] - before[k] for k in ("submits", "waits")})
    assert all(np.array_equal(f, frames[0]) for f in frames)
    assert counters[0] == counters[1] and counters[0]["submits"] >= 3, counters


# -- C. the pool ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_two_shard_pool_keeps_grid_and_zones_with_each_frame(gpu_pkg, bits):
    """two shards on one device, seven frames under three grids in turn (the last: off), zone statistics on throughout:
    mibayer_pool_frame_focus after mibayer_pool_wait answers for that frame, whichever shard converted it"""
    pkg = gpu_pkg
    w, h, n = 258, 37, 7
    vmax = (1 << (bits or 8)) - 1
    rng = np.random.default_rng([35, bits])
    fmt = "ARGB64" if bits else "RGBx"
    deep = dict(bits=bits, out16=True) if bits else {}
    grids = [(3, 2, vmax // 8), (1, 1, 0), (3, 2, vmax // 8), None]
    bufs = [frame_of(rng, w, h, bits) for _ in range(n)]
    with pkg.Context(w, h, "rggb", fmt, device=0, **deep) as never:
        plain = [never.process_host(np.ascontiguousarray(b).reshape(-1)).copy() for b in bufs]
    with pkg.Pool([0, 0], w, h, "rggb", fmt, inflight=2, **deep) as pool:
        assert focus_is_empty(pkg, pool)
        with pytest.raises(pkg.MibayerError):
            pool.set_focus(200, 1, 0)
        with pytest.raises(pkg.MibayerError):
            pool.set_focus(1, 1, 2 * vmax + 1)
        pool.set_stats(2, 2, 0, vmax)
        outs = [np.full_like(plain[0], 0xA5) for _ in bufs]
        done = 0

        def collect():
            nonlocal done
            assert pool.wait() == done + 1
            g = grids[done // 2]
            S = sm.samples(np.ascontiguousarray(bufs[done]).reshape(-1), w, h, bufs[done].shape[1], bits, False)
            assert pool.frame_stats().tobytes() == sm.zone_stats(S, 2, 2, 0, vmax).tobytes()
            if g is None:
                assert focus_is_empty(pkg, pool)
            else:
                pool._fzones = (g[1], g[0])
                same(pool.frame_focus(), fm.zone_focus(S, g[0], g[1], g[2], vmax), "frame %d" % done)
            done += 1

        for i, buf in enumerate(bufs):
            if i % 2 == 0:
                pool.set_focus(*(grids[i // 2] or (0, 0)))
            if pool.pending() == pool.capacity:
                collect()
            pool.submit(np.ascontiguousarray(buf).reshape(-1), outs[i], tag=i + 1)
        while pool.pending():
            collect()
        assert done == n and all(np.array_equal(o, p) for o, p in zip(outs, plain))


def test_pool_failover_redo_keeps_the_zones(gpu_pkg):
    pkg = gpu_pkg
    w, h, n = 66, 18, 6
    rng = np.random.default_rng(36)
    bufs = [frame_of(rng, w, h, 0) for _ in range(n)]
    wants = [model(b, w, h, 0, 2, 2, 20) for b in bufs]
    with pkg.Pool([0, 0], w, h, inflight=2) as pool:
        pool.set_focus(2, 2, 20)
        pool.inject_fault(1, 0)         # shard 1 reports a device error for its first frame: redone on shard 0
        dsts = [np.zeros((h, 4 * w), np.uint8) for _ in bufs]
        done = 0

        def collect():
            nonlocal done
            assert pool.wait() == done + 1
            same(pool.frame_focus(), wants[done], "frame %d" % done)
            done += 1

        for i in range(n):
            while True:
                # the capacity shrinks with the dropped shard, and the survivor's ring may be full before the pool is
                if pool.pending() >= pkg.lib().mibayer_pool_capacity(pool._h):
                    collect()
                    continue
                try:
                    pool.submit(bufs[i].reshape(-1), dsts[i], tag=i + 1)
                    break
                except pkg.MibayerError as e:
                    assert e.status == pkg.ERR_BUSY
                    collect()
        while pool.pending():
            collect()
        assert done == n and pool.alive() == 1


def test_pool_refuses_focus_on_an_rgb2bayer_pool(gpu_pkg):
    pkg = gpu_pkg
    with pkg.Pool([0, 0], 64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER) as inv:
        assert pkg.lib().mibayer_pool_set_focus(inv._h, 1, 1, 0) == pkg.ERR_ARG
        assert focus_is_empty(pkg, inv)
