"""GPU tests of the banded host path (choose_host_bands, enqueue_frame_banded, launch_frames over a unit range,
download_frame; csrc/mibayer_abi.hip): every band cut, seam and download of every kernel family, bit-exact against the
models the families' own tests use (tests/strip_cases.py `expect`, rgb24_model, planar_model, the CPU oracle for the
tile variants).  The tables are tests/band_cases.py; tests/test_band_cases.py shows without a GPU what they reach.

Every frame is a few dozen rows high: the band cut follows the frame's BYTES, so a destination stride far above the row
(band_cases.banded_stride: the first stride at which dst_bytes reaches 16 MiB) bands a frame of 266 x 52 pixels.  The
host destination is prefilled, and every byte of its padding -- the whole stride -- must be left as it was.

What these tests cannot show (tests/test_band_cases.py::test_no_band_reads_below_its_upload guards the rule instead): a
halo that is too small makes a band read rows whose upload is merely QUEUED, and whether it sees stale bytes is a matter
of timing."""
import threading

import numpy as np
import pytest

import band_cases as bc
import hist_model as hm
import planar_model as pm
import rgb24_model as rm
import stats_model as sm
import strip_cases as sc
import tile_cases as tc

pytestmark = pytest.mark.gpu

FILL = 0xA5
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)      # rows sum to 1 (tests/test_gpu_colour.py)
COUNT = {"contexts": 0, "frames": 0}    # of the running test (reported with -s / -rA)
RACED_FRAMES = 24               # section F: frames converted while another thread switches the stage


def reset_count():
    COUNT["contexts"] = COUNT["frames"] = 0


def report_count():
    print("contexts opened: %(contexts)d, host-path frames: %(frames)d" % COUNT)


# -- one family, one case -------------------------------------------------------------------------------------------------

def stage_of(pkg, fam, gains=(1.9, 1.0, 1.6)):
    """a stage that exercises every step (tests/test_gpu_strip_geometry.py); None for a plain arm"""
    if fam.kind == "tile" or not fam.arm.colour:
        return None
    return pkg.Colour.make(black=(1 << sc.depth_of(fam.arm.bits)) // 16, gains=gains, ccm=CCM, curve=pkg.TONE_SRGB)


def model_kw(col):
    return None if col is None else dict(black=tuple(col.black[:]), matrix=tuple(col.matrix[:]), tone=col.tone_table())


def open_ctx(pkg, fam, case, col=None, src_stride=0, dst_stride=0, inflight=1, variant=None):
    COUNT["contexts"] += 1
    if fam.kind == "tile":
        vid = tc.variant_id(pkg, fam.name) if variant is None else variant
        return pkg.Context(case.w, case.h, case.order, case.layout, src_stride=src_stride, dst_stride=dst_stride,
                           variant=vid, inflight=inflight, device=0)
    arm = fam.arm
    colour = (col if col is not None else True) if arm.colour else None
    if fam.kind == "strip":
        return pkg.Context(case.w, case.h, case.order, case.layout, src_stride=src_stride, dst_stride=dst_stride,
                           bits=arm.bits, src_big_endian=case.sbe, out16=arm.out16, dst_big_endian=case.dbe,
                           method=arm.method, colour=colour, inflight=inflight, device=0)
    flags = pkg.FLAG_DST_PLANAR if fam.kind == "planar" else 0
    return pkg.Context(case.w, case.h, case.order, case.fmt, src_stride=src_stride, dst_stride=dst_stride, bits=arm.bits,
                       src_big_endian=arm.sbe, method=arm.method, colour=colour, flags=flags, inflight=inflight, device=0)


def random_frame(fam, case, rng, sstride):
    """(h, sstride) bytes: random samples with junk above the depth, 0x5A in the row padding"""
    if fam.kind == "tile":
        buf = np.full((case.h, sstride), 0x5A, np.uint8)
        buf[:, :case.w] = rng.integers(0, 256, (case.h, case.w))
        return buf
    sbe = case.sbe if fam.kind == "strip" else fam.arm.sbe
    return sc.random_frame(rng, case.w, case.h, fam.arm.bits, sstride, sbe)


def expect(pkg, oracle, fam, buf, case, col=None):
    """the model's written bytes, (planes * h, row_bytes): the rows of plane 0, then of plane 1, ..."""
    kw = model_kw(col)
    if fam.kind == "tile":
        r, g, b = pkg.FORMATS[case.layout]
        return oracle.bayer2rgb(buf, case.w, case.order, r, g, b)
    if fam.kind == "strip":
        return sc.expect(fam.arm, buf, case, **(kw or {}))
    arm = fam.arm
    if fam.kind == "rgb24":
        out = rm.bayer2rgb_rgb24(buf, case.w, case.h, case.order, case.fmt, bits=arm.bits, method=arm.method, colour=kw,
                                 src_big_endian=arm.sbe, src_stride=buf.shape[1])
        return out[:, :3 * case.w]
    out = pm.bayer2rgb_planar(buf, case.w, case.h, case.order, case.fmt, bits=arm.bits, method=arm.method, colour=kw,
                              src_big_endian=arm.sbe, src_stride=buf.shape[1])
    return out[:, :, :case.w].reshape(3 * case.h, case.w)


_inputs = {}


def inputs(pkg, oracle, fam, case):
    """a case's frame and its expected bytes: computed once, shared by the product and the lab sweeps, read-only"""
    key = (fam.name, case)
    if key not in _inputs:
        sstride, _ = bc.strides(fam, case.w, case.h)
        rng = np.random.default_rng([bc.LAB_FAMILIES.index(fam), case.w, case.h])
        buf = random_frame(fam, case, rng, sstride)
        want = np.ascontiguousarray(expect(pkg, oracle, fam, buf, case, stage_of(pkg, fam)))
        buf.setflags(write=False)
        want.setflags(write=False)
        _inputs[key] = (buf, want)
    return _inputs[key]


def forget_inputs(fam):
    """drop a family's frames and expectations (a few MB each): its last sweep has run.  A later use computes them
    again"""
    for key in [k for k in _inputs if k[0] == fam.name]:
        del _inputs[key]


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else "%d bytes differ, first at row %d byte %d (got %d, want %d), rows %s" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])], rows_of(bad[:, 0]))


def rows_of(rows):
    """'3-17 32-35': the runs of rows that differ"""
    rows = sorted(set(int(r) for r in rows))
    runs, start = [], rows[0]
    for a, b in zip(rows, rows[1:] + [None]):
        if b != a + 1:
            runs.append("%d-%d" % (start, a) if a > start else "%d" % a)
            start = b
    return " ".join(runs)


def host_frame(ctx):
    return np.full((ctx.dst_rows, ctx.dst_stride), FILL, np.uint8)


def convert_alone(ctx, buf):
    """mibayer_process_host: the frame has the link to itself -- the banded path where the context bands"""
    COUNT["frames"] += 1
    return ctx.process_host(buf, host_frame(ctx))


def problems(got, want):
    """what is wrong with a host-path frame (rows, stride): the written bytes, and the padding over the whole stride"""
    n = want.shape[1]
    bad = []
    if not (got[:, n:] == FILL).all():
        rows = np.argwhere((got[:, n:] != FILL).any(axis=1))[:, 0]
        bad.append("row padding of the destination written in rows %s" % rows_of(rows))
    if not np.array_equal(got[:, :n], want):
        bad.append(first_difference(got[:, :n], want))
    return bad


def where(fam, case, nb):
    return "%s %dx%d %s (h %% %d = %d) in %d bands %s" % (fam.name, case.w, case.h, case.order, fam.unit,
                                                          case.h % fam.unit, nb, bc.band_rows(nb, case.h, fam.unit))


def open_banded(pkg, fam, case, inflight=1, col=None, variant=None):
    sstride, dstride = bc.strides(fam, case.w, case.h)
    ctx = open_ctx(pkg, fam, case, stage_of(pkg, fam) if col is None else col, sstride, dstride, inflight, variant)
    assert (ctx.src_stride, ctx.dst_stride) == (sstride, dstride) and ctx.dst_rows == bc.planes(fam) * case.h
    assert ctx.dst_bytes >= bc.BAND_MIN_BYTES > ctx.dst_bytes - 16 * ctx.dst_rows, (fam.name, case, ctx.dst_bytes)
    return ctx


# -- A. product build: every family, every height of its unit, both widths ------------------------------------------------

def run_product(pkg, oracle, fam, cases):
    bad = []
    for case in cases:
        buf, want = inputs(pkg, oracle, fam, case)
        nb = bc.expected_bands(fam, case)
        with open_banded(pkg, fam, case) as ctx:
            got = convert_alone(ctx, buf)
        bad += ["%s: %s" % (where(fam, case, nb), p) for p in problems(got, want)]
        # the same frame, two in flight through a context of the same geometry: never banded, the same bytes
        with open_banded(pkg, fam, case, inflight=2) as ctx:
            outs = [host_frame(ctx) for _ in range(2)]
            src = np.ascontiguousarray(buf).reshape(-1)
            for i, o in enumerate(outs):
                ctx.submit(src, o, tag=i + 1)
            COUNT["frames"] += 2
            assert [ctx.wait(), ctx.wait()] == [1, 2] and ctx.pending() == 0
        for o in outs:
            if not np.array_equal(o, got):
                bad.append("%s: banded and unbanded differ: %s" % (where(fam, case, nb), first_difference(got, o)))
    return bad


@pytest.mark.parametrize("half", [0, 1], ids=["heights_1st_3rd", "heights_2nd_4th"])
@pytest.mark.parametrize("fam", bc.PRODUCT_FAMILIES, ids=bc.family_id)
def test_every_band_cut_of_the_product_build(gpu_pkg, oracle, fam, half):
    """every height of the family's unit at both widths, in two tests (band_cases.product_half: no height is left out,
    tests/test_band_cases.py::test_cases_rotate_and_lab_cases_are_product_cases)"""
    reset_count()
    cases = bc.product_half(fam, half)
    assert sorted({c.h for c in cases}) == sorted(bc.HEIGHTS[fam.unit][half::2]) and {c.w for c in cases} == set(bc.widths(fam))
    assert len(cases) == 2 * len(bc.HEIGHTS[fam.unit][half::2]) and len({bc.expected_bands(fam, c) for c in cases}) >= 3
    bad = run_product(gpu_pkg, oracle, fam, cases)
    report_count()
    assert not bad, "\n".join(bad)


# -- B. lab build: the same heights under MIBAYER_HOST_BANDS, the library's count against the model's --------------------

def set_wanted(monkeypatch, env):
    if env is None:
        monkeypatch.delenv("MIBAYER_HOST_BANDS", raising=False)
    else:
        monkeypatch.setenv("MIBAYER_HOST_BANDS", str(env))


@pytest.mark.parametrize("env", bc.LAB_WANTS, ids=lambda e: "unset" if e is None else "want%d" % e)
@pytest.mark.parametrize("fam", bc.LAB_FAMILIES, ids=bc.family_id)
def test_every_band_cut_of_the_lab_build(gpu_lab_pkg, oracle, monkeypatch, fam, env):
    """ctx.host_bands (mibayer_internal_host_bands) == band_cases.host_bands for every case BEFORE it converts: what
    ties the model the product sweep relies on to the library"""
    reset_count()
    pkg = gpu_lab_pkg
    set_wanted(monkeypatch, env)
    bad, counts = [], set()
    for case in bc.lab_cases(fam, env):
        buf, want = inputs(pkg, oracle, fam, case)
        nb = bc.expected_bands(fam, case, env)
        counts.add(nb)
        with open_banded(pkg, fam, case) as ctx:
            if ctx.host_bands != nb:
                bad.append("%s: the library cuts %d bands" % (where(fam, case, nb), ctx.host_bands))
                continue
            got = convert_alone(ctx, buf)
        bad += ["%s: %s" % (where(fam, case, nb), p) for p in problems(got, want)]
    report_count()
    if env == bc.LAB_WANTS[-1]:         # the family's sweeps run one after the other, this setting last
        forget_inputs(fam)
    # the heights of every unit hold one that is not cut at all and one that is cut into all the bands wanted
    assert (min(counts), max(counts)) == ((1, 1) if fam.persistent else (1, bc.wanted(env))), (fam.name, env, counts)
    assert not bad, "\n".join(bad)


def test_the_band_count_is_not_exported_by_the_product_build(gpu_pkg):
    with gpu_pkg.Context(266, 52, device=0) as ctx:
        with pytest.raises(gpu_pkg.MibayerErrorNoLib):
            ctx.host_bands


# -- C. a plan change re-cuts the frame ------------------------------------------------------------------------------------

@pytest.mark.parametrize("env", [None, 8, 3], ids=["unset", "want8", "want3"])
def test_a_plan_change_recuts_the_bands_lab(gpu_lab_pkg, oracle, monkeypatch, env):
    """one context, one slot: variant 3, then 1, 2, 3 and 1 again (units 32, 8, 16, 32, 8).  The slot and its band
    events are made at the first frame, for the 4 bands (8 wanted; 2 with 3 wanted) of that moment; the next plan cuts
    7 (3), so bands 4 .. 6 (2) get their events in enqueue_frame_banded, when they first need them; then the count
    shrinks and grows once more.  With the default 4 wanted every plan cuts 4 bands and only the rows per unit change"""
    set_wanted(monkeypatch, env)
    recut(gpu_lab_pkg, oracle, env, True)


def test_a_plan_change_recuts_the_bands(gpu_pkg, oracle):
    """the product build: 4 bands under every plan of the walk, cut in units of 32, 8 and 16 rows"""
    recut(gpu_pkg, oracle, None, False)


def recut(pkg, oracle, env, lab):
    reset_count()
    w, h = bc.RECUT_SIZE
    fam = bc.family(tc.NT_NAMES[0])
    case = tc.rotate(3, w, h)
    buf, want = inputs(pkg, oracle, fam, case)
    units = [tc.shape_of(name).tile_h for name in bc.RECUT_PLANS]
    counts = [bc.host_bands(bc.wanted(env), bc.BAND_MIN_BYTES, h, u) for u in units]
    assert counts[0] == min(counts) and (env is None or counts[0] < counts[1]), counts      # the slot is born small
    with open_banded(pkg, fam, case, variant=0) as ctx:
        for step, name in enumerate(bc.RECUT_PLANS):
            vid = tc.variant_id(pkg, name)
            ctx.set_plan(vid, 0, 0)
            assert ctx.get_plan() == (vid, 0, 0)
            unit = tc.shape_of(name).tile_h
            nb = bc.host_bands(bc.wanted(env), ctx.dst_bytes, h, unit)
            if lab:
                assert ctx.host_bands == nb, (step, name, ctx.host_bands, nb)
            for again in range(2):
                bad = problems(convert_alone(ctx, buf), want)
                assert not bad, "step %d %s, %d bands of unit %d, frame %d: %s" % (step, name, nb, unit, again,
                                                                                  "\n".join(bad))
    report_count()


# -- D. unpadded rows: the 1-D download, and the default stride of 3-byte pixels and of planes ----------------------------

@pytest.mark.parametrize("name", bc.UNPADDED_FAMILIES)
def test_default_strides_once_per_download_shape(gpu_pkg, oracle, name):
    """height 52 (bands of 16, 16, 16 and 4 rows), the smallest width of 2 mod 4 whose frame reaches 16 MiB at the
    DEFAULT destination stride: 4- and 8-byte pixels download each band as one run of bytes, 3-byte pixels and planes
    end every row two bytes before the stride"""
    reset_count()
    pkg = gpu_pkg
    fam = bc.family(name)
    h = bc.UNPADDED_HEIGHT
    w = bc.unpadded_width(fam)
    case = bc.rotate(fam, bc.UNPADDED_FAMILIES.index(name), w, h)
    rng = np.random.default_rng([7, w, h])
    buf = random_frame(fam, case, rng, bc.src_row_bytes(fam, w))
    col = stage_of(pkg, fam)
    want = expect(pkg, oracle, fam, buf, case, col)
    with open_ctx(pkg, fam, case, col) as ctx:
        assert ctx.dst_stride == bc.default_dst_stride(fam, w) and w % 4 == 2
        assert ctx.dst_bytes >= bc.BAND_MIN_BYTES > bc.planes(fam) * bc.default_dst_stride(fam, w - 4) * h
        assert (ctx.dst_stride == bc.row_bytes(fam, w)) == (fam.kind in ("strip", "tile"))
        nb = bc.host_bands(bc.PRODUCT_WANT, ctx.dst_bytes, h, fam.unit)
        assert nb == 4
        got = convert_alone(ctx, buf)
    report_count()
    bad = problems(got, want)
    assert not bad, "%s: %s" % (where(fam, case, nb), "\n".join(bad))


# -- E. the once-per-frame launches behind the last band -------------------------------------------------------------------

def samples_of(fam, case, buf):
    sbe = case.sbe if fam.kind == "strip" else fam.arm.sbe
    return sm.samples(buf, case.w, case.h, buf.shape[1], fam.arm.bits, sbe)


@pytest.mark.parametrize("h", bc.ONCE_HEIGHTS)
@pytest.mark.parametrize("name", bc.ONCE_FAMILIES)
def test_statistics_and_histogram_once_per_banded_frame(gpu_pkg, oracle, name, h):
    """zone statistics and histogram both on, two frames of different content through the same slot: the counts are
    those of the whole mosaic of THAT frame -- not of a band, not of the bands added up, not of the frame before"""
    reset_count()
    pkg = gpu_pkg
    fam = bc.family(name)
    w = sc.SWEEP_WIDTHS[bc.ONCE_HEIGHTS.index(h)]
    case = bc.rotate(fam, 1 + bc.ONCE_FAMILIES.index(name), w, h)
    depth = sc.depth_of(fam.arm.bits)
    sstride, _ = bc.strides(fam, w, h)
    rng = np.random.default_rng([9, w, h])
    bufs = [random_frame(fam, case, rng, sstride) for _ in range(2)]
    # the second frame is darker: no count of the first can stand in for one of the second
    S1 = samples_of(fam, case, bufs[1]) >> 1
    bufs[1] = sc.frame_bytes(S1, fam.arm.bits, rng, sstride, case.sbe if fam.kind == "strip" else fam.arm.sbe)
    col = stage_of(pkg, fam)
    zx, zy = bc.stats_grid(h)
    lo, hi = (1 << depth) // 16, (1 << depth) - (1 << depth) // 16
    with open_banded(pkg, fam, case) as ctx:
        nb = bc.host_bands(bc.PRODUCT_WANT, ctx.dst_bytes, h, fam.unit)
        assert nb == 4
        win = bc.hist_window(nb, h, fam.unit, w)
        plain = [convert_alone(ctx, b).copy() for b in bufs]
        ctx.set_stats(zx, zy, lo, hi)
        ctx.set_hist(True, win)
        for f in (0, 1, 0):
            got = convert_alone(ctx, bufs[f])
            assert np.array_equal(got, plain[f]), (name, h, f, "the pixels changed with the statistics on")
            S = samples_of(fam, case, bufs[f])
            zones, want_zones = ctx.frame_stats(), sm.zone_stats(S, zx, zy, lo, hi)
            for field in ("sum", "count", "clipped"):
                assert np.array_equal(zones[field], want_zones[field]), (name, h, f, field, zones[field].reshape(-1, 4)[:6],
                                                                        want_zones[field].reshape(-1, 4)[:6])
            hist, want_hist = ctx.frame_hist(), hm.histogram(S, depth, win)
            assert hist.dtype == want_hist.dtype and np.array_equal(hist, want_hist), (
                name, h, f, int(hist.sum()), int(want_hist.sum()), np.argwhere(hist != want_hist)[:6])
            assert int(hist.sum()) == win[2] * win[3]
    for f in range(2):
        bad = problems(plain[f], expect(pkg, oracle, fam, bufs[f], case, col))
        assert not bad, "%s frame %d: %s" % (where(fam, case, nb), f, "\n".join(bad))
    report_count()


# -- F. one stage per frame ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", bc.STAGE_FAMILIES)
def test_a_banded_frame_is_of_one_stage(gpu_pkg, oracle, name):
    """set_colour (A), frame, set_colour (B), frame, and A again: every band of a frame runs under the stage that was
    set when the frame was accepted.  That half is deterministic, and cannot tell a stage taken per band from one taken
    per frame: the stage never changes while a frame is being queued.  The second half switches it from another thread
    meanwhile, as the 4K test of tests/test_gpu_colour.py does"""
    reset_count()
    pkg = gpu_pkg
    fam = bc.family(name)
    h = bc.STAGE_HEIGHT
    case = bc.rotate(fam, 5 + bc.STAGE_FAMILIES.index(name), sc.SWEEP_WIDTHS[bc.STAGE_FAMILIES.index(name)], h)
    buf, want_a = inputs(pkg, oracle, fam, case)
    stage_a = stage_of(pkg, fam)
    stage_b = pkg.Colour.make(black=0, gains=(1.0, 1.0, 2.4), curve=pkg.TONE_LINEAR)
    want_b = expect(pkg, oracle, fam, buf, case, stage_b)
    assert not np.array_equal(want_a, want_b)
    with open_banded(pkg, fam, case, col=stage_a) as ctx:
        nb = bc.host_bands(bc.PRODUCT_WANT, ctx.dst_bytes, h, fam.unit)
        assert nb == 4
        for step, (stage, want) in enumerate(((stage_a, want_a), (stage_b, want_b), (stage_a, want_a), (stage_b, want_b))):
            ctx.set_colour(stage)
            bad = problems(convert_alone(ctx, buf), want)
            assert not bad, "%s step %d: %s" % (where(fam, case, nb), step, "\n".join(bad))
        # ... and with the stage switched from another thread while the frames are queued: a host-side race for the
        # context's stage only (mibayer_set_colour copies under its lock and touches no queue).  On a correct library
        # the outcome is certain: each frame is wholly A or wholly B.  A stage read once per BAND is caught only when a
        # switch falls between two bands of a frame -- likely over 24 frames, not guaranteed (observed: at the first
        # raced frame, profiles/2026-10-20_band_seam_tests.md).  The small twin of
        # test_a_banded_frame_never_mixes_two_stages (tests/test_gpu_colour.py)
        stop = threading.Event()

        def switch():
            k = 0
            while not stop.is_set():
                k ^= 1
                ctx.set_colour((stage_a, stage_b)[k])
        t = threading.Thread(target=switch)
        t.start()
        mixed = []
        try:
            for i in range(RACED_FRAMES):
                out = convert_alone(ctx, buf)
                bad_a, bad_b = problems(out, want_a), problems(out, want_b)
                if bad_a and bad_b:
                    mixed.append("raced frame %d is of neither stage: against A %s; against B %s" % (i, bad_a, bad_b))
        finally:
            stop.set()
            t.join()
    assert not mixed, "%s: %s" % (where(fam, case, nb), "\n".join(mixed[:4]))
    report_count()
