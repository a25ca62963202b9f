"""GPU tests of the 8-bit tile kernels (bayer2rgb_lds_kernel, fast and generic arm, and bayer2rgb_lds_aligned_kernel;
csrc/mibayer_kernels.hip) and of the launcher's choice among them (plan_launch, csrc/mibayer_abi.hip): every tile seam,
every position at which a row can end, the staging tail, the halo bound, the last tile row, every per-row shift of the
aligned arm and both sides of its edge-wave test, every block order, and the value extremes -- bit-exact against the
CPU oracle (the C restatement pinned to the reference's own frame driver).  The tables are tests/tile_cases.py;
tests/test_tile_cases.py shows without a GPU what they reach.

Where the tables' brief cannot be read literally (tests/test_tile_cases.py asserts what holds instead): the identity
order (band 0) has no idle block, a band of ONE tile row cannot hold rows of two frames (there one XCD walks rows of two
frames), and the last wave of a row never has wave_x + 256 below the width."""
import numpy as np
import pytest

import tile_cases as tc

pytestmark = pytest.mark.gpu

GUARD = 4096
FILL = 0x3C
SLACK = 128                     # behind the last guard: destination offsets of up to 120 bytes


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else "%d bytes differ, first at row %d byte %d (got %d, want %d)" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


# -- inputs and expected bytes: computed once, shared by every variant -----------------------------------------------

_random = {}
_wanted = {}


def random_frames(seed, w, h, n, sstride):
    key = (seed, w, h, n, sstride)
    if key not in _random:
        rng = np.random.default_rng([seed, w, h, n])
        src = rng.integers(0, 256, (n, h, sstride), dtype=np.uint8)
        src.setflags(write=False)
        _random[key] = src
    return _random[key]


def wanted(oracle, pkg, tag, src, case):
    """the oracle's rows (n, h, 4 w) for frames `src` (n, h, stride); tag names the frames"""
    key = (tag, case)
    if key not in _wanted:
        r, g, b = pkg.FORMATS[case.layout]
        out = np.stack([oracle.bayer2rgb(f, case.w, case.order, r, g, b) for f in src])
        out.setflags(write=False)
        _wanted[key] = out
    return _wanted[key]


# -- one launch, and everything around its pixels --------------------------------------------------------------------

def convert(ctx, src, src_off=0, dst_off=0, dst_gap=0, as_list=False):
    """one mibayer_process_device launch (as_list: one mibayer_process_device_list launch at the same addresses) over
    the frames src (n, h, src_stride).  The destination lies GUARD + dst_off bytes inside an allocation prefilled with
    FILL, its frames dst_bytes + dst_gap apart; the source src_off bytes inside its own.  Returns the destination's
    bytes from its first frame on, n * (dst_bytes + dst_gap) of them, what is wrong with the guards ("" = nothing) and
    the allocation's base address"""
    n = len(src)
    assert src[0].size == ctx.src_bytes
    fb = ctx.dst_bytes + dst_gap
    total = n * fb + 2 * GUARD + SLACK
    d_src = ctx.device_alloc(n * ctx.src_bytes + src_off + 16)
    d_dst = ctx.device_alloc(total)
    try:
        ctx.to_device(d_src + src_off, src)
        ctx.to_device(d_dst, np.full(total, FILL, np.uint8))
        if as_list:
            ctx.process_device_list([d_src + src_off + f * ctx.src_bytes for f in range(n)],
                                    [d_dst + GUARD + dst_off + f * fb for f in range(n)])
        else:
            ctx.process_device(d_src + src_off, d_dst + GUARD + dst_off, n, dst_frame_bytes=fb)
        ctx.sync()
        out = ctx.from_device(d_dst, total)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    lo = GUARD + dst_off
    wrong = "" if (out[:lo] == FILL).all() and (out[lo + n * fb:] == FILL).all() else "guard bytes written"
    return out[lo:lo + n * fb], wrong, d_dst


def problems(ctx, body, wrong, want, dst_gap=0):
    """what is wrong with a launch's output: guards, the gaps between pitched frames, the row padding, the pixels"""
    n, h, w4 = want.shape
    fb = ctx.dst_bytes + dst_gap
    bad = [wrong] if wrong else []
    frames = body.reshape(n, fb)
    if dst_gap and not (frames[:, ctx.dst_bytes:] == FILL).all():
        bad.append("gap between the frames written")
    rows = frames[:, :ctx.dst_bytes].reshape(n, h, ctx.dst_stride)
    if not (rows[:, :, w4:] == FILL).all():
        bad.append("row padding of the destination written")
    for f in range(n):
        if not np.array_equal(rows[f, :, :w4], want[f]):
            bad.append("frame %d: %s" % (f, first_difference(rows[f, :, :w4], want[f])))
            break
    return bad


def where(name, case, extra=""):
    shape = tc.shape_of(name)
    return "%s %dx%d %s %s (w %% 16 = %d, h %% %d = %d)%s" % (name, case.w, case.h, case.order, case.layout,
                                                              case.w % 16, shape.tile_h, case.h % shape.tile_h, extra)


def run_geometry(pkg, oracle, name, cases, seed, plan=None, dst_pad=24, offsets=(0, 0), padded=True):
    """random frames, padded strides on both sides (padded = False: the default strides), through process_device;
    collects every failing case so that one run names every width that is wrong.  plan: (band, align) for
    mibayer_set_plan, None: Context (variant = id).  Returns the failures"""
    vid = tc.variant_id(pkg, name)
    shape = tc.shape_of(name)
    bad = []
    for case in cases:
        sstride, dstride = (case.w + 3) & ~3, 4 * case.w
        if padded:
            sstride, dstride = tc.src_stride_of(case.w), 4 * case.w + dst_pad
        src = random_frames(seed, case.w, case.h, 1, sstride)
        want = wanted(oracle, pkg, ("random", seed, sstride), src, case)
        with pkg.Context(case.w, case.h, case.order, case.layout, src_stride=sstride, dst_stride=dstride,
                         variant=0 if plan else vid, device=0) as ctx:
            assert (ctx.src_stride, ctx.dst_stride) == (sstride, dstride)
            if plan:
                ctx.set_plan(vid, *plan)
                assert ctx.get_plan() == (vid,) + tuple(plan) and ctx.plan_source == pkg.PLAN_SET
            geo = ctx.launch_geometry(1)
            assert (geo["tile_w"], geo["tile_h"]) == (shape.tile_w, shape.tile_h), (name, geo)
            assert geo["tiles_x"] == -(-case.w // shape.tile_w) and geo["tile_rows"] == -(-case.h // shape.tile_h)
            body, wrong, _ = convert(ctx, src, *offsets)
            for p in problems(ctx, body, wrong, want):
                bad.append(where(name, case, "" if padded else " default strides") + ": " + p)
    return bad


# -- 1. every width --------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", tc.PRODUCTION_NAMES)
def test_every_width_at_height_35(gpu_pkg, oracle, name):
    cases = tc.width_cases(tc.PRODUCTION_NAMES.index(name))
    assert [c.w for c in cases] == list(tc.WIDTHS) and {c.h for c in cases} == {tc.SWEEP_HEIGHT}
    assert {tc.expected_arm(tc.sweep_launch(c)) for c in cases} == {"generic"}
    bad = run_geometry(gpu_pkg, oracle, name, cases, 1)
    # the widths of 0 mod 16 once more, unpadded: the fast arm (1040: a second tile of one 16-byte chunk)
    fast = tc.fast_width_cases(tc.PRODUCTION_NAMES.index(name))
    assert {tc.expected_arm(tc.sweep_launch(c, padded=False)) for c in fast} == {"fast"}
    bad += run_geometry(gpu_pkg, oracle, name, fast, 6, padded=False)
    assert not bad, "\n".join(bad)


# -- 2. every height -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("align", [0, 128], ids=["generic", "aligned128"])
@pytest.mark.parametrize("name", tc.NT_NAMES)
def test_every_height_at_widths_262_and_1028(gpu_pkg, oracle, name, align):
    cases = tc.height_cases(tc.NT_NAMES.index(name))
    assert sorted({c.w for c in cases}) == list(tc.HEIGHT_WIDTHS) and len(cases) == 2 * len(tc.HEIGHTS)
    assert {tc.expected_arm(tc.height_launch(c, align)) for c in cases} == {"aligned128" if align else "generic"}
    bad = run_geometry(gpu_pkg, oracle, name, cases, 2, plan=(0, align), dst_pad=8)
    assert not bad, "\n".join(bad)


# -- 3. the weakest base pointers ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", tc.NT_NAMES + tc.HY_NAMES)
def test_weakest_base_pointers(gpu_pkg, oracle, name):
    """source and destination at 4 mod 16: the generic arm of every shape, also at the widths of its fast path"""
    k = tc.PRODUCTION_NAMES.index(name)
    cases = [tc.rotate(3 * i + k, w, tc.SWEEP_HEIGHT) for i, w in enumerate(tc.weakest_widths(tc.shape_of(name)))]
    assert {tc.expected_arm(tc.sweep_launch(c, weakest=True)) for c in cases} == {"generic"}
    bad = run_geometry(gpu_pkg, oracle, name, cases, 3, offsets=(4, 4))
    assert not bad, "\n".join(bad)


# -- 4. the aligned arm ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", tc.ARM128_NAMES)
def test_aligned_arm_every_shift(gpu_pkg, oracle, name):
    pkg = gpu_pkg
    vid = tc.variant_id(pkg, name)
    k = tc.ARM128_NAMES.index(name)
    bad = []
    for i, row in enumerate(tc.ALIGNED_CASES):
        w, h, pad, off, n, gap = row
        case = tc.rotate(i + 3 * k, w, h)
        band = tc.ALIGNED_BANDS[(i + k) % 3]
        sstride, dstride = tc.src_stride_of(w), 4 * w + pad
        src = random_frames(4, w, h, n, sstride)
        want = wanted(oracle, pkg, ("random", 4, sstride, n), src, case)
        assert tc.expected_arm(tc.aligned_launch(row)) == "aligned128"
        with pkg.Context(w, h, case.order, case.layout, src_stride=sstride, dst_stride=dstride, device=0) as ctx:
            ctx.set_plan(vid, band, tc.ALIGN)
            assert ctx.get_plan() == (vid, band, tc.ALIGN)
            for as_list in ((False, True) if n > 1 else (False,)):
                body, wrong, base = convert(ctx, src, 0, off, gap, as_list)
                assert base % tc.ALIGN == 0, "tile_cases.row_shifts assumes allocations at 0 mod 128"
                for p in problems(ctx, body, wrong, want, gap):
                    bad.append(where(name, case, " pitch +%d offset %d frames %d gap %d band %d%s shifts %s" % (
                        pad, off, n, gap, band, " list" if as_list else "", sorted(tc.row_shifts(row)))) + ": " + p)
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("align", [64, 128])
def test_aligned_arm_over_a_list_of_8_byte_aligned_destinations(gpu_pkg, gpu_lab_pkg, oracle, align):
    """five separately allocated frames of 642x50 whose destinations are all 8-byte aligned but not all 16-byte
    aligned: neither the fast arm nor a grid to sit on, so the list launch takes the sector-aligned arm (64: the lab
    build's flavour).  Every destination has its own guard bytes on both sides"""
    pkg = gpu_lab_pkg if align == 64 else gpu_pkg
    name, (w, h), n = "lds_2x4_r4_dpp_nt", (642, 50), 5
    offs = (0, 8, 16, 24, 72)
    case = tc.rotate(align // 64, w, h)
    sstride = tc.src_stride_of(w)
    src = random_frames(7, w, h, n, sstride)
    want = wanted(oracle, pkg, ("random", 7, sstride, n), src, case)
    with pkg.Context(w, h, case.order, case.layout, src_stride=sstride, device=0) as ctx:
        assert ctx.dst_stride == 4 * w and ctx.dst_stride % 8 == 0
        ctx.set_plan(tc.variant_id(pkg, name), 1, align)
        assert ctx.get_plan() == (tc.variant_id(pkg, name), 1, align)
        total = ctx.dst_bytes + 2 * GUARD + SLACK
        srcs = [ctx.device_alloc(ctx.src_bytes) for _ in range(n)]
        dsts = [ctx.device_alloc(total) for _ in range(n)]
        try:
            assert all(d % 128 == 0 for d in dsts), "the offsets assume allocations at 0 mod 128"
            for d, s in zip(srcs, src):
                ctx.to_device(d, s)
            for d in dsts:
                ctx.to_device(d, np.full(total, FILL, np.uint8))
            ptrs = [d + GUARD + o for d, o in zip(dsts, offs)]
            assert all(p % 8 == 0 for p in ptrs) and any(p % 16 for p in ptrs)
            ctx.process_device_list(srcs, ptrs)
            ctx.sync()
            raw = [ctx.from_device(d, total) for d in dsts]
        finally:
            for d in srcs + dsts:
                ctx.device_free(d)
    bad = []
    for f, (r, o) in enumerate(zip(raw, offs)):
        lo = GUARD + o
        if not ((r[:lo] == FILL).all() and (r[lo + ctx.dst_bytes:] == FILL).all()):
            bad.append("frame %d: guard bytes written" % f)
        got = r[lo:lo + ctx.dst_bytes].reshape(h, 4 * w)
        if not np.array_equal(got, want[f]):
            bad.append("frame %d (destination at %d mod 128): %s" % (f, o, first_difference(got, want[f])))
    assert not bad, "\n".join(bad)


# -- 5. block orders -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("fast", [False, True], ids=["generic", "fast"])
def test_batches_under_every_block_order(gpu_pkg, oracle, fast):
    """PLAN_CASES through set_plan, one process_device over the batch: frames dst_bytes + 4 apart (the generic arm, the
    phase changes per frame), and unpitched at the next width of 0 mod 16 (the fast arm)"""
    pkg = gpu_pkg
    bad = []
    for i, (pw, h, n, name, band) in enumerate(tc.PLAN_CASES):
        w = tc.fast_width(pw) if fast else pw
        case = tc.rotate(i, w, h)
        vid = tc.variant_id(pkg, name)
        sstride, dstride, gap = (w, 4 * w, 0) if fast else (tc.src_stride_of(w), 4 * w + 24, 4)
        L = tc.make_launch(w, h, sstride, dstride, nframes=n, dst_gap=gap)
        assert tc.expected_arm(L) == ("fast" if fast else "generic")
        src = random_frames(5, w, h, n, sstride)
        want = wanted(oracle, pkg, ("random", 5, sstride, n), src, case)
        with pkg.Context(w, h, case.order, case.layout, src_stride=sstride, dst_stride=dstride, device=0) as ctx:
            ctx.set_plan(vid, band, 0)
            assert ctx.get_plan() == (vid, band, 0)
            tiles_x, tile_rows, eff, grid = tc.plan_geometry(w, h, n, name, band)
            geo = ctx.launch_geometry(n)
            assert (geo["tiles_x"], geo["tile_rows"], geo["band"]) == (tiles_x, tile_rows, eff)
            assert geo["grid_blocks"] == grid
            body, wrong, _ = convert(ctx, src, dst_gap=gap)
            for p in problems(ctx, body, wrong, want, gap):
                bad.append(where(name, case, " frames %d band %d" % (n, band)) + ": " + p)
    assert not bad, "\n".join(bad)


# -- 6. value extremes -----------------------------------------------------------------------------------------------

_extreme = {}


def extreme_frames(w, h, sstride):
    """the 16 plane frames and the 9 pattern frames of strip_cases at depth 8, as two batches of source bytes"""
    key = (w, h, sstride)
    if key not in _extreme:
        sets = []
        for frames in (tc.plane_frames(w, h, 8), tc.pattern_frames(w, h, 8)):
            buf = np.full((len(frames), h, sstride), 0x5A, np.uint8)
            for f, S in enumerate(frames):
                buf[f, :, :w] = S
            buf.setflags(write=False)
            sets.append(buf)
        assert (len(sets[0]), len(sets[1])) == (16, 9)
        _extreme[key] = sets
    return _extreme[key]


@pytest.mark.parametrize("name", tc.PRODUCTION_NAMES)
def test_value_extremes(gpu_pkg, oracle, name):
    """every Bayer site constant 0 or 255 in all 16 combinations, stripes, impulses and blocks: each set in one batch
    launch at a fast geometry, at a generic one and -- where the name has the arm -- under the 128-byte arm"""
    pkg = gpu_pkg
    vid = tc.variant_id(pkg, name)
    k = tc.PRODUCTION_NAMES.index(name)
    runs = [("fast", tc.EXTREME_FAST, 0, 0), ("generic", tc.EXTREME_GENERIC, 0, 0)]
    if name in tc.ARM128_NAMES:
        runs.append(("aligned128", tc.EXTREME_GENERIC, tc.EXTREME_ALIGNED_PAD, tc.ALIGN))
    bad = []
    for r, (arm, (w, h), pad, align) in enumerate(runs):
        case = tc.rotate(k + 4 * r, w, h)
        sstride, dstride = (w + 3) & ~3, 4 * w + pad
        for s, src in enumerate(extreme_frames(w, h, sstride)):
            assert tc.expected_arm(tc.make_launch(w, h, sstride, dstride, nframes=len(src), align=align)) == arm
            want = wanted(oracle, pkg, ("extremes", s), src, case)
            assert want.min() == 0 and want.max() == 255
            with pkg.Context(w, h, case.order, case.layout, dst_stride=dstride, device=0) as ctx:
                assert (ctx.src_stride, ctx.dst_stride) == (sstride, dstride)
                ctx.set_plan(vid, 0, align)
                assert ctx.get_plan() == (vid, 0, align)
                body, wrong, _ = convert(ctx, src)
                for p in problems(ctx, body, wrong, want):
                    bad.append(where(name, case, " %s, %s frames" % (arm, ("plane", "pattern")[s])) + ": " + p)
    assert not bad, "\n".join(bad)
