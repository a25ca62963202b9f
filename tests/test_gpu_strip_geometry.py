"""GPU tests of the strip kernels' shared code (store_strip8 / store_strip16, emit_cgd, reflect_row, launch_strip;
csrc/mibayer_kernels.hip): every position at which a row can end, the seam between two strips, the chunk edges, the
value extremes and the colour stage at the ends of its ranges -- bit-exact against the NumPy models
(tests/highbit_model.py, mhc_model.py, colour_model.py).  The tables are tests/strip_cases.py; tests/test_strip_cases.py
shows without a GPU what they reach.

Two things differ from a literal reading of the tables' brief, both on the asking-more side: width 272 is in the list
(the full last group in lane 3 behind the seam, which 254 .. 270 leave out), and the pattern batch has a ninth frame
(3x3 blocks: the only one that takes F_G and F_diag above the range).  A black level of vmax + 1 is run at depth 8 only:
at depth 16 it is 65536, which mibayer_set_colour refuses -- that refusal is asserted instead."""
import ctypes

import numpy as np
import pytest

import strip_cases as sc

pytestmark = pytest.mark.gpu

GUARD = 4096
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)      # rows sum to 1 (tests/test_gpu_colour.py)
OPENED = [0]                    # contexts opened by the running test (reported with -s / -rA)


def arm_id(arm):
    return arm.name


def srgb_stage(pkg, arm):
    """a stage that exercises every step, as make_colour of tests/test_gpu_colour.py: black level at 1/16 of the range,
    gains, a CCM with negative entries, the sRGB curve; None for a plain arm"""
    if not arm.colour:
        return None
    return pkg.Colour.make(black=(1 << sc.depth_of(arm.bits)) // 16, gains=(1.9, 1.0, 1.6), ccm=CCM, curve=pkg.TONE_SRGB)


def model_kw(col):
    return {} if col is None else dict(black=tuple(col.black[:]), matrix=tuple(col.matrix[:]), tone=col.tone_table())


def open_ctx(pkg, arm, case, col=None, src_stride=0, dst_stride=0):
    OPENED[0] += 1
    return pkg.Context(case.w, case.h, case.order, case.layout, src_stride=src_stride, dst_stride=dst_stride,
                       bits=arm.bits, src_big_endian=case.sbe, out16=arm.out16, dst_big_endian=case.dbe,
                       method=arm.method, colour=(col if col is not None else True) if arm.colour else None, device=0)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else "%d bytes differ, first at row %d byte %d (got %d, want %d)" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def convert_on_device(ctx, bufs, src_off=0, dst_off=0):
    """one mibayer_process_device launch over len(bufs) frames; the destination lies GUARD bytes inside its allocation
    on both sides, the base pointers src_off / dst_off bytes off the allocations' alignment.  Returns the frames' rows
    (n, h, dst_stride) and what is wrong with the bytes around them ("" = nothing)"""
    n = len(bufs)
    src = np.stack([np.ascontiguousarray(b).reshape(-1) for b in bufs])
    assert src.shape[1] == ctx.src_bytes
    total = n * ctx.dst_bytes + 2 * GUARD + dst_off
    d_src = ctx.device_alloc(src.size + src_off + 16)
    d_dst = ctx.device_alloc(total)
    try:
        ctx.to_device(d_src + src_off, src)
        ctx.to_device(d_dst, np.full(total, 0x3C, np.uint8))
        ctx.process_device(d_src + src_off, d_dst + GUARD + dst_off, n)
        ctx.sync()
        out = ctx.from_device(d_dst, total)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    lo = GUARD + dst_off
    wrong = "" if (out[:lo] == 0x3C).all() and (out[lo + n * ctx.dst_bytes:] == 0x3C).all() else "guard bytes written"
    return out[lo:lo + n * ctx.dst_bytes].reshape(n, ctx.height, ctx.dst_stride), wrong


def run_geometry(pkg, arm, cases, seed, weakest_alignment=False, dst_off=None):
    """random frames with junk above the depth, padded strides on both sides, through process_device; collects every
    failing case so that one run names every residue that is wrong"""
    rng = np.random.default_rng(seed)
    col = srgb_stage(pkg, arm)
    px = 8 if arm.out16 else 4
    bad = []
    for case in cases:
        sstride = sc.src_row_bytes(case.w, arm.bits) + 12          # rows dword-aligned, not 8-byte-aligned
        dstride = px * case.w + 24
        buf = sc.random_frame(rng, case.w, case.h, arm.bits, sstride, case.sbe)
        want = sc.expect(arm, buf, case, **model_kw(col))
        # the weakest base pointers the stride rules of include/mibayer.h allow: source = 4 mod 8, destination = 4 mod 16
        # (4-byte pixels) or 8 mod 16 (8-byte pixels)
        offsets = (4, dst_off or px) if weakest_alignment else (0, 0)
        with open_ctx(pkg, arm, case, col, sstride, dstride) as ctx:
            assert (ctx.src_stride, ctx.dst_stride) == (sstride, dstride)
            out, wrong = convert_on_device(ctx, [buf], *offsets)
        frame = out[0]
        where = (arm.name, case.w, case.h, case.order, case.layout)
        if wrong:
            bad.append((where, wrong))
        if not (frame[:, px * case.w:] == 0x3C).all():
            bad.append((where, "row padding of the destination written"))
        if not np.array_equal(frame[:, :px * case.w], want):
            bad.append((where, "w %% 16 = %d, h %% 16 = %d, sbe %d dbe %d: %s" % (
                case.w % 16, case.h % 16, case.sbe, case.dbe, first_difference(frame[:, :px * case.w], want))))
    return bad


# -- A. geometry -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", sc.ARMS, ids=arm_id)
def test_every_width_at_height_18(gpu_pkg, arm):
    OPENED[0] = 0
    cases = [c for c in sc.geometry_cases(arm)][:len(sc.WIDTHS)]
    assert [c.w for c in cases] == list(sc.WIDTHS) and {c.h for c in cases} == {sc.SWEEP_HEIGHT}
    bad = run_geometry(gpu_pkg, arm, cases, 1)
    print("contexts opened: %d" % OPENED[0])
    assert not bad, bad


@pytest.mark.parametrize("arm", sc.ARMS, ids=arm_id)
def test_every_height_at_widths_266_and_268(gpu_pkg, arm):
    OPENED[0] = 0
    cases = [c for c in sc.geometry_cases(arm)][len(sc.WIDTHS):]
    assert sorted({c.w for c in cases}) == list(sc.SWEEP_WIDTHS) and len(cases) == 2 * len(sc.HEIGHTS)
    bad = run_geometry(gpu_pkg, arm, cases, 2)
    print("contexts opened: %d" % OPENED[0])
    assert not bad, bad


@pytest.mark.parametrize("arm", sc.ARMS, ids=arm_id)
def test_weakest_base_pointer_alignment(gpu_pkg, arm):
    OPENED[0] = 0
    bad = run_geometry(gpu_pkg, arm, sc.alignment_cases(arm), 3, weakest_alignment=True)
    if arm.out16:
        # what the entry points accept is weaker still: an 8-byte-pixel destination at 4 mod 8
        bad += run_geometry(gpu_pkg, arm, sc.alignment_cases(arm)[-2:], 5, weakest_alignment=True, dst_off=4)
    print("contexts opened: %d" % OPENED[0])
    assert not bad, bad


@pytest.mark.parametrize("arm", sc.ARMS, ids=arm_id)
def test_host_path_once_per_arm(gpu_pkg, arm):
    OPENED[0] = 0
    rng = np.random.default_rng(4)
    col = srgb_stage(gpu_pkg, arm)
    px = 8 if arm.out16 else 4
    case = sc.rotate(arm, 2 + sc.ARMS.index(arm), sc.SWEEP_WIDTHS[sc.ARMS.index(arm) % 2], sc.SWEEP_HEIGHT)
    sstride, dstride = sc.src_row_bytes(case.w, arm.bits) + 12, px * case.w + 24
    buf = sc.random_frame(rng, case.w, case.h, arm.bits, sstride, case.sbe)
    want = sc.expect(arm, buf, case, **model_kw(col))
    with open_ctx(gpu_pkg, arm, case, col, sstride, dstride) as ctx:
        got = ctx.process_host(buf)
    where = (arm.name, case.w, case.h, case.order, case.layout)
    print("contexts opened: %d" % OPENED[0])
    assert np.array_equal(got[:, :px * case.w], want), (where, first_difference(got[:, :px * case.w], want))
    assert (got[:, px * case.w:] == 0xA5).all(), (where, "row padding of the destination written")


# -- B. value extremes -------------------------------------------------------------------------------------------------

EXTREMES = sc.extreme_cases()


@pytest.mark.parametrize("arm", EXTREMES, ids=arm_id)
def test_value_extremes(gpu_pkg, arm):
    """16 plane frames (every Bayer site constant 0 or max) in one batch launch, the pattern frames in a second, then
    the 16 plane frames once more as a list launch of exactly kMaxList frames"""
    OPENED[0] = 0
    pkg = gpu_pkg
    i = EXTREMES.index(arm)
    rng = np.random.default_rng(50 + i)
    depth = sc.depth_of(arm.bits)
    col = pkg.Colour(tone=sc.LINEAR_TONE) if arm.colour else None      # identity matrix, zero black level
    px = 8 if arm.out16 else 4
    for batch, ((w, h), frames) in enumerate(((sc.PLANE_SIZE, sc.plane_frames(*sc.PLANE_SIZE, depth)),
                                              (sc.PATTERN_SIZE, sc.pattern_frames(*sc.PATTERN_SIZE, depth)))):
        case = sc.rotate(arm, i + 7 * batch, w, h)
        where = (arm.name, w, h, case.order, case.layout)
        bufs = [sc.frame_bytes(S, arm.bits, rng, big_endian=case.sbe) for S in frames]
        wants = [sc.expect(arm, b, case, **model_kw(col)) for b in bufs]
        with open_ctx(pkg, arm, case, col) as ctx:
            assert ctx.dst_stride == px * w
            out, wrong = convert_on_device(ctx, bufs)
            assert not wrong, (where, wrong)
            for f, want in enumerate(wants):
                assert np.array_equal(out[f], want), (where, "batch frame %d" % f, first_difference(out[f], want))
            if batch:
                continue
            assert len(bufs) == sc.MAX_LIST
            srcs = [ctx.device_alloc(ctx.src_bytes) for _ in bufs]
            dsts = [ctx.device_alloc(ctx.dst_bytes) for _ in bufs]
            try:
                for d, b in zip(srcs, bufs):
                    ctx.to_device(d, b)
                ctx.process_device_list(srcs, dsts)
                ctx.sync()
                got = [ctx.from_device(d, ctx.dst_bytes).reshape(h, -1) for d in dsts]
            finally:
                for d in srcs + dsts:
                    ctx.device_free(d)
            for f, want in enumerate(wants):
                assert np.array_equal(got[f], want), (where, "list frame %d" % f, first_difference(got[f], want))
    print("contexts opened: %d" % OPENED[0])


# -- C. the colour stage at the ends of its ranges ---------------------------------------------------------------------

_stage_inputs = {}


def stage_inputs(method, bits):
    """the two frames of section C and their plain little-endian ARGB64 rows (the colour model's input), once per
    (method, depth)"""
    key = (method, bits)
    if key not in _stage_inputs:
        import colour_model as cm
        rng = np.random.default_rng(1000 + bits)
        w, h = sc.STAGE_SIZE
        bufs = [sc.frame_bytes(S, bits, rng) for S in sc.stage_frames(rng, bits)]
        plain = [cm.plain_argb64(b, w, h, "gbrg", bits, method, stride=b.shape[1])[0] for b in bufs]
        _stage_inputs[key] = (bufs, plain)
    return _stage_inputs[key]


def build_stage(pkg, stage):
    col = pkg.Colour(black=stage.black, matrix=stage.matrix, tone=stage.tone)
    if stage.junk is not None:
        col.tone[:] = list(stage.junk)
        assert col.has_tone == 0
    return col


@pytest.mark.parametrize("bits,out16,layout", sc.STAGE_IO, ids=["8_to_BGRx", "16_to_ARGB64"])
@pytest.mark.parametrize("method", ["bilinear", "mhc"])
def test_colour_stage_at_the_ends_of_its_ranges(gpu_pkg, method, bits, out16, layout):
    import colour_model as cm
    OPENED[0] = 0
    pkg = gpu_pkg
    depth = sc.depth_of(bits)
    w, h = sc.STAGE_SIZE
    arm = sc.Arm("colour_%s_%d_to_%s" % (method, depth, layout), method, bits, out16, True)
    case = sc.Case(w, h, "gbrg", layout, False, False)
    bufs, plain = stage_inputs(method, bits)
    frame_names = ("random", "constant max")
    with open_ctx(pkg, arm, case) as ctx:
        for stage in sc.colour_stages(depth):
            ctx.set_colour(build_stage(pkg, stage))
            out, wrong = convert_on_device(ctx, bufs)
            where = (arm.name, w, h, case.order, layout, stage.name)
            assert not wrong, (where, wrong)
            for f in range(2):
                want = cm.colour(plain[f], depth, layout, out16, black=stage.black, matrix=stage.matrix, tone=stage.tone)
                assert np.array_equal(out[f], want), (where, frame_names[f], first_difference(out[f], want))
        if depth == 16:
            # a black level of vmax + 1 = 65536 is outside mibayer_colour's range: refused, and the stage stays
            before = bytes(ctx.get_colour())
            over = pkg.Colour(black=(65535, 65535, 65535))
            over.black[1] = 65536
            assert pkg.lib().mibayer_set_colour(ctx._h, ctypes.byref(over)) == pkg.ERR_ARG
            assert bytes(ctx.get_colour()) == before
    print("contexts opened: %d" % OPENED[0])
