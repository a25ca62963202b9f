"""GPU tests of the noise reduction (include/mibayer.h, group `nr`): mosaic_nr_kernel through mibayer_nr_device, byte for
byte against tests/nr_model.py.  The shapes are the table of tests/nr_cases.py (what each reaches:
tests/test_nr_cases.py); the host path is tests/test_gpu_nr_host.py."""
import numpy as np
import pytest

import nr_cases as nc
import nr_model as nm
import stats_model as sm
import strip_cases as sc

pytestmark = pytest.mark.gpu

SRC_FILL, DST_FILL, GUARD = 0x5A, 0xC3, 64


def run_device(ctx, frames, src_pitch=None, dst_pitch=None, offset=0):
    """frames: (n, src_bytes) bytes -> (n, src_bytes) bytes after ONE mibayer_nr_device call.  Both sides are surrounded
    by guards, sit `offset` bytes into their allocations and have a frame pitch of their own; the destination is
    poisoned first: everything outside the frames, between them included, must keep the poison, and the source must not
    change"""
    frames = np.ascontiguousarray(frames, np.uint8)
    n, nb = frames.shape
    assert nb == ctx.src_bytes
    sp, dp = src_pitch or nb, dst_pitch or nb
    stotal, dtotal = offset + n * sp + GUARD, offset + n * dp + GUARD
    src = np.full(stotal, SRC_FILL, np.uint8)
    for f in range(n):
        src[offset + f * sp:offset + f * sp + nb] = frames[f]
    before = np.full(dtotal, DST_FILL, np.uint8)
    d_src, d_dst = ctx.device_alloc(stotal), ctx.device_alloc(dtotal)
    try:
        ctx.to_device(d_src, src)
        ctx.to_device(d_dst, before)
        ctx.nr_device(d_src + offset, d_dst + offset, n, sp, dp)
        ctx.sync()
        out = ctx.from_device(d_dst, dtotal)
        assert np.array_equal(ctx.from_device(d_src, stotal), src), "the source changed"
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    keep = np.ones(dtotal, bool)
    for f in range(n):
        keep[offset + f * dp:offset + f * dp + nb] = False
    assert (out[keep] == DST_FILL).all(), "bytes outside the frames were written"
    return np.stack([out[offset + f * dp:offset + f * dp + nb] for f in range(n)])


def check(pkg, ctx, frames, curve, bits=0, sbe=False, where="", segment_of=None, **kw):
    """one call against the model: the frames' samples denoised, the stride padding still the destination's poison.
    `segment_of`: row -> (ya, yb) of the workgroups that walk it, for the message"""
    w, h, stride = ctx.width, ctx.height, ctx.src_stride
    ctx.set_nr(pkg.Nr(curve))
    assert ctx.get_nr() == [int(v) for v in curve]
    got = run_device(ctx, frames, **kw)
    poison = np.full(ctx.src_bytes, DST_FILL, np.uint8)
    for f in range(len(frames)):
        if f == 0 or not np.array_equal(frames[f], frames[f - 1]):      # (a batch of one frame repeated: one model run)
            want = nm.denoise_raw(frames[f], poison, w, h, stride, bits, sbe, curve)
        if not np.array_equal(got[f], want):
            bad = np.argwhere(got[f].reshape(h, stride) != want.reshape(h, stride))
            seg = " in the segment of rows %d .. %d" % segment_of(bad[0][0]) if segment_of else ""
            raise AssertionError("%s %dx%d frame %d: %d bytes differ, first at row %d byte %d%s (got %d, want %d)"
                                 % (where, w, h, f, len(bad), bad[0][0], bad[0][1], seg,
                                    got[f].reshape(h, stride)[tuple(bad[0])], want.reshape(h, stride)[tuple(bad[0])]))
    return got


def open_case(pkg, case, pad=0):
    stride = sc.src_row_bytes(case.w, case.bits) + pad
    return pkg.Context(case.w, case.h, sc.ORDERS[(case.w + case.h) % 4], "RGBx", src_stride=stride, bits=case.bits,
                       src_big_endian=case.sbe, device=0)


def as_bytes(rng, S, case, stride):
    return sc.frame_bytes(S, case.bits, rng, stride, case.sbe).reshape(-1)


# -- A. the kernel's geometry ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", nc.CASES, ids=nc.case_id)
def test_noisy_ramps_on_every_seam(gpu_pkg, case):
    """the frames of tests/nr_cases.py (half of the neighbours included, |d| = t and t + 1 both present, every seam column
    and row changed) and the planted boundaries at 0 and at max; rows carry 4 bytes of padding, which keep the
    destination's poison like the half dword behind a width of 2 mod 4; a batch has two frame pitches and base pointers at
    4 mod 16"""
    rng = np.random.default_rng([1, case.w, case.h, case.bits])
    curve = nc.curve_of(case)
    with open_case(gpu_pkg, case, pad=4) as ctx:
        kw = dict(bits=case.bits, sbe=case.sbe, where=nc.case_id(case))
        if case.nframes > 1:
            kw.update(src_pitch=ctx.src_bytes + 20, dst_pitch=ctx.src_bytes + 36, offset=4)
        frames = np.stack([as_bytes(rng, nc.seam_samples(case, f), case, ctx.src_stride) for f in range(case.nframes)])
        check(gpu_pkg, ctx, frames, curve, **kw)
        if case.w >= 10 and case.h >= 7:
            for at_max in (False, True):
                S, _ = nc.boundary_samples(case, at_max)
                check(gpu_pkg, ctx, np.stack([as_bytes(rng, S, case, ctx.src_stride)] * case.nframes), curve, **kw)


# every long case under its noisy ramps; the planted boundaries where a frame admits them; uniform random samples under
# a rising curve for one case per width of a sample (8-bit, 16-bit big-endian)
LONG_RUNS = [(c, "noise") for c in nc.LONG_CASES] \
    + [(c, at) for c in nc.LONG_CASES if c.w >= 10 and c.h >= 7 for at in ("at_0", "at_max")] \
    + [(c, "rising") for c in (nc.LONG_CASES[0], nc.LONG_CASES[3])]


@pytest.mark.parametrize("case,content", LONG_RUNS, ids=lambda v: v if isinstance(v, str) else nc.case_id(v))
def test_segments_longer_than_the_minimum(gpu_pkg, case, content):
    """long batches of narrow frames, whose workgroups walk 17 .. 64 rows (tests/test_nr_cases.py: which, and that the
    frames show a window that stops at its segment): ONE call for the whole batch and every frame compared.  The noisy
    ramps, every frame its own noise; the planted boundaries at 0 and at max in every frame; uniform random samples under
    a rising curve.  Frame pitches and base pointers as in the batches above"""
    rng = np.random.default_rng([4, case.w, case.h, case.bits])
    curve = nc.curve_of(case)
    with open_case(gpu_pkg, case, pad=4) as ctx:
        if content == "noise":
            frames = np.stack([as_bytes(rng, nc.seam_samples(case, f), case, ctx.src_stride) for f in range(case.nframes)])
        elif content == "rising":
            tm = nm.t_max(nc.depth(case))
            curve = [tm * i // 16 for i in range(17)]
            frames = np.stack([sc.random_frame(rng, case.w, case.h, case.bits, ctx.src_stride, case.sbe).reshape(-1)
                               for _ in range(case.nframes)])
        else:
            S, _ = nc.boundary_samples(case, content == "at_max")
            frames = np.stack([as_bytes(rng, S, case, ctx.src_stride)] * case.nframes)
        check(gpu_pkg, ctx, frames, curve, bits=case.bits, sbe=case.sbe, where=nc.case_id(case) + " " + content,
              segment_of=lambda row: nc.segment_of(case, row), src_pitch=ctx.src_bytes + 20,
              dst_pitch=ctx.src_bytes + 36, offset=4)


@pytest.mark.parametrize("bits,sbe", [(0, False)] + [(b, e) for b in (10, 12, 14, 16) for e in (False, True)],
                         ids=lambda v: {False: "le", True: "be"}.get(v, str(v)) if isinstance(v, bool) else "%d" % (v or 8))
def test_zero_curve_and_a_curve_that_differs_in_every_interval(gpu_pkg, bits, sbe):
    """uniform random samples (deep ones with junk above `bits`): every level, so every node interval of the curve, with a
    curve whose nodes all differ, rising and falling; the zero curve is the identity on the masked samples"""
    rng = np.random.default_rng([2, bits, sbe])
    depth = bits or 8
    w, h = (1030, 21) if bits == 0 else (518, 21)
    case = nc.Case(w, h, bits, sbe, 1)
    tm = nm.t_max(depth)
    ramp = [tm * i // 16 for i in range(17)]
    zigzag = [(tm if i % 2 else tm // 3) - i for i in range(17)]
    with open_case(gpu_pkg, case) as ctx:
        frame = sc.random_frame(rng, w, h, bits, ctx.src_stride, sbe).reshape(1, -1)
        S = sm.samples(frame[0], w, h, ctx.src_stride, bits, sbe)
        assert set((S >> (depth - 4)).reshape(-1).tolist()) == set(range(16))
        for curve in (ramp, ramp[::-1], zigzag):
            share = nm.included(S, curve, depth).mean()
            assert 0.02 < share < 0.98, share
            check(gpu_pkg, ctx, frame, curve, bits, sbe, where="random %d-bit" % depth)
        got = check(gpu_pkg, ctx, frame, [0] * 17, bits, sbe, where="zero curve")
        assert np.array_equal(sm.samples(got[0], w, h, ctx.src_stride, 16 if bits else 0, sbe), S)


@pytest.mark.parametrize("bits", [0, 12, 16])
def test_values_0_and_max(gpu_pkg, bits):
    """all 0, all max, 0 and max alternating per site, and 0 or max at random: under the largest curve P and N reach
    24 T_MAX where max - 0 <= T_MAX (8 and 10 .. 11 bits) and nothing is included where it is not"""
    rng = np.random.default_rng([3, bits])
    depth = bits or 8
    vmax = (1 << depth) - 1
    for w, h in ((6, 5), (10, 6), (262, 21)):
        case = nc.Case(w, h, bits, False, 1)
        y, x = np.mgrid[0:h, 0:w]
        sites = np.choose(2 * (y & 1) + (x & 1), (0, vmax, vmax, 0))
        with open_case(gpu_pkg, case) as ctx:
            for S in (np.zeros((h, w), np.int64), np.full((h, w), vmax), sites, rng.choice([0, vmax], (h, w)),
                      rng.choice([0, nm.t_max(depth)], (h, w))):
                frame = as_bytes(rng, S, case, ctx.src_stride).reshape(1, -1)
                for t in (nm.t_max(depth), 1):
                    check(gpu_pkg, ctx, frame, [t] * 17, bits, where="extremes")


# -- B. the rules of the header -----------------------------------------------------------------------------------------------

def test_errors_follow_the_header(gpu_pkg):
    pkg = gpu_pkg
    L = pkg.lib()
    with pkg.Context(64, 48, device=0) as ctx:
        d = ctx.device_alloc(6 * ctx.src_bytes)
        e = d + 3 * ctx.src_bytes
        try:
            n = ctx.src_bytes
            assert L.mibayer_nr_device(ctx._h, d, n, e, n, 1, None) == pkg.ERR_EMPTY
            assert ctx.get_nr() is None
            ctx.set_nr(pkg.Nr(range(17)))
            assert ctx.get_nr() == list(range(17))
            s = ctx.stream
            assert L.mibayer_nr_device(ctx._h, d, n, e, n, 0, s) == pkg.OK
            assert L.mibayer_nr_device(ctx._h, d, n, d, n, 1, s) == pkg.ERR_ARG          # out of place only
            assert L.mibayer_nr_device(ctx._h, d, n, e, n, -1, s) == pkg.ERR_ARG
            assert L.mibayer_nr_device(ctx._h, None, n, e, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_nr_device(ctx._h, d, n, None, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_nr_device(ctx._h, d + 2, n, e, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_nr_device(ctx._h, d, n, e + 1, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_nr_device(ctx._h, d, n - 4, e, n, 2, s) == pkg.ERR_GEOMETRY
            assert L.mibayer_nr_device(ctx._h, d, n, e, n + 2, 2, s) == pkg.ERR_GEOMETRY
            assert L.mibayer_nr_device(ctx._h, d, n + 4, e, n + 8, 2, s) == pkg.OK
            short = pkg.Nr(3)
            short.struct_size -= 4
            high = pkg.Nr(3)
            high.curve[16] = 256
            for bad in (short, high):
                assert L.mibayer_set_nr(ctx._h, bad) == pkg.ERR_ARG
            assert ctx.get_nr() == list(range(17))      # a refused set leaves the one from before
            ctx.set_nr(pkg.Nr(255))
            ctx.set_nr(None)
            assert ctx.get_nr() is None
            ctx.sync()
        finally:
            ctx.device_free(d)
    for bits, tm in ((10, 1023), (12, 2047), (16, 2047)):
        with pkg.Context(64, 48, bits=bits, device=0) as deep:
            assert L.mibayer_set_nr(deep._h, pkg.Nr(tm + 1)) == pkg.ERR_ARG
            deep.set_nr(pkg.Nr(tm))
    for w, h in ((4, 48), (64, 4), (64, 3)):
        with pkg.Context(w, h, device=0) as small:
            assert L.mibayer_set_nr(small._h, pkg.Nr(4)) == pkg.ERR_GEOMETRY
            assert L.mibayer_set_nr(small._h, pkg.Nr(256)) == pkg.ERR_ARG
            assert L.mibayer_set_nr(small._h, None) == pkg.OK
    with pkg.Context(64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER, device=0) as inv:
        assert L.mibayer_set_nr(inv._h, pkg.Nr(4)) == pkg.ERR_ARG
        assert L.mibayer_set_nr(inv._h, None) == pkg.ERR_ARG
