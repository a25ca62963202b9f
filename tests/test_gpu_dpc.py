"""GPU tests of the defective pixel correction (include/mibayer.h, group `dpc`): mosaic_dpc_kernel and
mosaic_dpc_list_kernel through mibayer_dpc_device, byte for byte against tests/dpc_model.py.  The shapes are the table of
tests/dpc_cases.py (what each reaches: tests/test_dpc_cases.py); the host path is tests/test_gpu_dpc_host.py."""
import numpy as np
import pytest

import dpc_cases as dc
import dpc_model as dm
import stats_model as sm
import strip_cases as sc

pytestmark = pytest.mark.gpu

SRC_FILL, DST_FILL, GUARD = 0x5A, 0xC3, 64


def run_device(ctx, frames, src_pitch=None, dst_pitch=None, offset=0):
    """frames: (n, src_bytes) bytes -> (n, src_bytes) bytes after ONE mibayer_dpc_device call, and the bytes the
    destination held before.  Both sides are surrounded by guards, sit `offset` bytes into their allocations and have a
    frame pitch of their own; the destination is poisoned first: everything outside the frames, between them included,
    must keep the poison, and the source must not change"""
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
        ctx.dpc_device(d_src + offset, d_dst + offset, n, sp, dp)
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


def check(pkg, ctx, frames, hot, cold, defects=None, bits=0, sbe=False, where="", segment_of=None, **kw):
    """one call against the model; returns the share of samples the detection flags in frame 0.  `segment_of`: row ->
    (ya, yb) of the workgroups that walk it, for the message"""
    w, h, stride = ctx.width, ctx.height, ctx.src_stride
    ctx.set_dpc(pkg.Dpc(hot, cold, defects))
    got = run_device(ctx, frames, **kw)
    poison = np.full(ctx.src_bytes, DST_FILL, np.uint8)
    for f in range(len(frames)):
        want = dm.correct_raw(frames[f], poison, w, h, stride, bits, sbe, hot, cold, defects)
        if not np.array_equal(got[f], want):
            bad = np.argwhere(got[f].reshape(h, stride) != want.reshape(h, stride))
            seg = " in the segment of rows %d .. %d" % segment_of(bad[0][0]) if segment_of else ""
            raise AssertionError("%s %dx%d hot %d cold %d frame %d: %d bytes differ, first at row %d byte %d%s (got %d, want %d)"
                                 % (where, w, h, hot, cold, f, len(bad), bad[0][0], bad[0][1], seg,
                                    got[f].reshape(h, stride)[tuple(bad[0])], want.reshape(h, stride)[tuple(bad[0])]))
    return float(dm.flagged(sm.samples(frames[0], w, h, stride, bits, sbe), hot, cold).mean())


def open_case(pkg, case, pad=0):
    stride = sc.src_row_bytes(case.w, case.bits) + pad
    return pkg.Context(case.w, case.h, sc.ORDERS[(case.w + case.h) % 4], "RGBx", src_stride=stride, bits=case.bits,
                       src_big_endian=case.sbe, device=0)


def seam_frames(rng, case, stride, phase=None):
    """the frames of dpc_cases.seam_samples as bytes"""
    return np.stack([sc.frame_bytes(dc.seam_samples(case, f, phase), case.bits, rng, stride, case.sbe).reshape(-1)
                     for f in range(case.nframes)])


# -- A. the kernel's geometry ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", dc.CASES, ids=dc.case_id)
def test_defects_on_every_seam(gpu_pkg, case):
    """detected by threshold, phase by phase (tests/test_dpc_cases.py: the detection must find every one), then all of
    them named in the list with the detection off, then both; rows carry 4 bytes of padding, which keep the
    destination's poison like the half dword behind a width of 2 mod 4"""
    rng = np.random.default_rng([1, case.w, case.h, case.bits])
    vmax = (1 << (case.bits or 8)) - 1
    with open_case(gpu_pkg, case, pad=4) as ctx:
        frames, where = seam_frames(rng, case, ctx.src_stride), dc.planted(case.w, case.h, case.bits, case.nframes)
        kw = dict(bits=case.bits, sbe=case.sbe, where=dc.case_id(case))
        if case.nframes > 1:
            kw.update(src_pitch=ctx.src_bytes + 20, dst_pitch=ctx.src_bytes + 36, offset=4)
        for phase in range(4):
            share = check(gpu_pkg, ctx, seam_frames(rng, case, ctx.src_stride, phase), vmax // 8, vmax // 8, None, **kw)
            assert share > 0
        check(gpu_pkg, ctx, frames, -1, -1, where, **kw)
        check(gpu_pkg, ctx, frames, vmax // 8, vmax // 8, where[::3], **kw)


@pytest.mark.parametrize("planted", ["phase0", "phase1", "phase2", "phase3", "listed"])
@pytest.mark.parametrize("case", dc.LONG_CASES, ids=dc.case_id)
def test_segments_longer_than_the_minimum(gpu_pkg, case, planted):
    """long batches of narrow frames, whose workgroups walk 17 .. 64 rows (tests/test_dpc_cases.py: which, and that the
    frames show a window that stops at its segment): ONE call for the whole batch, every frame compared.  Detected by
    threshold, one phase of the planted samples per test, so every one of them at the new seams must be found; and all
    of them at once with a list of 257 .. 511 entries that holds every planted position: two workgroups of the list kernel
    per frame, the second partial, up to the last frame.  Frame pitches and base pointers as in the batch test below"""
    rng = np.random.default_rng([7, case.w, case.h, case.bits])
    vmax = (1 << (case.bits or 8)) - 1
    with open_case(gpu_pkg, case, pad=4) as ctx:
        kw = dict(bits=case.bits, sbe=case.sbe, where=dc.case_id(case), segment_of=lambda row: dc.segment_of(case, row),
                  src_pitch=ctx.src_bytes + 20, dst_pitch=ctx.src_bytes + 52, offset=4)
        if planted == "listed":
            lst = dc.long_list(case, rng)
            assert 256 < len(dm.sort_defects(lst)) < 512
            check(gpu_pkg, ctx, seam_frames(rng, case, ctx.src_stride), vmax // 8, vmax // 8, lst, **kw)
        else:
            frames = seam_frames(rng, case, ctx.src_stride, int(planted[-1]))
            assert check(gpu_pkg, ctx, frames, vmax // 8, vmax // 8, None, **kw) > 0


@pytest.mark.parametrize("bits,sbe", [(0, False)] + [(b, e) for b in (10, 12, 14, 16) for e in (False, True)],
                         ids=lambda v: {False: "le", True: "be"}.get(v, str(v)) if isinstance(v, bool) else "%d" % (v or 8))
def test_random_frames_every_threshold_and_arm(gpu_pkg, bits, sbe):
    """uniform random samples (deep ones with junk above `bits`) at thresholds 0, a middle value and max, each arm alone
    and both.  At 0 and at the middle value both arms of every branch are taken: the model flags between 1 % and 99 % of
    the samples (the definition's prototype: 23 % at 0, 5.7 % at 40 of 255); at max no sample can be flagged, since
    S <= max <= hi + max, and the pass is the identity on the masked samples"""
    rng = np.random.default_rng([2, bits, sbe])
    vmax = (1 << (bits or 8)) - 1
    w, h = (1030, 37) if bits == 0 else (518, 37)
    case = dc.Case(w, h, bits, sbe, 1)
    with open_case(gpu_pkg, case) as ctx:
        frame = sc.random_frame(rng, w, h, bits, ctx.src_stride, sbe).reshape(1, -1)
        for t in (0, vmax * 40 // 255, vmax):
            for hot, cold in ((t, -1), (-1, t), (t, t)):
                share = check(gpu_pkg, ctx, frame, hot, cold, None, bits, sbe, where="random %d-bit" % (bits or 8))
                assert (share == 0.0) if t == vmax else (0.01 < share < 0.99), (bits, hot, cold, share)
        # both off and no list: the identity on the masked samples
        ctx.set_dpc(gpu_pkg.Dpc(-1, -1, None))
        got = run_device(ctx, frame)
        S = sm.samples(frame[0], w, h, ctx.src_stride, bits, sbe)
        assert np.array_equal(sm.samples(got[0], w, h, ctx.src_stride, 16 if bits else 0, sbe), S)


@pytest.mark.parametrize("bits", [0, 12, 16])
def test_values_0_and_max(gpu_pkg, bits):
    """every sample 0 or max, thresholds 0, max - 1 and max: hi + hot and S + cold reach 2 max"""
    rng = np.random.default_rng([3, bits])
    vmax = (1 << (bits or 8)) - 1
    for w, h in ((4, 4), (6, 5), (262, 21)):
        with open_case(gpu_pkg, dc.Case(w, h, bits, False, 1)) as ctx:
            frame = sc.frame_bytes(rng.choice([0, vmax], (h, w)), bits, rng, ctx.src_stride).reshape(1, -1)
            for t in (0, vmax - 1, vmax):
                check(gpu_pkg, ctx, frame, t, t, None, bits, where="extremes")


# -- B. batches ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 12])
def test_batch_of_three_with_two_frame_pitches(gpu_pkg, bits):
    """3 frames, the source's 20 and the destination's 52 bytes further apart than a frame is long, rows with 12 bytes
    of padding, the base pointers at 4 mod 16: nothing bleeds across a frame seam (each frame's first and last rows are
    random, and so are its neighbours'), and the poison between and around the frames stays"""
    rng = np.random.default_rng([4, bits])
    w, h = (1030, 37) if bits == 0 else (518, 21)
    vmax = (1 << (bits or 8)) - 1
    with open_case(gpu_pkg, dc.Case(w, h, bits, False, 3), pad=12) as ctx:
        frames = np.stack([sc.random_frame(rng, w, h, bits, ctx.src_stride).reshape(-1) for _ in range(3)])
        lst = np.stack([rng.integers(0, w, 200), rng.integers(0, h, 200)], 1)
        check(gpu_pkg, ctx, frames, vmax // 5, vmax // 7, lst, bits, where="batch", src_pitch=ctx.src_bytes + 20,
              dst_pitch=ctx.src_bytes + 52, offset=4)


# -- C. the list ----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bits", [0, 14])
def test_lists_of_0_1_and_hundreds(gpu_pkg, bits):
    """unsorted input with duplicates, entries on all four borders and corners, entries the detection flags too; what
    mibayer_get_dpc returns is the sorted copy without the duplicates"""
    pkg = gpu_pkg
    rng = np.random.default_rng([5, bits])
    w, h = (1030, 37) if bits == 0 else (518, 37)
    vmax = (1 << (bits or 8)) - 1
    with open_case(pkg, dc.Case(w, h, bits, False, 1)) as ctx:
        frame = sc.random_frame(rng, w, h, bits, ctx.src_stride).reshape(1, -1)
        S = sm.samples(frame[0], w, h, ctx.src_stride, bits)
        flagged = np.argwhere(dm.flagged(S, vmax // 6, vmax // 6))[:, ::-1]
        assert len(flagged) > 50
        border = [(0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1), (1, 1), (w - 2, h - 2), (w // 2, 0), (w // 2, h - 1),
                  (0, h // 2), (w - 1, h // 2), (1, h // 2), (w - 2, 1)]
        many = np.concatenate([np.stack([rng.integers(0, w, 400), rng.integers(0, h, 400)], 1), border, flagged[:50],
                               border[:5]])
        many = many[rng.permutation(len(many))]
        for lst in (np.zeros((0, 2), np.uint32), np.array([[w - 1, h - 1]]), many):
            for hot, cold in ((-1, -1), (vmax // 6, vmax // 6)):
                check(pkg, ctx, frame, hot, cold, lst, bits, where="list of %d" % len(lst))
                got_hot, got_cold, got = ctx.get_dpc()
                assert (got_hot, got_cold) == (hot, cold) and np.array_equal(got, dm.sort_defects(lst))
        assert len(dm.sort_defects(many)) < len(many)


def test_the_largest_list(gpu_pkg):
    """MIBAYER_DPC_MAX_DEFECTS entries: every sample of a 256 x 256 frame is listed"""
    pkg = gpu_pkg
    rng = np.random.default_rng(6)
    w = h = 256
    with open_case(pkg, dc.Case(w, h, 0, False, 1)) as ctx:
        frame = sc.random_frame(rng, w, h, 0, ctx.src_stride).reshape(1, -1)
        y, x = np.mgrid[0:h, 0:w]
        lst = np.stack([x.reshape(-1), y.reshape(-1)], 1)[rng.permutation(w * h)]
        assert len(lst) == pkg.DPC_MAX_DEFECTS == dm.MAX_DEFECTS
        check(pkg, ctx, frame, -1, -1, lst, where="full list")
        assert pkg.lib().mibayer_set_dpc(ctx._h, pkg.Dpc(-1, -1, np.concatenate([lst, lst[:1]]))) == pkg.ERR_ARG


# -- D. the rules of the header -----------------------------------------------------------------------------------------------

def test_errors_follow_the_header(gpu_pkg):
    pkg = gpu_pkg
    L = pkg.lib()
    with pkg.Context(64, 48, device=0) as ctx:
        d = ctx.device_alloc(6 * ctx.src_bytes)
        e = d + 3 * ctx.src_bytes
        try:
            n = ctx.src_bytes
            assert L.mibayer_dpc_device(ctx._h, d, n, e, n, 1, None) == pkg.ERR_EMPTY
            assert ctx.get_dpc() is None
            ctx.set_dpc(pkg.Dpc(3, -1, [(5, 7), (1, 2), (5, 7)]))
            hot, cold, lst = ctx.get_dpc()
            assert (hot, cold) == (3, -1) and lst.tolist() == [[1, 2], [5, 7]]
            s = ctx.stream
            assert L.mibayer_dpc_device(ctx._h, d, n, e, n, 0, s) == pkg.OK
            assert L.mibayer_dpc_device(ctx._h, d, n, d, n, 1, s) == pkg.ERR_ARG          # out of place only
            assert L.mibayer_dpc_device(ctx._h, d, n, e, n, -1, s) == pkg.ERR_ARG
            assert L.mibayer_dpc_device(ctx._h, None, n, e, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_dpc_device(ctx._h, d, n, None, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_dpc_device(ctx._h, d + 2, n, e, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_dpc_device(ctx._h, d, n, e + 1, n, 1, s) == pkg.ERR_ARG
            assert L.mibayer_dpc_device(ctx._h, d, n - 4, e, n, 2, s) == pkg.ERR_GEOMETRY
            assert L.mibayer_dpc_device(ctx._h, d, n, e, n + 2, 2, s) == pkg.ERR_GEOMETRY
            assert L.mibayer_dpc_device(ctx._h, d, n + 4, e, n + 8, 2, s) == pkg.OK
            # the rules of mibayer_set_dpc
            short = pkg.Dpc(3, 3)
            short.struct_size -= 4
            null_list = pkg.Dpc(3, 3)
            null_list.ndefects = 1
            for bad in (pkg.Dpc(256, 0), pkg.Dpc(0, 256), pkg.Dpc(-2, 0), pkg.Dpc(0, -2), pkg.Dpc(0, 0, [(64, 0)]),
                        pkg.Dpc(0, 0, [(0, 48)]), pkg.Dpc(0, 0, [(1, 1), (0xffffffff, 1)]), short, null_list):
                assert L.mibayer_set_dpc(ctx._h, bad) == pkg.ERR_ARG
            assert ctx.get_dpc()[0] == 3                # a refused set leaves the one from before
            ctx.set_dpc(pkg.Dpc(255, 255, [(63, 47)]))
            ctx.set_dpc(None)
            assert ctx.get_dpc() is None
            ctx.sync()
        finally:
            ctx.device_free(d)
    with pkg.Context(64, 48, bits=10, device=0) as deep:
        assert L.mibayer_set_dpc(deep._h, pkg.Dpc(1024, 0)) == pkg.ERR_ARG
        deep.set_dpc(pkg.Dpc(1023, 1023))
    with pkg.Context(64, 3, device=0) as flat:
        assert L.mibayer_set_dpc(flat._h, pkg.Dpc(4, 4)) == pkg.ERR_GEOMETRY
        assert L.mibayer_set_dpc(flat._h, pkg.Dpc(256, 4)) == pkg.ERR_ARG
        assert L.mibayer_set_dpc(flat._h, None) == pkg.OK
    with pkg.Context(64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER, device=0) as inv:
        assert L.mibayer_set_dpc(inv._h, pkg.Dpc(4, 4)) == pkg.ERR_ARG
        assert L.mibayer_set_dpc(inv._h, None) == pkg.ERR_ARG
