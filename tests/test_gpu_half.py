"""GPU tests of the half-size demosaic (include/mibayer.h, MIBAYER_FLAG_HALF): bayer2rgb_half_kernel
(csrc/mibayer_kernels.hip) on the device path, bit-exact against tests/half_model.py.  The shapes are the table of
tests/half_cases.py -- lane, wave and workgroup extent - 1, 0, + 1 in output pixels, the smallest frames, chunks of
rows short, exact and one over, dropped last rows -- for every output family, from 8-bit and from deep mosaics with junk
above their depth, with and without the colour stage.  Every destination is prefilled with 0xA5, has a stride padded by
8 and lies inside a larger allocation: nothing but the first px * OW bytes of a row may change -- not the row padding
(which is also what separates the rows of two planes), not the bytes between two frames, not the bytes after the last
one -- and the mosaic must come back as it went in."""
import numpy as np
import pytest

import half_cases as hc
import half_model as hf
import strip_cases as sc

pytestmark = pytest.mark.gpu

FILL = hf.GUARD
GUARD = 4096
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)      # rows sum to 1 (tests/test_gpu_colour.py)


def fam_id(fam):
    return fam.fmt + ("be" if fam.dbe else "")


def stage_for(pkg, bits):
    """matrix + sRGB curve and a black level, as tests/test_gpu_planar.py"""
    return pkg.Colour.make(black=(1 << sc.depth_of(bits)) // 16, gains=(1.9, 1.0, 1.6), ccm=CCM, curve=pkg.TONE_SRGB)


def model_kw(col):
    return None if col is None else dict(black=tuple(col.black[:]), matrix=tuple(col.matrix[:]), tone=col.tone_table())


def open_ctx(pkg, case, col=None, src_stride=0, dst_stride=0, **kw):
    fam = case.family
    return pkg.Context(case.w, case.h, case.order, fam.fmt, src_stride=src_stride, dst_stride=dst_stride, bits=case.bits,
                       src_big_endian=case.sbe, dst_big_endian=fam.dbe, method="half", colour=col, device=0, **kw)


def expect(case, buf, col, dst_stride):
    fam = case.family
    return hf.frame(buf, case.w, case.h, case.order, fam.fmt, bits=case.bits, colour=model_kw(col),
                    src_big_endian=case.sbe, dst_big_endian=fam.dbe, src_stride=buf.shape[1], dst_stride=dst_stride)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else "%d bytes differ, first at row %d byte %d (got %d, want %d)" % (
        len(bad), bad[0][0], bad[0][1], got[tuple(bad[0])], want[tuple(bad[0])])


def convert_on_device(ctx, bufs, src_off=0, dst_off=0, src_pitch=None, dst_pitch=None, as_list=False):
    """one launch over len(bufs) frames (mibayer_process_device, or _list over separate allocations) into destinations
    prefilled with FILL that lie GUARD bytes inside their allocation, the base pointers src_off / dst_off bytes off the
    allocations' alignment, the frames src_pitch / dst_pitch bytes apart.  Returns the frames (n, rows, dst_stride),
    whether any byte outside them changed, and whether the mosaics changed"""
    n = len(bufs)
    flat = [np.ascontiguousarray(b).reshape(-1) for b in bufs]
    assert all(f.size == ctx.src_bytes for f in flat)
    spitch, dpitch = src_pitch or ctx.src_bytes, dst_pitch or ctx.dst_bytes
    allocs = []

    def alloc(nbytes):
        allocs.append(ctx.device_alloc(nbytes))
        return allocs[-1]
    try:
        if as_list:
            total = ctx.dst_bytes + 2 * GUARD + dst_off
            d_srcs = [alloc(ctx.src_bytes + src_off + 16) + src_off for _ in range(n)]
            d_dsts = [alloc(total) for _ in range(n)]
            for f, s, d in zip(flat, d_srcs, d_dsts):
                ctx.to_device(s, f)
                ctx.to_device(d, np.full(total, FILL, np.uint8))
            ctx.process_device_list(d_srcs, [d + GUARD + dst_off for d in d_dsts])
            ctx.sync()
            outs = [ctx.from_device(d, total) for d in d_dsts]
            srcs = [ctx.from_device(s, ctx.src_bytes) for s in d_srcs]
        else:
            total = n * dpitch + 2 * GUARD + dst_off
            src = np.full(n * spitch, 0x3C, np.uint8)
            for k, f in enumerate(flat):
                src[k * spitch:k * spitch + f.size] = f
            d_src, d_dst = alloc(src.size + src_off + 16), alloc(total)
            ctx.to_device(d_src + src_off, src)
            ctx.to_device(d_dst, np.full(total, FILL, np.uint8))
            ctx.process_device(d_src + src_off, d_dst + GUARD + dst_off, n, src_frame_bytes=spitch, dst_frame_bytes=dpitch)
            ctx.sync()
            out = ctx.from_device(d_dst, total)
            back = ctx.from_device(d_src + src_off, src.size)
            srcs, flat = [back], [src]
            outs = None
    finally:
        for p in allocs:
            ctx.device_free(p)
    lo = GUARD + dst_off
    if outs is None:
        body = out[lo:lo + n * dpitch].reshape(n, dpitch)
        outside = not ((out[:lo] == FILL).all() and (out[lo + n * dpitch:] == FILL).all()
                       and (body[:, ctx.dst_bytes:] == FILL).all())
        frames = body[:, :ctx.dst_bytes]
    else:
        outside = not all((o[:lo] == FILL).all() and (o[lo + ctx.dst_bytes:] == FILL).all() for o in outs)
        frames = np.stack([o[lo:lo + ctx.dst_bytes] for o in outs])
    touched = not all(np.array_equal(a, b) for a, b in zip(srcs, flat))
    return frames.reshape(n, ctx.dst_rows, ctx.dst_stride).copy(), outside, touched


def run_cases(pkg, cases, seed, with_colour):
    """random frames (junk above the depth), a source stride padded by 12, a destination stride padded by 8.  Collects
    every failing case so that one run names every size that is wrong"""
    rng = np.random.default_rng(seed)
    bad = []
    for case in cases:
        fam = case.family
        ow, oh = hc.out_size(case.w, case.h)
        col = stage_for(pkg, case.bits) if with_colour else None
        sstride = sc.src_row_bytes(case.w, case.bits) + 12      # rows dword-aligned, not 8-byte-aligned
        dstride = hc.padded_dst_stride(fam, ow)
        buf = sc.random_frame(rng, case.w, case.h, case.bits, sstride, case.sbe)
        with open_ctx(pkg, case, col, sstride, dstride) as ctx:
            assert ctx.half and (ctx.out_width, ctx.out_height) == (ow, oh) and (ctx.width, ctx.height) == (case.w, case.h)
            assert ctx.dst_stride == dstride and ctx.dst_bytes == dstride * oh * (3 if fam.px == 1 else 1)
            want = expect(case, buf, col, dstride)
            out, outside, touched = convert_on_device(ctx, [buf])
        where = (fam_id(fam), case.w, case.h, case.order, case.bits, case.sbe)
        if outside:
            bad.append((where, "bytes outside the frame written"))
        if touched:
            bad.append((where, "the mosaic changed"))
        if not np.array_equal(out[0], want):
            pad = (out[0][:, fam.px * ow:] == FILL).all()
            bad.append((where, "padding %s; %s" % ("intact" if pad else "WRITTEN", first_difference(out[0], want))))
    return bad


# -- every family, every size, both sample widths ----------------------------------------------------------------------

@pytest.mark.parametrize("colour", [False, True], ids=["plain", "colour"])
@pytest.mark.parametrize("fam", hc.FAMILIES, ids=fam_id)
def test_every_size_of_the_table(gpu_pkg, fam, colour):
    i = hc.FAMILIES.index(fam)
    bad = run_cases(gpu_pkg, hc.cases(fam, i), 100 + i, colour)
    assert not bad, bad


def test_the_identity_stage_gives_the_plain_bytes(gpu_pkg):
    """zero black level, the identity matrix and no curve: the bytes of the same cfg without the flag; a linear tone
    table on top leaves 16-bit output unchanged"""
    rng = np.random.default_rng(7)
    for i, fam in enumerate(hc.FAMILIES):
        case = hc.Case(2 * 261, 11, hc.ORDERS[i % 4], fam, *hc.SAMPLES[i % len(hc.SAMPLES)])
        buf = sc.random_frame(rng, case.w, case.h, case.bits, None, case.sbe)
        row = fam.px * 261              # (the destination of process_batch_via_device is not prefilled: no padding here)
        with open_ctx(gpu_pkg, case) as plain:
            assert plain.variant_name == "half_256x4"
            want = plain.process_batch_via_device(buf[None])[0][:, :row]
        with open_ctx(gpu_pkg, case, True) as ctx:
            assert ctx.variant_name == "colour_half_256x4" and ctx.colour
            assert np.array_equal(ctx.process_batch_via_device(buf[None])[0][:, :row], want), fam
            if fam.px == 8:
                ctx.set_colour(gpu_pkg.Colour(tone=gpu_pkg.colour_tone(gpu_pkg.TONE_LINEAR)))
                assert np.array_equal(ctx.process_batch_via_device(buf[None])[0][:, :row], want), fam
            stride = ctx.dst_stride
        assert np.array_equal(want, expect(case, buf, None, stride)[:, :row]), fam


# -- batches, lists, alignment -------------------------------------------------------------------------------------------

BATCH_FAMILIES = (hc.FAMILIES[1], hc.FAMILIES[5], hc.FAMILIES[6], hc.FAMILIES[8])     # BGRx, ARGB64 be, RGB, GBR


@pytest.mark.parametrize("fam", BATCH_FAMILIES, ids=fam_id)
def test_batch_of_3_with_pitches_larger_than_a_frame(gpu_pkg, fam):
    rng = np.random.default_rng(21)
    for bits, sbe, ow in ((0, False, 259), (12, True, 257)):
        case = hc.Case(2 * ow, 2 * hc.ROWS + 3, "gbrg", fam, bits, sbe)
        col = stage_for(gpu_pkg, bits) if bits else None
        sstride = sc.src_row_bytes(case.w, bits) + 4
        dstride = hc.padded_dst_stride(fam, ow)
        bufs = [sc.random_frame(rng, case.w, case.h, bits, sstride, sbe) for _ in range(3)]
        with open_ctx(gpu_pkg, case, col, sstride, dstride) as ctx:
            out, outside, touched = convert_on_device(ctx, bufs, src_pitch=ctx.src_bytes + 36,
                                                      dst_pitch=ctx.dst_bytes + 200)
        assert not outside and not touched, (fam, bits)
        for k in range(3):
            assert np.array_equal(out[k], expect(case, bufs[k], col, dstride)), (fam, bits, k)


@pytest.mark.parametrize("fam", BATCH_FAMILIES, ids=fam_id)
def test_list_launch_of_17_frames(gpu_pkg, fam):
    """one more than a list launch holds: a launch of 16 and a launch of 1"""
    rng = np.random.default_rng(22)
    assert hc.MAX_LIST == 16
    case = hc.Case(2 * 67, 2 * hc.ROWS + 1, "grbg", fam, 10, False)
    col = stage_for(gpu_pkg, case.bits)
    bufs = [sc.random_frame(rng, case.w, case.h, case.bits, None, case.sbe) for _ in range(17)]
    dstride = hc.padded_dst_stride(fam, 67)
    with open_ctx(gpu_pkg, case, col, 0, dstride) as ctx:
        out, outside, touched = convert_on_device(ctx, bufs, as_list=True)
    assert not outside and not touched
    for k in range(17):
        assert np.array_equal(out[k], expect(case, bufs[k], col, dstride)), (fam, k)


@pytest.mark.parametrize("fam", hc.FAMILIES[:1] + BATCH_FAMILIES[1:], ids=fam_id)
def test_base_pointers_at_4_mod_8(gpu_pkg, fam):
    rng = np.random.default_rng(23)
    for bits, sbe in ((0, False), (16, False)):
        for ow in (255, 256, 261):
            dst_off = 4                 # 16-bit channels too: their rows are 8 bytes apart, the base is only dword-aligned
            case = hc.Case(2 * ow, 9, "bggr", fam, bits, sbe)
            bufs = [sc.random_frame(rng, case.w, case.h, bits, None, sbe) for _ in range(2)]
            with open_ctx(gpu_pkg, case) as ctx:
                out, outside, touched = convert_on_device(ctx, bufs, src_off=4, dst_off=dst_off,
                                                          src_pitch=ctx.src_bytes + 4, dst_pitch=ctx.dst_bytes + 8)
                for as_list in (False, True):
                    if as_list:
                        out, outside, touched = convert_on_device(ctx, bufs, src_off=4, dst_off=dst_off, as_list=True)
                    assert not outside and not touched, (fam, bits, ow, as_list)
                    for k in range(2):
                        assert np.array_equal(out[k], expect(case, bufs[k], None, ctx.dst_stride)), (fam, bits, ow, k)


def test_one_long_batch_of_narrow_frames(gpu_pkg):
    """64 frames of 6 x (2 ROWS + 1): three output pixels in one lane, a wave per frame"""
    rng = np.random.default_rng(24)
    for fam, bits in ((hc.FAMILIES[3], 0), (hc.FAMILIES[4], 14), (hc.FAMILIES[7], 0), (hc.FAMILIES[10], 12)):
        case = hc.Case(6, 2 * hc.ROWS + 1, "rggb", fam, bits, False)
        bufs = [sc.random_frame(rng, case.w, case.h, bits, None, False) for _ in range(64)]
        with open_ctx(gpu_pkg, case) as ctx:
            assert (ctx.out_width, ctx.out_height) == (3, hc.ROWS)
            out, outside, touched = convert_on_device(ctx, bufs)
        assert not outside and not touched, fam
        for k in range(64):
            assert np.array_equal(out[k], expect(case, bufs[k], None, ctx.dst_stride)), (fam, k)


# -- a HALF context is a deep context: one kernel shape, no plans --------------------------------------------------------

def test_plans_are_refused_and_the_generator_works(gpu_pkg):
    pkg = gpu_pkg
    with pkg.Context(258, 37, "rggb", "BGRx", method="half", device=0, flags=pkg.FLAG_HIPGRAPH) as ctx:
        assert ctx.variant_name == "half_256x4" and ctx.method == "half"
        assert (ctx.out_width, ctx.out_height, ctx.dst_stride, ctx.dst_bytes) == (129, 18, 516, 516 * 18)
        d_src, d_dst = ctx.device_alloc(2 * ctx.src_bytes), ctx.device_alloc(2 * ctx.dst_bytes)
        try:
            for call in (lambda: ctx.autotune(d_src, d_dst, 2), lambda: ctx.autotune_list([d_src], [d_dst]),
                         lambda: ctx.set_plan(1, 0), lambda: ctx.set_plan_for(1, 1, 0), lambda: ctx.launch_geometry(1)):
                with pytest.raises(pkg.MibayerError) as err:
                    call()
                assert err.value.status == pkg.ERR_ARG
            # pitches smaller than a frame are refused by the OUTPUT frame's size, not the mosaic's
            with pytest.raises(pkg.MibayerError) as err:
                ctx.process_device(d_src, d_dst, 2, dst_frame_bytes=ctx.dst_bytes - 4)
            assert err.value.status == pkg.ERR_GEOMETRY
            ctx.fill_synthetic(d_src, 2, seed=5)
            ctx.process_device(d_src, d_dst, 2)
            ms = ctx.time_device(d_src, d_dst, 2, warmup=1, reps=2)
            ctx.sync()
            assert ms > 0
            src = ctx.from_device(d_src, 2 * ctx.src_bytes).reshape(2, 37, 260)
            out = ctx.from_device(d_dst, 2 * ctx.dst_bytes).reshape(2, 18, 516)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_dst)
        for k in range(2):
            assert np.array_equal(out[k], hf.frame(src[k], 258, 37, "rggb", "BGRx", src_stride=260))
        # the HIPGRAPH flag is accepted and the host path runs without graphs
        assert np.array_equal(ctx.process_host(src[0]), out[0])
    # the generator writes 8-bit mosaics only
    with pkg.Context(258, 37, "rggb", "BGRx", method="half", bits=12, device=0) as ctx:
        d_src = ctx.device_alloc(ctx.src_bytes)
        try:
            with pytest.raises(pkg.MibayerError) as err:
                ctx.fill_synthetic(d_src, 1, seed=5)
            assert err.value.status == pkg.ERR_ARG
        finally:
            ctx.device_free(d_src)
    # a default context is what it was
    with pkg.Context(258, 37, "rggb", "BGRx", device=0) as ctx:
        assert not ctx.half and (ctx.out_width, ctx.out_height) == (258, 37) and ctx.dst_bytes == 258 * 4 * 37
