"""GPU tests of planar 8-bit output (include/mibayer.h, MIBAYER_FLAG_DST_PLANAR): store_planes8
(csrc/mibayer_kernels.hip) under the deep, MHC and colour kernels, bit-exact against tests/planar_model.py -- the 4-byte
models' RGBx frame dealt to three planes.  A lane writes its group of 4 pixels as one dword per plane at 4 g of the row,
the 2-pixel tail of a width % 4 == 2 row as two bytes per plane; the shapes are the smallest at which that can go wrong
(tests/strip_cases.py): full group and tail, the last group in lanes 63 / 0 / 1 around the first strip seam and behind
the second, the chunk edges.  Every destination is prefilled with 0xA5 and nothing but the first `width` bytes of a row
of a plane may change: a store past the last row of plane k would show in the first row of plane k + 1 or in the
padding."""
import collections

import numpy as np
import pytest

import planar_model as pm
import strip_cases as sc

pytestmark = pytest.mark.gpu

FILL = 0xA5
GUARD = 4096
CCM = (1.62, -0.48, -0.14, -0.21, 1.43, -0.22, 0.03, -0.55, 1.52)      # rows sum to 1 (tests/test_gpu_colour.py)

Arm = collections.namedtuple("Arm", "name method bits sbe colour")
DEEP8 = Arm("deep_8_to_planar", "bilinear", 0, False, False)     # bayer2rgb_deep_kernel<true, false>
MHC8 = Arm("mhc_8_to_planar", "mhc", 0, False, False)
ARMS = (
    DEEP8,
    Arm("deep_12_to_planar", "bilinear", 12, False, False),
    MHC8,
    Arm("mhc_10be_to_planar", "mhc", 10, True, False),
    Arm("colour_bilinear_8_to_planar", "bilinear", 0, False, True),
    Arm("colour_mhc_14_to_planar", "mhc", 14, False, True),
)
WIDTHS = (20, 22, 254, 256, 258, 260, 510, 516)
HEIGHTS = (3, 4, 15, 16, 17, 33)
HEIGHT_WIDTHS = (258, 260)
assert set(WIDTHS) <= set(sc.WIDTHS) and set(HEIGHTS) <= set(sc.HEIGHTS)

Case = collections.namedtuple("Case", "w h order fmt")


def rotate(i, w, h):
    """Bayer order (period 4) and plane permutation (period 6) rotate with the case index: 12 pairs in turn"""
    return Case(w, h, sc.ORDERS[i % 4], pm.PERMUTATIONS[i % 6])


def test_the_cases_cover_all_six_permutations_and_four_orders():
    """every arm's width sweep alone meets every permutation and every Bayer order"""
    for a in range(len(ARMS)):
        cases = [rotate(a + i, w, sc.SWEEP_HEIGHT) for i, w in enumerate(WIDTHS)]
        assert {c.fmt for c in cases} == set(pm.PERMUTATIONS), a
        assert {c.order for c in cases} == set(sc.ORDERS), a


def arm_id(arm):
    return arm.name


def stage_of(pkg, arm):
    """matrix + sRGB curve (and a black level), as tests/test_gpu_strip_geometry.py; None for a plain arm"""
    if not arm.colour:
        return None
    return pkg.Colour.make(black=(1 << sc.depth_of(arm.bits)) // 16, gains=(1.9, 1.0, 1.6), ccm=CCM, curve=pkg.TONE_SRGB)


def model_kw(col):
    return None if col is None else dict(black=tuple(col.black[:]), matrix=tuple(col.matrix[:]), tone=col.tone_table())


def open_ctx(pkg, arm, case, col=None, src_stride=0, dst_stride=0, flags=0, **kw):
    return pkg.Context(case.w, case.h, case.order, case.fmt, src_stride=src_stride, dst_stride=dst_stride,
                       bits=arm.bits, src_big_endian=arm.sbe, method=arm.method, flags=flags | pkg.FLAG_DST_PLANAR,
                       colour=(col if col is not None else True) if arm.colour else None, device=0, **kw)


def frame(rng, arm, case, stride=None):
    return sc.random_frame(rng, case.w, case.h, arm.bits, stride, arm.sbe)


def expect(arm, buf, case, col=None, dst_stride=None):
    """the model's frame (3, h, dst_stride); the padding is FILL"""
    return pm.bayer2rgb_planar(buf, case.w, case.h, case.order, case.fmt, bits=arm.bits, method=arm.method,
                               colour=model_kw(col), src_big_endian=arm.sbe, src_stride=buf.shape[1],
                               dst_stride=dst_stride)


def first_difference(got, want):
    bad = np.argwhere(got != want)
    return "no difference" if not len(bad) else "%d bytes differ, first at plane %d row %d byte %d (got %d, want %d)" % (
        len(bad), bad[0][0], bad[0][1], bad[0][2], got[tuple(bad[0])], want[tuple(bad[0])])


def convert_on_device(ctx, bufs, src_off=0, dst_off=0, dst_pitch=None):
    """one mibayer_process_device launch over len(bufs) frames into a destination prefilled with FILL that lies GUARD
    bytes inside its allocation, the base pointers src_off / dst_off bytes off the allocations' alignment, the frames
    dst_pitch bytes apart.  Returns the frames (n, 3, h, dst_stride) and whether any byte outside them changed"""
    n = len(bufs)
    src = np.stack([np.ascontiguousarray(b).reshape(-1) for b in bufs])
    assert src.shape[1] == ctx.src_bytes and ctx.dst_bytes == 3 * ctx.dst_stride * ctx.height
    pitch = dst_pitch or ctx.dst_bytes
    total = n * pitch + 2 * GUARD + dst_off
    d_src = ctx.device_alloc(src.size + src_off + 16)
    d_dst = ctx.device_alloc(total)
    try:
        ctx.to_device(d_src + src_off, src)
        ctx.to_device(d_dst, np.full(total, FILL, np.uint8))
        ctx.process_device(d_src + src_off, d_dst + GUARD + dst_off, n, dst_frame_bytes=pitch)
        ctx.sync()
        out = ctx.from_device(d_dst, total)
    finally:
        ctx.device_free(d_src)
        ctx.device_free(d_dst)
    lo = GUARD + dst_off
    body = out[lo:lo + n * pitch].reshape(n, pitch)
    outside = not ((out[:lo] == FILL).all() and (out[lo + n * pitch:] == FILL).all()
                   and (body[:, ctx.dst_bytes:] == FILL).all())
    return body[:, :ctx.dst_bytes].reshape(n, 3, ctx.height, ctx.dst_stride).copy(), outside


def run_cases(pkg, arm, sizes, seed, first_index=0):
    """random frames (junk above the depth), a padded source stride; the destination stride alternates between the
    default and ROUND_UP_4 (w) + 8.  Collects every failing case so that one run names every width that is wrong"""
    rng = np.random.default_rng(seed)
    col = stage_of(pkg, arm)
    bad = []
    for i, (w, h) in enumerate(sizes):
        case = rotate(first_index + i, w, h)
        sstride = sc.src_row_bytes(w, arm.bits) + 12            # rows dword-aligned, not 8-byte-aligned
        dstride = pm.default_stride(w) + 8 if i % 2 else 0
        buf = frame(rng, arm, case, sstride)
        with open_ctx(pkg, arm, case, col, sstride, dstride) as ctx:
            assert ctx.dst_stride == (dstride or pm.default_stride(w)) and ctx.dst_bytes == 3 * ctx.dst_stride * h
            want = expect(arm, buf, case, col, ctx.dst_stride)
            out, outside = convert_on_device(ctx, [buf])
        where = (arm.name, w, h, case.order, case.fmt, ctx.dst_stride)
        if outside:
            bad.append((where, "bytes outside the frame written"))
        if not np.array_equal(out[0], want):
            pad = (out[0][:, :, w:] == FILL).all()
            bad.append((where, "padding %s; %s" % ("intact" if pad else "WRITTEN", first_difference(out[0], want))))
    return bad


# -- arms, widths, heights ---------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS, ids=arm_id)
def test_widths_at_height_18(gpu_pkg, arm):
    bad = run_cases(gpu_pkg, arm, [(w, sc.SWEEP_HEIGHT) for w in WIDTHS], 1, ARMS.index(arm))
    assert not bad, bad


@pytest.mark.parametrize("arm", ARMS, ids=arm_id)
def test_heights_at_widths_258_and_260(gpu_pkg, arm):
    bad = run_cases(gpu_pkg, arm, [(w, h) for w in HEIGHT_WIDTHS for h in HEIGHTS], 2, ARMS.index(arm) + 1)
    assert not bad, bad


def test_plain_8_bit_planes_are_the_production_kernels_bytes(gpu_pkg):
    """deep 8 -> planes (bayer2rgb_deep_kernel<true, false>) against a context WITHOUT the flag: the production kernels'
    RGBx frame, which is pinned to the reference, de-interleaved -- no model involved"""
    rng = np.random.default_rng(3)
    for i, w in enumerate(WIDTHS):
        case = rotate(i, w, sc.SWEEP_HEIGHT)
        buf = frame(rng, DEEP8, case)
        with gpu_pkg.Context(w, case.h, case.order, "RGBx", device=0) as plain:
            assert not plain.deep
            four = plain.process_batch_via_device(buf[None])[0].reshape(case.h, w, 4)
        with open_ctx(gpu_pkg, DEEP8, case) as ctx:
            assert ctx.deep and ctx.planar and ctx.cfg.flags & gpu_pkg.FLAG_DST_PLANAR
            got = ctx.planes(ctx.process_batch_via_device(buf[None])[0])
        assert got.shape == (3, case.h, w) and (four[:, :, 3] == 255).all()
        for c in range(3):
            assert np.array_equal(got[case.fmt[c]], four[:, :, c]), (case, c)


# -- bytes that must not be written ------------------------------------------------------------------------------------

@pytest.mark.parametrize("path", ["device", "host"])
@pytest.mark.parametrize("arm", [DEEP8, MHC8], ids=arm_id)
def test_padding_keeps_what_it_held(gpu_pkg, arm, path):
    """width % 4 == 2 at the default stride (a row ends two bytes before it) and every width at ROUND_UP_4 (w) + 8:
    bytes [w, stride) of every row of every plane are still 0xA5, and the first row of plane k + 1 is the model's"""
    rng = np.random.default_rng(4)
    sizes = [(w, 0) for w in (22, 258, 510)] + [(w, pm.default_stride(w) + 8) for w in (22, 258, 260, 510)]
    for i, (w, dstride) in enumerate(sizes):
        case = rotate(i, w, sc.SWEEP_HEIGHT)
        buf = frame(rng, arm, case)
        with open_ctx(gpu_pkg, arm, case, dst_stride=dstride) as ctx:
            stride = ctx.dst_stride
            assert stride == (dstride or w + 2)
            want = expect(arm, buf, case, dst_stride=stride)
            if path == "device":
                got, outside = convert_on_device(ctx, [buf])
                got = got[0]
                assert not outside, (case, stride)
            else:
                got = ctx.process_host(buf, np.full((3 * case.h, stride), FILL, np.uint8)).reshape(3, case.h, stride)
        assert (got[:, :, w:] == FILL).all(), (arm.name, path, case, stride, "padding written")
        assert np.array_equal(got[1:, 0], want[1:, 0]), (arm.name, path, case, "first row of planes 1, 2")
        assert np.array_equal(got, want), (arm.name, path, case, stride, first_difference(got, want))


# -- alignment and batching --------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS, ids=arm_id)
def test_base_pointers_at_4_mod_16_and_a_pitched_batch(gpu_pkg, arm):
    """source and destination at 4 mod 16; then three frames whose destination pitch is 3 * stride * h + 4"""
    rng = np.random.default_rng(5)
    col = stage_of(gpu_pkg, arm)
    for i, w in enumerate((254, 258, 260)):
        case = rotate(i + ARMS.index(arm), w, sc.SWEEP_HEIGHT)
        bufs = [frame(rng, arm, case) for _ in range(3)]
        with open_ctx(gpu_pkg, arm, case, col) as ctx:
            wants = [expect(arm, b, case, col, ctx.dst_stride) for b in bufs]
            one, outside = convert_on_device(ctx, bufs[:1], 4, 4)
            assert not outside and np.array_equal(one[0], wants[0]), (arm.name, case, first_difference(one[0], wants[0]))
            out, outside = convert_on_device(ctx, bufs, 4, 4, dst_pitch=ctx.dst_bytes + 4)
            with pytest.raises(gpu_pkg.MibayerError) as e:      # a pitch of one plane short of the frame
                convert_on_device(ctx, bufs, dst_pitch=2 * ctx.dst_stride * case.h)
            assert e.value.status == gpu_pkg.ERR_GEOMETRY
        assert not outside, (arm.name, case, "bytes between or around the frames written")
        for f in range(3):
            assert np.array_equal(out[f], wants[f]), (arm.name, case, f, first_difference(out[f], wants[f]))


def list_launch(ctx, bufs):
    """one mibayer_process_device_list call over separately allocated frames, each destination prefilled with FILL
    and GUARD bytes longer than the frame; returns the frames and whether a byte behind one changed"""
    srcs = [ctx.device_alloc(ctx.src_bytes) for _ in bufs]
    dsts = [ctx.device_alloc(ctx.dst_bytes + GUARD) for _ in bufs]
    try:
        for d, b in zip(srcs, bufs):
            ctx.to_device(d, b)
        for d in dsts:
            ctx.to_device(d, np.full(ctx.dst_bytes + GUARD, FILL, np.uint8))
        ctx.process_device_list(srcs, dsts)
        ctx.sync()
        raw = [ctx.from_device(d, ctx.dst_bytes + GUARD) for d in dsts]
    finally:
        for d in srcs + dsts:
            ctx.device_free(d)
    behind = any(not (r[ctx.dst_bytes:] == FILL).all() for r in raw)
    return [r[:ctx.dst_bytes].reshape(3, ctx.height, ctx.dst_stride) for r in raw], behind


@pytest.mark.parametrize("n", [3, sc.MAX_LIST + 1])
@pytest.mark.parametrize("arm", [DEEP8, ARMS[1], MHC8, ARMS[4]], ids=arm_id)
def test_list_launches(gpu_pkg, arm, n):
    """3 separately allocated frames, and 17: one more than kMaxList, so the call splits into two launches"""
    rng = np.random.default_rng(6)
    col = stage_of(gpu_pkg, arm)
    case = rotate(n + ARMS.index(arm), 258, sc.SWEEP_HEIGHT)
    bufs = [frame(rng, arm, case) for _ in range(n)]
    with open_ctx(gpu_pkg, arm, case, col) as ctx:
        got, behind = list_launch(ctx, bufs)
        assert not behind
        for f, b in enumerate(bufs):
            want = expect(arm, b, case, col, ctx.dst_stride)
            assert np.array_equal(got[f], want), (arm.name, case, f, first_difference(got[f], want))


# -- host path ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", ARMS, ids=arm_id)
def test_host_path_synchronous_and_three_in_flight(gpu_pkg, arm):
    rng = np.random.default_rng(7)
    col = stage_of(gpu_pkg, arm)
    case = rotate(2 + ARMS.index(arm), (258, 260)[ARMS.index(arm) % 2], sc.SWEEP_HEIGHT)
    bufs = [frame(rng, arm, case) for _ in range(5)]
    with open_ctx(gpu_pkg, arm, case, col, inflight=3) as ctx:
        shape = (3, case.h, ctx.dst_stride)
        wants = [expect(arm, b, case, col, ctx.dst_stride) for b in bufs]
        got = ctx.process_host(bufs[0]).reshape(shape)
        assert np.array_equal(got, wants[0]), (arm.name, case, first_difference(got, wants[0]))
        dsts = [np.full(shape, FILL, np.uint8) for _ in bufs]
        srcs = [np.ascontiguousarray(b).reshape(-1) for b in bufs]
        tags = []
        for i in range(len(bufs) + 3):
            if i >= 3:
                tags.append(ctx.wait())
            if i < len(bufs):
                ctx.submit(srcs[i], dsts[i], tag=i + 1)
        assert tags == [1, 2, 3, 4, 5] and ctx.pending() == 0
    for f in range(len(bufs)):
        assert np.array_equal(dsts[f], wants[f]), (arm.name, case, f, first_difference(dsts[f], wants[f]))


BANDED = (2730, 2048)           # stride 2732: dst_bytes = 3 * 2732 * 2048 = 16 785 408 >= 16 MiB, where banding starts


@pytest.mark.parametrize("arm", [DEEP8, MHC8], ids=arm_id)
def test_host_path_banded_frame(gpu_pkg, arm):
    """one frame the host path converts in four bands (four kernel launches over chunk ranges, three 2-D downloads of
    `width` bytes a row per band, one per plane): a tail group and two padding bytes in every row at once"""
    w, h = BANDED
    case = Case(w, h, "grbg" if arm is DEEP8 else "bggr", (2, 0, 1) if arm is DEEP8 else (1, 2, 0))
    rng = np.random.default_rng(8)
    buf = frame(rng, arm, case)
    with open_ctx(gpu_pkg, arm, case) as ctx:
        assert ctx.dst_stride == 2732 and ctx.dst_bytes == 16785408 >= 16 << 20
        got = ctx.process_host(buf, np.full((3 * h, 2732), FILL, np.uint8)).reshape(3, h, 2732)
        via_device = ctx.process_batch_via_device(buf[None])[0].reshape(3, h, 2732)
    assert (got[:, :, w:] == FILL).all(), "padding written on the banded host path"
    assert np.array_equal(got[:, :, :w], via_device[:, :, :w]), first_difference(got[:, :, :w], via_device[:, :, :w])
    want = expect(arm, buf, case, dst_stride=2732)
    assert np.array_equal(got, want), (arm.name, first_difference(got, want))


# -- pool and statistics -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("arm", [DEEP8, ARMS[3]], ids=arm_id)
def test_pool_over_two_shards_of_one_device(gpu_pkg, arm):
    rng = np.random.default_rng(9)
    w, h, n = 258, sc.SWEEP_HEIGHT, 7
    case = rotate(1 + ARMS.index(arm), w, h)
    bufs = [np.ascontiguousarray(frame(rng, arm, case)).reshape(-1) for _ in range(n)]
    stride = pm.default_stride(w)
    outs = [np.full((3, h, stride), FILL, np.uint8) for _ in range(n)]
    with gpu_pkg.Pool([0, 0], w, h, case.order, case.fmt, inflight=2, bits=arm.bits, src_big_endian=arm.sbe,
                      method=arm.method, flags=gpu_pkg.FLAG_DST_PLANAR) as pool:
        done = []
        for i in range(n):
            while pool.pending() >= pool.capacity:
                done.append(pool.wait())
            pool.submit(bufs[i], outs[i], tag=i + 1)
        while pool.pending():
            done.append(pool.wait())
    assert done == list(range(1, n + 1))
    for i in range(n):
        want = expect(arm, bufs[i].reshape(h, -1), case, dst_stride=stride)
        assert np.array_equal(outs[i], want), (arm.name, i, first_difference(outs[i], want))


def test_statistics_are_those_of_a_four_byte_context(gpu_pkg):
    """mibayer_set_stats reads the mosaic only: the same zones as on a 4-byte context, and the planes unchanged"""
    rng = np.random.default_rng(10)
    w, h = 258, 34
    case = Case(w, h, "gbrg", (2, 0, 1))
    buf = frame(rng, DEEP8, case)
    with gpu_pkg.Context(w, h, case.order, "BGRx", device=0) as four, open_ctx(gpu_pkg, DEEP8, case) as ctx:
        plain = ctx.process_host(buf).copy()
        four.set_stats(4, 3, 8, 247)
        ctx.set_stats(4, 3, 8, 247)
        four.process_host(buf)
        got = ctx.process_host(buf)
        a, b = four.frame_stats(), ctx.frame_stats()
    assert np.array_equal(got, plain) and np.array_equal(plain.reshape(3, h, -1), expect(DEEP8, buf, case))
    assert a.tobytes() == b.tobytes() and int(a["count"].sum()) > 0


# -- the deep-context contract -----------------------------------------------------------------------------------------

def test_a_planar_context_is_a_deep_context(gpu_pkg):
    """mibayer_get_cfg round trip, and the refusals of a context with one kernel shape and no plans"""
    pkg = gpu_pkg
    L = pkg.lib()
    with pkg.Context(258, 18, "rggb", "GBR", device=0, flags=pkg.FLAG_HIPGRAPH) as ctx:
        f = ctx.cfg
        assert (f.width, f.height, f.src_stride, f.dst_stride) == (258, 18, 260, 260)
        assert (f.r_off, f.g_off, f.b_off) == (2, 0, 1) and f.flags == pkg.FLAG_DST_PLANAR | pkg.FLAG_HIPGRAPH
        assert ctx.variant_name == "deep_256x16" and ctx.dst_bytes == 3 * 260 * 18
        d_src, d_dst = ctx.device_alloc(ctx.src_bytes), ctx.device_alloc(ctx.dst_bytes)
        try:
            with pytest.raises(pkg.MibayerError) as e:
                ctx.autotune(d_src, d_dst, 1)
            assert e.value.status == pkg.ERR_ARG
            with pytest.raises(pkg.MibayerError) as e:
                ctx.autotune_list([d_src], [d_dst])
            assert e.value.status == pkg.ERR_ARG
            assert L.mibayer_set_plan(ctx._h, 1, 0, 0) == pkg.ERR_ARG
            assert L.mibayer_set_plan_for(ctx._h, 1, 1, 0, 0) == pkg.ERR_ARG
            with pytest.raises(pkg.MibayerError) as e:
                ctx.launch_geometry(1)
            assert e.value.status == pkg.ERR_ARG
            # an 8-bit mosaic: the synthetic generator works, and the frame converts on the host path (no graphs)
            ctx.fill_synthetic(d_src, 1, seed=7)
            ctx.sync()
            src = ctx.from_device(d_src, ctx.src_bytes).reshape(18, 260)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_dst)
        got = ctx.process_host(src)
        want = pm.bayer2rgb_planar(src, 258, 18, "rggb", "GBR", src_stride=260)
        assert np.array_equal(got.reshape(3, 18, 260), want)
        assert np.array_equal(ctx.planes(got), want[:, :, :258])
    with pkg.Context(258, 18, "rggb", "RGBP", device=0, method="mhc") as mhc:
        assert mhc.variant_name == "mhc_256x16"
    with pkg.Context(258, 18, "rggb", "RGBP", device=0, bits=12) as deep:
        d_src = deep.device_alloc(deep.src_bytes)
        try:
            with pytest.raises(pkg.MibayerError):
                deep.fill_synthetic(d_src, 1, seed=7)
        finally:
            deep.device_free(d_src)

