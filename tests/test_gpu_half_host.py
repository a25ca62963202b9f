"""GPU tests of the half-size demosaic on the host path (csrc/mibayer_abi.hip: the frame is uploaded whole, the mosaic
passes and the half-size launch run on the mosaic, OH rows of px * OW bytes come back) and through the pool, bit-exact
against tests/half_model.py on the mosaic the models corrected, denoised and shaded.  The statistics are taken on the
mosaic, in source coordinates: they are those of a full-resolution context over the same frame.  The device path is
tests/test_gpu_half.py."""
import numpy as np
import pytest

import half_cases as hc
import half_model as hf
import strip_cases as sc
from test_gpu_dpc_host import KX, KY, cut_defects, shading_of, thresholds
from test_gpu_half import fam_id, model_kw, stage_for
from test_gpu_nr_host import apply, curve_of, model_mosaic

pytestmark = pytest.mark.gpu

W, H = 266, 53
OW, OH = 133, 26
FILL = hf.GUARD
# (family, bits, big-endian samples, colour stage)
ARMS = ((hc.FAMILIES[2], 0, False, False), (hc.FAMILIES[4], 12, True, True), (hc.FAMILIES[7], 10, False, False),
        (hc.FAMILIES[9], 0, False, True))


def arm_id(arm):
    return "%s_from_%d%s" % (fam_id(arm[0]), arm[1] or 8, "_colour" if arm[3] else "")


def open_half(pkg, fam, bits, sbe, col, dstride, method="half", **kw):
    return pkg.Context(W, H, "gbrg", fam.fmt, dst_stride=dstride, bits=bits, src_big_endian=sbe, dst_big_endian=fam.dbe,
                       method=method, colour=col, device=0, **kw)


def want_frame(mosaic, fam, bits, sbe, col, dstride):
    return hf.frame(mosaic, W, H, "gbrg", fam.fmt, bits=bits, colour=model_kw(col), src_big_endian=sbe,
                    dst_big_endian=fam.dbe, src_stride=mosaic.shape[1], dst_stride=dstride)


@pytest.mark.parametrize("arm", ARMS, ids=arm_id)
def test_process_host_and_three_in_flight_alone_and_behind_every_pass(gpu_pkg, arm):
    """process_host and submit / wait with three in flight, into destinations prefilled with 0xA5 at a stride padded by
    8: first with no pass on, then behind defect correction + noise reduction + shading with zones, histogram and focus
    measured -- the half frame is the model's of the corrected mosaic, and the three measurements are those a
    full-resolution context takes of the same frame"""
    pkg = gpu_pkg
    fam, bits, sbe, colour = arm
    vmax = (1 << (bits or 8)) - 1
    rng = np.random.default_rng([41, ARMS.index(arm)])
    col = stage_for(pkg, bits) if colour else None
    dstride = hc.padded_dst_stride(fam, OW)
    sstride = sc.src_row_bytes(W, bits)
    bufs = [sc.random_frame(rng, W, H, bits, sstride, sbe) for _ in range(4)]
    hot, cold = thresholds(bits)
    dpc = (hot, cold, cut_defects(W, H, [16, 32], rng))
    curve, shade = curve_of(bits), shading_of(W, H, bits, rng)
    rows = OH * (3 if fam.px == 1 else 1)

    with open_half(pkg, fam, bits, sbe, col, dstride, inflight=3) as ctx:
        assert (ctx.out_width, ctx.out_height, ctx.dst_rows, ctx.dst_bytes) == (OW, OH, rows, rows * dstride)
        for passes in (False, True):
            apply(pkg, ctx, dpc if passes else None, curve if passes else None, shade if passes else None)
            if passes:
                ctx.set_stats(3, 2, vmax // 16, vmax - vmax // 16)
                ctx.set_hist(True)
                ctx.set_focus(3, 5, vmax // 8)
            mosaics = [model_mosaic(b, W, H, sstride, bits, sbe, dpc if passes else None, curve if passes else None,
                                    shade if passes else None) for b in bufs]
            wants = [want_frame(m, fam, bits, sbe, col, dstride) for m in mosaics]
            if passes:
                assert not np.array_equal(mosaics[0], bufs[0])
            # one frame, synchronously
            dst = np.full((rows, dstride), FILL, np.uint8)
            src = np.ascontiguousarray(bufs[0]).reshape(-1).copy()
            got = ctx.process_host(src, dst)
            assert np.array_equal(got, wants[0]), (passes, "padding intact: %s" % (got[:, fam.px * OW:] == FILL).all())
            assert np.array_equal(src, np.ascontiguousarray(bufs[0]).reshape(-1))
            measured = (ctx.frame_stats().tobytes(), ctx.frame_hist().tobytes(), ctx.frame_focus().tobytes()) if passes else None
            # three in flight
            dsts = [np.full((rows, dstride), FILL, np.uint8) for _ in bufs]
            done = 0
            for i, b in enumerate(bufs):
                if ctx.pending() == 3:
                    assert ctx.wait() == done + 1
                    done += 1
                ctx.submit(np.ascontiguousarray(b).reshape(-1), dsts[i], tag=i + 1)
            while ctx.pending():
                assert ctx.wait() == done + 1
                done += 1
            for i in range(len(bufs)):
                assert np.array_equal(dsts[i], wants[i]), (passes, i)
            if not passes:
                continue
            # the measurements are the mosaic's: a full-resolution context over the same frame takes the same
            full_fmt = "ARGB64" if bits else "RGBx"
            with pkg.Context(W, H, "gbrg", full_fmt, bits=bits, src_big_endian=sbe, out16=bool(bits), device=0) as full:
                assert not full.half and full.dst_bytes == (8 if bits else 4) * W * H
                apply(pkg, full, dpc, curve, shade)
                full.set_stats(3, 2, vmax // 16, vmax - vmax // 16)
                full.set_hist(True)
                full.set_focus(3, 5, vmax // 8)
                full.process_host(np.ascontiguousarray(bufs[0]).reshape(-1))
                assert measured == (full.frame_stats().tobytes(), full.frame_hist().tobytes(),
                                    full.frame_focus().tobytes())
            assert int(ctx.frame_hist().sum()) == W * H               # source coordinates: every sample of the mosaic


def test_an_8k_context_is_launched_whole(gpu_lab_pkg):
    """the host path of a HALF context has no bands (an open item): host_bands is 1 where the full-resolution context of
    the same mosaic is cut into several.  The contexts are created only, no frame is converted"""
    pkg = gpu_lab_pkg
    with pkg.Context(8192, 4320, "rggb", "RGBx", method="half", device=0) as ctx:
        assert ctx.dst_bytes == 4096 * 4 * 2160 >= 16 << 20 and ctx.host_bands == 1
    with pkg.Context(8192, 4320, "rggb", "ARGB64", method="half", bits=12, device=0) as ctx:
        assert ctx.host_bands == 1
    with pkg.Context(8192, 4320, "rggb", "RGBx", device=0) as full:
        assert full.host_bands > 1


@pytest.mark.parametrize("arm", ARMS[:2], ids=arm_id)
def test_two_shard_pool_returns_the_same_bytes(gpu_pkg, arm):
    pkg = gpu_pkg
    fam, bits, sbe, colour = arm
    rng = np.random.default_rng([42, ARMS.index(arm)])
    col = stage_for(pkg, bits) if colour else None
    bufs = [sc.random_frame(rng, W, H, bits, None, sbe) for _ in range(5)]
    with open_half(pkg, fam, bits, sbe, col, 0) as ctx:
        dstride = ctx.dst_stride
        plain = [ctx.process_host(np.ascontiguousarray(b).reshape(-1)).copy() for b in bufs]
    for b, p in zip(bufs, plain):
        assert np.array_equal(p, want_frame(b, fam, bits, sbe, col, dstride))
    with pkg.Pool([0, 0], W, H, "gbrg", fam.fmt, inflight=2, bits=bits, src_big_endian=sbe, dst_big_endian=fam.dbe,
                  method="half", colour=col) as pool:
        outs = [np.full_like(plain[0], FILL) for _ in bufs]
        done = 0
        for i, b in enumerate(bufs):
            if pool.pending() == pool.capacity:
                assert pool.wait() == done + 1
                done += 1
            pool.submit(np.ascontiguousarray(b).reshape(-1), outs[i], tag=i + 1)
        while pool.pending():
            assert pool.wait() == done + 1
            done += 1
        assert done == len(bufs) and all(np.array_equal(o, p) for o, p in zip(outs, plain))


def test_shading_tables_and_defect_lists_are_in_source_coordinates(gpu_pkg):
    """the limits of the mosaic passes are the mosaic's on a HALF context: a defect in the last source column and row is
    accepted, one past them is refused"""
    pkg = gpu_pkg
    with pkg.Context(W, H, "gbrg", "RGBx", method="half", device=0) as ctx:
        ctx.set_dpc(pkg.Dpc(-1, -1, np.array([(W - 1, H - 1)], np.uint32)))
        with pytest.raises(pkg.MibayerError):
            ctx.set_dpc(pkg.Dpc(-1, -1, np.array([(W, 0)], np.uint32)))
        nx, ny = pkg.shading_nodes(W, H, KX, KY)
        assert (nx, ny) != pkg.shading_nodes(OW, OH, KX, KY)
        ctx.set_stats(64, 26, 0, 255)                  # zones_y <= H / 2 of the MOSAIC
        with pytest.raises(pkg.MibayerError):
            ctx.set_stats(64, 27, 0, 255)
