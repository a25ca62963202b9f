"""GPU tests of mosaic_hist_kernel over the tables of tests/hist_cases.py: every arm of the pair fusion under every lane
state, every sample value of every depth in both byte orders, the frame x strip x segment split under an odd window
origin, and the rows-per-workgroup rule between and at its clamps -- each through ONE mibayer_hist_device launch into
a junk-prefilled buffer, bit-exact against tests/hist_model.py, and every table's row sums against the window's size.
What the tables reach is asserted, without a GPU, by tests/test_hist_cases.py."""
import numpy as np
import pytest

import hist_cases as tc
import hist_model as hm
from test_gpu_hist import same

pytestmark = pytest.mark.gpu


def context(pkg, W, H, bits=0, big_endian=False, stride=0):
    if bits:
        return pkg.Context(W, H, "grbg", "ARGB64", src_stride=stride, device=0, bits=bits, src_big_endian=big_endian)
    return pkg.Context(W, H, "rggb", "RGBx", src_stride=stride, device=0)


def check(got, want, W, H, win):
    """one table against the model, and its row sums against the window alone"""
    same(got, want)
    assert got.sum(axis=1).tolist() == tc.window_counts(W, H, win)


@pytest.mark.parametrize("family", tc.FAMILIES)
def test_pair_fusion_arms(gpu_pkg, family):
    shapes = {}
    for c in tc.fusion_cases():
        shapes.setdefault((c.W, c.H, c.stride), []).append(c)
    for (W, H, stride), cases in shapes.items():
        raw = tc.fusion_frame(family, stride, H)
        S = tc.samples(raw, W, H)
        with context(gpu_pkg, W, H, stride=stride) as ctx:
            for c in cases:
                got, want = ctx.hist_batch_via_device(raw[None], c.win)[0], hm.histogram(S, 8, c.win)
                assert np.array_equal(got, want), (c, np.argwhere(got != want)[:8])
                check(got, want, W, H, c.win)


@pytest.mark.parametrize("big_endian", (False, True), ids=("le", "be"))
@pytest.mark.parametrize("bits", tc.DEEP_BITS)
def test_every_value_of_a_depth(gpu_pkg, bits, big_endian):
    W, H = tc.VALUE_SIZE
    with context(gpu_pkg, W, H, bits, big_endian) as ctx:
        got = ctx.hist_batch_via_device(tc.value_frame(bits, big_endian)[None])[0]
    assert (got == tc.VALUE_BIN).all(), np.argwhere(got != tc.VALUE_BIN)[:8]
    W, H = tc.EDGE_SIZE
    with context(gpu_pkg, W, H, bits, big_endian) as ctx:
        for raw in (tc.boundary_frame(bits, big_endian), tc.extremes_frame(bits, big_endian)):
            want = hm.histogram(tc.samples(raw, W, H, bits, big_endian), bits)
            check(ctx.hist_batch_via_device(raw[None])[0], want, W, H, (0, 0, 0, 0))


def test_every_byte_value(gpu_pkg):
    W, H = tc.VALUE_SIZE
    with context(gpu_pkg, W, H) as ctx:
        got = ctx.hist_batch_via_device(tc.value_frame(8)[None])[0]
    assert (got == tc.VALUE_BIN).all(), np.argwhere(got != tc.VALUE_BIN)[:8]


@pytest.mark.parametrize("case", tc.SPLIT_CASES, ids=lambda c: "%dbit" % (c.bits or 8))
def test_frames_strips_segments_and_window_together(gpu_pkg, case):
    padded, raws = tc.split_frames(case)
    S = [tc.samples(r, case.W, case.H, case.bits, case.big_endian) for r in raws]
    with context(gpu_pkg, case.W, case.H, case.bits, case.big_endian, case.stride) as ctx:
        for win in tc.SPLIT_WINDOWS[case.W]:
            want = np.stack([hm.histogram(s, tc.depth(case.bits), win) for s in S])
            for offset in (0, tc.SPLIT_OFFSET):
                got = ctx.hist_batch_via_device(padded, win, src_frame_bytes=padded.shape[1], src_offset=offset)
                for f in range(case.frames):
                    check(got[f], want[f], case.W, case.H, win)


@pytest.mark.parametrize("W,H,frames", list(tc.ROWS_CASES))
def test_rows_per_workgroup(gpu_pkg, W, H, frames):
    raws = tc.rows_frames(W, H, frames)
    with context(gpu_pkg, W, H) as ctx:
        got = ctx.hist_batch_via_device(raws)
    same(got, tc.histograms(raws))
    assert (got.sum(axis=2) == np.asarray(tc.window_counts(W, H, (0, 0, 0, 0)))).all()


def test_second_call_zeroes_the_fused_counts(gpu_pkg):
    family, c = tc.REPEAT_CASE
    raw = tc.fusion_frame(family, c.stride, c.H)
    want = hm.histogram(tc.samples(raw, c.W, c.H), 8, c.win)
    with context(gpu_pkg, c.W, c.H, stride=c.stride) as ctx:
        d_src, d_hist = ctx.device_alloc(raw.size), ctx.device_alloc(4096)
        try:
            ctx.to_device(d_src, raw)
            ctx.to_device(d_hist, np.full(4096, 0xA5, np.uint8))
            for _ in range(2):
                ctx.hist_device(d_src, d_hist, c.win)
            ctx.sync()
            check(ctx.from_device(d_hist, 4096).view(np.uint32).reshape(4, 256), want, c.W, c.H, c.win)
        finally:
            ctx.device_free(d_src)
            ctx.device_free(d_hist)


def test_host_path_slot_copy_sees_fused_counts(gpu_pkg):
    family, c = tc.HOST_CASE
    raw = tc.fusion_frame(family, c.stride, c.H)
    want = hm.histogram(tc.samples(raw, c.W, c.H), 8, c.win)
    with context(gpu_pkg, c.W, c.H) as ctx:
        assert ctx.src_stride == c.stride
        plain = ctx.process_host(raw).copy()
        ctx.set_hist(True, c.win)
        for _ in range(2):
            assert np.array_equal(ctx.process_host(raw), plain)
            check(ctx.frame_hist(), want, c.W, c.H, c.win)
