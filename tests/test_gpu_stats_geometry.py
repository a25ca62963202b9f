"""GPU tests of the launch geometry of mosaic_stats_kernel over the tables of tests/stats_cases.py: segment seams, the
frame x strip split of blockIdx.x, the top of the LDS table, zone seams on wave and workgroup seams, the ends of the
deep ranges and the identity of the four sites under 64-bit sums -- each through ONE mibayer_stats_device launch into a
junk-prefilled buffer, bit-exact against tests/stats_model.py.  What the tables reach is asserted, without a GPU, by
tests/test_stats_cases.py.  Two host-path tests change the grid while frames are in flight, in a ring and in a pool."""
import ctypes

import numpy as np
import pytest

import stats_cases as tc
import stats_model as sm
from test_gpu_stats import same

pytestmark = pytest.mark.gpu


def context(pkg, W, H, bits, big_endian=False, stride=0):
    if bits:
        return pkg.Context(W, H, "grbg", "ARGB64", src_stride=stride, device=0, bits=bits, src_big_endian=big_endian)
    return pkg.Context(W, H, "rggb", "RGBx", src_stride=stride, device=0)


@pytest.mark.parametrize("fmt", tc.SEG_FORMATS, ids=lambda f: "%dbit" % (f[1] or 8))
@pytest.mark.parametrize("H,zones_y", tc.SEG_CASES)
def test_segment_seams(gpu_pkg, H, zones_y, fmt):
    W, bits, big_endian = fmt
    raw = tc.seg_frame(fmt, H, zones_y)
    S = tc.samples(raw, W, H, bits, big_endian)
    with context(gpu_pkg, W, H, bits, big_endian, tc.SEG_STRIDE) as ctx:
        for lo, hi in tc.SEG_RANGES[bits]:
            same(ctx.stats_batch_via_device(raw[None], 1, zones_y, lo, hi)[0], sm.zone_stats(S, 1, zones_y, lo, hi))


@pytest.mark.parametrize("W,bits,frames", tc.BATCH_CASES)
def test_frame_and_strip_split(gpu_pkg, W, bits, frames):
    H = tc.BATCH_HEIGHT
    padded, raws = tc.batch_frames(W, bits, frames)
    lo, hi = tc.zone_range(bits)
    with context(gpu_pkg, W, H, bits) as ctx:
        for zx, zy in tc.BATCH_ZONES:
            want = np.stack([sm.zone_stats(tc.samples(r, W, H, bits), zx, zy, lo, hi) for r in raws])
            same(ctx.stats_batch_via_device(padded, zx, zy, lo, hi, src_frame_bytes=padded.shape[1]), want)


@pytest.mark.parametrize("W,H,bits,zones_x,zones_y", tc.ZONE_CASES)
def test_zone_table_and_zone_seams(gpu_pkg, W, H, bits, zones_x, zones_y):
    raw = tc.zone_frame(W, H, bits, zones_x, zones_y)
    lo, hi = tc.zone_range(bits)
    want = sm.zone_stats(tc.samples(raw, W, H, bits), zones_x, zones_y, lo, hi)
    with context(gpu_pkg, W, H, bits) as ctx:
        same(ctx.stats_batch_via_device(raw[None], zones_x, zones_y, lo, hi)[0], want)


@pytest.mark.parametrize("big_endian", (False, True), ids=("le", "be"))
@pytest.mark.parametrize("bits", tc.DEEP_BITS)
def test_deep_range_ends(gpu_pkg, bits, big_endian):
    W, H = tc.DEEP_SIZE
    with context(gpu_pkg, W, H, bits, big_endian) as ctx:
        for lo, hi in tc.deep_ranges(bits):
            raw = tc.deep_range_frame(bits, big_endian, lo, hi)
            want = sm.zone_stats(tc.samples(raw, W, H, bits, big_endian), *tc.DEEP_ZONES, lo, hi)
            same(ctx.stats_batch_via_device(raw[None], *tc.DEEP_ZONES, lo, hi)[0], want)


def test_sites_keep_their_identity_under_64_bit_sums(gpu_pkg):
    W, H = tc.SITE_SIZE
    raw = tc.site_frame()
    with gpu_pkg.Context(W, H, "bggr", "ARGB64", device=0, bits=16) as ctx:
        got = ctx.stats_batch_via_device(raw[None], 1, 1, 0, 65535)[0]
    same(got, sm.zone_stats(tc.samples(raw, W, H, 16), 1, 1, 0, 65535))
    assert got["sum"][0, 0].tolist() == [67600 * v for v in tc.SITE_PLANES]


# -- the grid of a frame is the one it was accepted with ------------------------------------------------------------

HOST_SIZE = (66, 70)            # the (1, 1) grid walks it in two segments
# what happens to frames 1 .. 6: a grid (zones_x, zones_y, lo, hi) for the frames accepted from then on, or a frame
HOST_SCRIPT = ((3, 2, 16, 239), 1, 2, (1, 1, 0, 255), 3, 4, (0, 0, 0, 0), 5, (2, 2, 8, 247), 6)
COUNTS = (1, 2, 4, 6, 7)        # the zone counts every answer is asked with


def run_script(pkg, pipe, frame_stats, capacity):
    """HOST_SCRIPT on a context or a pool: as many frames in flight as `capacity` allows, and after every wait() the
    answers of mibayer_frame_stats / mibayer_pool_frame_stats to every count of COUNTS"""
    W, H = HOST_SIZE
    assert tc.geometry(W, H, 0, 1, 1).segs == 2
    rng = np.random.default_rng(70)
    raws = {i: tc.random_frame(rng, W, H, 0) for i in range(1, 7)}
    dsts = {i: np.zeros((H, 4 * W), np.uint8) for i in raws}
    grids, grid, done = {}, None, []

    def collect():
        tag = pipe.wait()
        assert tag == len(done) + 1             # in submission order
        g = grids[tag]
        n = g[0] * g[1]
        for count in COUNTS:
            out = np.zeros(count, sm.STATS_DTYPE)
            rc = frame_stats(pipe._h, ctypes.c_void_p(out.ctypes.data), count)
            if n == 0:
                assert rc == pkg.ERR_EMPTY, (tag, count)
            elif count != n:
                assert rc == pkg.ERR_ARG, (tag, count)
            else:
                assert rc == pkg.OK, (tag, count)
                same(out.reshape(g[1], g[0]), sm.zone_stats(tc.samples(raws[tag], W, H, 0), *g))
        done.append(tag)

    for step in HOST_SCRIPT:
        if isinstance(step, tuple):
            grid = step
            pipe.set_stats(*grid)
            continue
        if pipe.pending() == capacity:
            collect()
        grids[step] = grid
        pipe.submit(raws[step].reshape(-1), dsts[step], tag=step)
    assert pipe.pending() >= 2                  # the grid did change under frames in flight
    while pipe.pending():
        collect()
    assert done == [1, 2, 3, 4, 5, 6] and {g[0] * g[1] for g in grids.values()} == {6, 1, 0, 4} < set(COUNTS) | {0}
    return raws, dsts


def test_ring_keeps_the_grid_each_frame_was_accepted_with(gpu_pkg):
    W, H = HOST_SIZE
    with gpu_pkg.Context(W, H, device=0, inflight=3) as ctx:
        raws, dsts = run_script(gpu_pkg, ctx, gpu_pkg.lib().mibayer_frame_stats, 3)
    with gpu_pkg.Context(W, H, device=0) as plain:
        for i, raw in raws.items():
            assert np.array_equal(dsts[i], plain.process_host(raw)), i    # the converted bytes do not change


def test_pool_keeps_the_grid_each_frame_was_accepted_with(gpu_pkg):
    W, H = HOST_SIZE
    with gpu_pkg.Pool([0, 0], W, H, inflight=2) as pool:
        raws, dsts = run_script(gpu_pkg, pool, gpu_pkg.lib().mibayer_pool_frame_stats, pool.capacity)
    with gpu_pkg.Context(W, H, device=0) as plain:
        for i, raw in raws.items():
            assert np.array_equal(dsts[i], plain.process_host(raw)), i
