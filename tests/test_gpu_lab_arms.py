"""GPU tests of the tile kernels that only the lab build has (`make lab`, csrc/mibayer_kernels.hip: variant ids 10 and
up -- bayer2rgb_direct_kernel, bayer2rgb_persist_kernel and the bayer2rgb_lds_kernel arms with other neighbour
exchanges, store and load policies and tile shapes).  The product build's suite cannot reach them: every name that is
not a production name runs here, bit-exact against the CPU oracle, at one geometry of its fast arm and one of its
generic arm, each as a batch of two frames inside a guarded allocation; the persistent arms also with workgroups that
walk several tiles, under both of their block orders."""
import numpy as np
import pytest

import tile_cases as tc
from test_gpu_tile_geometry import convert, problems

pytestmark = pytest.mark.gpu

ORDER_LAYOUT = (("rggb", "BGRx"), ("gbrg", "xRGB"))     # swap_rows 0 and 1


def lab_only_names(pkg):
    return [n for n in pkg.variant_names()[1:] if n not in tc.PRODUCTION_NAMES]


def tile_of(pkg, vid):
    """(tile_w, tile_h) as mibayer_launch_geometry reports them for the variant"""
    with pkg.Context(64, 8, "rggb", "BGRx", variant=vid, device=0) as ctx:
        geo = ctx.launch_geometry(1)
    return geo["tile_w"], geo["tile_h"]


def frames_and_wanted(oracle, pkg, w, h, n, order, layout, seed):
    rng = np.random.default_rng([seed, w, h, n])
    src = rng.integers(0, 256, (n, h, (w + 3) & ~3), dtype=np.uint8)
    r, g, b = pkg.FORMATS[layout]
    return src, np.stack([oracle.bayer2rgb(f, w, order, r, g, b) for f in src])


def test_the_lab_build_has_arms_beyond_the_production_names(lab_pkg):
    names = lab_only_names(lab_pkg)
    assert len(names) >= 15 and len(set(names)) == len(names)
    for stem in ("persist_", "direct_", "_shfl_", "_ldsnb_", "_swar", "_ldnt", "_glds", "_sc1"):
        assert any(stem in n for n in names), stem
    assert sum(n.startswith("persist_") for n in names) == 2


def test_every_lab_arm_fast_and_generic(gpu_lab_pkg, oracle):
    """(tile_w + 16) x (tile_h + 3): the fast arm, one tile seam, a last tile of 16 px and a last tile row of 3 rows (one
    wave stores 3 of its rows, the waves below it none).  (tile_w + 10) x (tile_h + 3): the generic arm, the staging
    tail of 12 readable bytes and the two-pixel last lane.  Two frames each: a tile row that follows a frame seam"""
    pkg = gpu_lab_pkg
    n = 2
    bad = []
    for name in lab_only_names(pkg):
        vid = tc.variant_id(pkg, name)
        tw, th = tile_of(pkg, vid)
        for arm, w in (("fast", tw + 16), ("generic", tw + 10)):
            h = th + 3
            assert tc.expected_arm(tc.make_launch(w, h, nframes=n)) == arm
            if arm == "generic":
                assert tc.tail_chunk(w, tw) == (1, 0, 12) and w % 4 == 2
            for order, layout in ORDER_LAYOUT:
                src, want = frames_and_wanted(oracle, pkg, w, h, n, order, layout, 11)
                with pkg.Context(w, h, order, layout, variant=vid, device=0) as ctx:
                    geo = ctx.launch_geometry(n)
                    assert (geo["tile_w"], geo["tile_h"], geo["tiles_x"], geo["tile_rows"]) == (tw, th, 2, 2 * n)
                    body, wrong, _ = convert(ctx, src)
                    for p in problems(ctx, body, wrong, want):
                        bad.append("%s %dx%d x %d %s %s (%s): %s" % (name, w, h, n, order, layout, arm, p))
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("block_order", ["chunk", "identity"])
@pytest.mark.parametrize("name", ["persist_4x2_r4_nt", "persist_1x8_r4_nt"])
def test_persistent_arm_walks_several_tiles(gpu_lab_pkg, oracle, monkeypatch, name, block_order):
    """one workgroup per CU, frames of 3 tile rows x 2 tiles, and enough of them that EVERY workgroup converts at least
    two tiles: the loop of bayer2rgb_persist_kernel (loads of tile n + 1 in flight across tile n), under the variant's
    own chunk-per-XCD order and under the identity order"""
    pkg = gpu_lab_pkg
    monkeypatch.setenv("MIBAYER_PERSIST_WGS", "1")
    vid = tc.variant_id(pkg, name)
    tw, th = tile_of(pkg, vid)
    w, h = tw + 16, 2 * th + 3
    per_frame = 6

    def plan(ctx):
        if block_order == "identity":
            ctx.set_plan(vid, 0, 0)
            assert ctx.get_plan() == (vid, 0, 0)

    # the smallest batch at which the condition below holds (the grid follows the CU count)
    with pkg.Context(w, h, "rggb", "BGRx", variant=vid, device=0) as ctx:
        plan(ctx)
        grid = ctx.launch_geometry(1024)["grid_blocks"]
    n = -(-2 * grid // per_frame)
    while True:
        rows = 3 * n
        band = -(-rows // tc.NUM_XCD)
        if min(band, rows - (tc.NUM_XCD - 1) * band) * 2 >= 2 * grid // tc.NUM_XCD:
            break
        n += 1
    assert n <= 256, (grid, n)

    bad = []
    for order, layout in ORDER_LAYOUT:
        src, want = frames_and_wanted(oracle, pkg, w, h, n, order, layout, 12)
        assert tc.expected_arm(tc.make_launch(w, h, nframes=n)) == "fast"
        with pkg.Context(w, h, order, layout, variant=vid, device=0) as ctx:
            plan(ctx)
            geo = ctx.launch_geometry(n)
            assert (geo["tile_w"], geo["tile_h"], geo["tiles_x"], geo["tile_rows"]) == (tw, th, 2, 3 * n)
            assert geo["grid_blocks"] == grid and grid % tc.NUM_XCD == 0
            tiles = geo["tile_rows"] * geo["tiles_x"]
            if block_order == "identity":
                assert geo["band"] == 0
                assert tiles >= 2 * grid                # block b walks b, b + grid, ...
            else:
                # XCD k walks tile rows [k band, (k + 1) band) with grid / 8 workgroups; the last chunk is the short one
                assert geo["band"] == -(-geo["tile_rows"] // tc.NUM_XCD) > 0
                chunk_rows = min(geo["band"], geo["tile_rows"] - (tc.NUM_XCD - 1) * geo["band"])
                assert chunk_rows * geo["tiles_x"] >= 2 * grid // tc.NUM_XCD
            body, wrong, _ = convert(ctx, src)
            for p in problems(ctx, body, wrong, want):
                bad.append("%s %dx%d x %d %s %s, %s order, %d workgroups: %s" % (name, w, h, n, order, layout, block_order,
                                                                                 grid, p))
    assert not bad, "\n".join(bad)
