"""The case tables of tests/tile_cases.py reach what they are meant to reach -- asserted from the tables alone (and, for
the block orders, from the library's host arithmetic), so that the GPU tests built on them
(tests/test_gpu_tile_geometry.py) cannot go vacuous when a table is edited."""
import pytest

import tile_cases as tc

SHAPE_IDS = [s.stem for s in tc.SHAPES]


# -- the tables ------------------------------------------------------------------------------------------------------

def test_names_are_the_librarys(pkg):
    names = pkg.variant_names()
    assert names[1:10] == list(tc.PRODUCTION_NAMES)
    assert set(tc.ALL_FORMATS) == set(pkg.FORMATS) and len(tc.ALL_FORMATS) == 8
    assert [(s.tile_w, s.tile_h) for s in tc.SHAPES] == [(1024, 8), (512, 16), (256, 32)]
    assert all(s.tile_w % tc.WAVE_PX == 0 and s.tile_h % tc.ROWS_PER_WAVE == 0 for s in tc.SHAPES)
    assert len(set(tc.ARM128_NAMES)) == 6 and not set(tc.ARM128_NAMES) & set(tc.HY_NAMES)
    for name in tc.PRODUCTION_NAMES:
        assert tc.shape_of(name).stem in name


def test_the_issues_minimum_is_in_the_tables():
    assert set(tc.WIDTHS) >= {20, 22, 24, 26, 28, 30, 32, 34, 254, 256, 258, 260, 262, 266, 510, 512, 514, 516, 518,
                              522, 1022, 1024, 1026, 1028, 1030, 1034, 1040, 2050}
    assert set(tc.HEIGHTS) >= {3, 4, 5, 6, 7, 8, 9, 10, 11, 12, 15, 16, 17, 18, 19, 20, 31, 32, 33, 34, 35, 36, 63, 64,
                               65, 67}
    assert tc.SWEEP_HEIGHT == 35 and tc.HEIGHT_WIDTHS == (262, 1028)
    assert all(w % 2 == 0 and w >= 4 for w in tc.WIDTHS) and all(h >= 3 for h in tc.HEIGHTS)


# -- widths ----------------------------------------------------------------------------------------------------------

def test_widths_cover_every_residue_inside_one_wave():
    assert {w % 16 for w in tc.WIDTHS if w <= tc.WAVE_PX - 8} == set(range(0, 16, 2))


@pytest.mark.parametrize("shape", tc.SHAPES, ids=SHAPE_IDS)
def test_widths_put_the_last_group_on_both_sides_of_every_seam(shape):
    ends = [tc.tile_position(w, shape.tile_w) for w in tc.WIDTHS]
    per_tile = shape.tile_w // tc.WAVE_PX
    # the tile seam: lane 63 of the last wave of tile 0, lanes 0, 1, 2 of the first wave of tile 1
    seam = {(e["tile"], e["wave"], e["lane"], e["full"]) for e in ends}
    for full in (False, True):
        assert (0, per_tile - 1, 63, full) in seam
        assert (1, 0, 0, full) in seam
    assert (1, 0, 1, False) in seam and (1, 0, 2, False) in seam
    # the wave seam inside a tile (shapes of more than one wave per row)
    if per_tile > 1:
        for full in (False, True):
            assert (0, 0, 63, full) in seam and (0, 1, 0, full) in seam
        assert (0, 1, 1, False) in seam
    # the sweep's widths in the terms of the issue: TW - 2, TW, TW + 2, TW + 4, TW + 6, TW + 10
    tw = shape.tile_w
    assert {tw - 2, tw, tw + 2, tw + 4, tw + 6, tw + 10} <= set(tc.WIDTHS)
    assert {tw - 2, tw, tw + 2, tw + 4, tw + 6, tw + 10} <= set(tc.weakest_widths(shape))
    assert {32, 256, 512, 1024} <= set(tc.weakest_widths(shape))


@pytest.mark.parametrize("shape", tc.SHAPES, ids=SHAPE_IDS)
def test_widths_cover_the_staging_tail(shape):
    tails = [tc.tail_chunk(w, shape.tile_w) for w in tc.WIDTHS]
    assert {a for _, _, a in tails} == {4, 8, 12, 16}
    # ... inside one tile, and 8 and 12 again in the FIRST chunk behind a tile seam
    assert {a for t, _, a in tails if t == 0} == {4, 8, 12, 16}
    behind = {a for t, c, a in tails if t == 1 and c == 0}
    assert {4, 8, 12} <= behind
    # a width whose tail chunk is 12 bytes, at the seam of THIS shape (522 for the 512-px tiles)
    assert shape.tile_w + 10 in tc.WIDTHS and tc.tail_chunk(shape.tile_w + 10, shape.tile_w) == (1, 0, 12)


@pytest.mark.parametrize("shape", tc.SHAPES, ids=SHAPE_IDS)
def test_widths_cover_the_halo_bound(shape):
    tw = shape.tile_w
    assert tw in tc.WIDTHS and not tc.right_halo_readable(tw, tw)               # right halo past wlimit4
    assert tw - 2 in tc.WIDTHS and not tc.right_halo_readable(tw - 2, tw)
    for w in (tw + 2, tw + 4):  # readable, and the LAST readable dword: col + 4 == wlimit4
        assert w in tc.WIDTHS and tc.right_halo_readable(w, tw) and tw + 4 == tc.wlimit4(w)
    assert tc.right_halo_readable(tw + 6, tw) and tw + 4 < tc.wlimit4(tw + 6)   # ... and one that is not the last
    # three tiles and a tail: a tile with a readable halo on BOTH sides
    wide = max(tc.WIDTHS)
    assert wide > 2 * tw and tc.right_halo_readable(wide, tw, 1)


def test_width_sweep_takes_the_fast_and_the_generic_arm():
    cases = tc.width_cases()
    assert [c.w for c in cases] == list(tc.WIDTHS) and {c.h for c in cases} == {tc.SWEEP_HEIGHT}
    # padded strides: generic whatever the width; the widths of 0 mod 16 once more with unpadded strides: fast
    assert {tc.expected_arm(tc.sweep_launch(c)) for c in cases} == {"generic"}
    fast = tc.fast_width_cases()
    assert [c.w for c in fast] == [32, 256, 512, 1024, 1040] and {c.h for c in fast} == {tc.SWEEP_HEIGHT}
    assert {tc.expected_arm(tc.sweep_launch(c, padded=False)) for c in fast} == {"fast"}
    assert {tc.expected_arm(tc.sweep_launch(c, padded=False)) for c in cases if c.w % 16} == {"generic"}
    # ... a second tile of 16 px (one chunk) behind a full one, and W == TW for every shape
    assert all(1040 % s.tile_w == 16 and s.tile_w in [c.w for c in fast] for s in tc.SHAPES)
    # the value extremes and the batches run the fast arm at widths of 0 mod 16, the generic one elsewhere
    assert tc.expected_arm(tc.make_launch(*tc.EXTREME_FAST, nframes=16)) == "fast"
    assert tc.expected_arm(tc.make_launch(*tc.EXTREME_GENERIC, nframes=16)) == "generic"
    w, h = tc.EXTREME_GENERIC
    assert tc.expected_arm(tc.make_launch(w, h, dst_stride=4 * w + tc.EXTREME_ALIGNED_PAD, nframes=16,
                                          align=128)) == "aligned128"
    assert tc.expected_arm(tc.make_launch(w, h, dst_stride=4 * w + tc.EXTREME_ALIGNED_PAD, nframes=16, align=128,
                                          has_arm=False)) == "generic"
    for pw, ph, n, _, _ in tc.PLAN_CASES:
        assert pw % 16 and tc.expected_arm(tc.make_launch(pw, ph, tc.src_stride_of(pw), 4 * pw + 24, nframes=n,
                                                          dst_gap=4)) == "generic"
        fw = tc.fast_width(pw)
        assert fw % 16 == 0 and tc.expected_arm(tc.make_launch(fw, ph, nframes=n)) == "fast"
        for s in tc.SHAPES:     # the same tile grid as the generic run
            assert -(-fw // s.tile_w) == -(-pw // s.tile_w)


@pytest.mark.parametrize("shape", tc.SHAPES, ids=SHAPE_IDS)
def test_weakest_base_pointers_take_the_generic_arm_at_fast_widths(shape):
    widths = tc.weakest_widths(shape)
    cases = [tc.rotate(i, w, tc.SWEEP_HEIGHT) for i, w in enumerate(widths)]
    assert {tc.expected_arm(tc.sweep_launch(c, weakest=True)) for c in cases} == {"generic"}
    fast_widths = [c for c in cases if c.w % 16 == 0]
    assert len(fast_widths) >= 4
    for c in fast_widths:       # the base pointers alone do it: with unpadded strides too
        L = tc.make_launch(c.w, c.h, src_mod=4, dst_mod=4)
        assert tc.expected_arm(L) == "generic" and tc.expected_arm(L._replace(src_mod=0, dst_mod=0)) == "fast"


def test_sweeps_see_every_order_and_layout():
    for k in range(len(tc.PRODUCTION_NAMES)):
        for cases in (tc.width_cases(k), tc.height_cases(k)):
            assert {c.order for c in cases} == set(tc.ORDERS)
            assert {c.layout for c in cases} == set(tc.ALL_FORMATS)
            assert len({(c.order, c.layout) for c in cases}) >= 24
    assert len({(c.order, c.layout) for c in (tc.rotate(i, 4, 3) for i in range(32))}) == 32
    # the variants do not all meet a width under the same order and layout
    for i, w in enumerate(tc.WIDTHS):
        assert len({(tc.width_cases(k)[i].order, tc.width_cases(k)[i].layout)
                    for k in range(len(tc.PRODUCTION_NAMES))}) >= 4, w


# -- heights ---------------------------------------------------------------------------------------------------------

def test_heights_cover_dn_last_and_the_three_row_frame():
    assert {tc.dn_last(h) for h in tc.HEIGHTS if 4 <= h <= 7} == {0, 1, 2, 3}
    assert 3 in tc.HEIGHTS and tc.dn_last(3) == 1
    assert {h % 2 for h in tc.HEIGHTS} == {0, 1}
    cases = tc.height_cases()
    for w in tc.HEIGHT_WIDTHS:
        assert [c.h for c in cases if c.w == w] == list(tc.HEIGHTS)
    # 262: two tiles per row for the 256-px tiles and one for the others; 1028: a tile seam for every shape
    assert [-(-262 // s.tile_w) for s in tc.SHAPES] == [1, 1, 2]
    assert all(-(-1028 // s.tile_w) >= 2 for s in tc.SHAPES)
    for c in cases:
        assert tc.expected_arm(tc.height_launch(c, 0)) == "generic"
        assert tc.expected_arm(tc.height_launch(c, 128)) == "aligned128"


@pytest.mark.parametrize("shape", tc.SHAPES, ids=SHAPE_IDS)
def test_heights_cover_the_last_tile_row(shape):
    th = shape.tile_h
    assert {h % th for h in tc.HEIGHTS} >= {0, 1, 2, 3, th - 1}
    # dn (H-1) = row H-4 lies in the tile row ABOVE the last one when H % tile_h is 1, 2 or 3 (and H > tile_h)
    for r in (1, 2, 3):
        hs = [h for h in tc.HEIGHTS if h % th == r and h > th]
        assert hs, r
        for h in hs:
            assert tc.dn_last(h) // th == (h - 1) // th - 1
    assert any(h % th == 0 and tc.dn_last(h) // th == (h - 1) // th for h in tc.HEIGHTS)
    # the sweep height: more than one tile row, the last of 3 rows
    assert tc.SWEEP_HEIGHT > th and tc.SWEEP_HEIGHT % th == 3
    # waves of the last tile row: without a row inside the frame, with 1, 2 and 3 rows, and with all 4
    seen = set()
    for h in tc.HEIGHTS:
        seen |= set(tc.wave_nrows(h, th))
    assert any(n <= 0 for n in seen) and {1, 2, 3, 4} <= seen
    assert any(n <= 0 for n in tc.wave_nrows(tc.SWEEP_HEIGHT, th)) and 3 in tc.wave_nrows(tc.SWEEP_HEIGHT, th)


# -- the aligned arm -------------------------------------------------------------------------------------------------

ALL_SHIFTS = set(range(0, 32, 2))


def test_aligned_cases_are_well_formed_and_take_the_arm():
    assert len(set(tc.ALIGNED_CASES)) == len(tc.ALIGNED_CASES)
    for row in tc.ALIGNED_CASES:
        w, h, pad, off, n, gap = row
        assert w % 2 == 0 and w >= 4 and h >= 3 and pad % 8 == 0 and off % 8 == 0 and gap % 8 == 0 and 1 <= n <= 4, row
        assert tc.expected_arm(tc.aligned_launch(row)) == "aligned128", row
        if n > 1:
            assert tc.expected_arm(tc.aligned_launch(row, as_list=True)) == "aligned128", row
        assert all(a % 8 == 0 for _, _, a in tc.row_addresses(row)), row
    # ... and would not without the padding: on the grid the arm is NOT taken
    assert tc.expected_arm(tc.aligned_launch((32, 18, 0, 0, 1, 0))) == "generic"
    assert tc.expected_arm(tc.aligned_launch((30, 17, 8, 0, 1, 0))) == "generic"
    assert tc.expected_arm(tc.aligned_launch((288, 6, 0, 0, 1, 0))) == "generic"


@pytest.mark.parametrize("parity", [2, 0], ids=["width%4==2", "width%4==0"])
def test_aligned_cases_see_all_16_shifts(parity):
    rows = [r for r in tc.ALIGNED_CASES if r[0] % 4 == parity]
    union = set()
    for r in rows:
        union |= tc.row_shifts(r)
    assert union == ALL_SHIFTS
    # ... in one frame, too: a single case that walks through all of them
    assert any(tc.row_shifts(r) == ALL_SHIFTS for r in rows)
    # ... and for every shape across a tile seam of its own
    for s in tc.SHAPES:
        union = set()
        for r in rows:
            if s.tile_w < r[0] <= s.tile_w + 30:
                union |= tc.row_shifts(r)
        assert union == ALL_SHIFTS, s


def test_aligned_cases_narrow_frames_batches_and_the_constant_shift():
    by_width = {r[0]: r for r in tc.ALIGNED_CASES}
    assert {4, 6, 14, 30, 32, 34} <= set(by_width)
    # the head (columns 0 .. s-1) is longer than, as long as and shorter than the row
    heads = set()
    for w in (4, 6, 14, 30):
        heads |= {(s > w) - (s < w) for s in tc.row_shifts(by_width[w]) if s}
    assert heads == {-1, 0, 1}
    # on the grid but for the offset: one shift for the whole frame
    assert tc.row_shifts(by_width[288]) == {30} and by_width[288][2] == 0 and by_width[288][3] == 8
    assert 4 * 288 % 128 == 0
    # batches of 2 to 4 frames whose pitch moves the phase from frame to frame
    batches = [r for r in tc.ALIGNED_CASES if r[4] > 1]
    assert {r[4] for r in batches} == {2, 3, 4} and all(r[5] == 8 for r in batches)
    for r in batches:
        first = {f: a for f, j, a in tc.row_addresses(r) if j == 0}
        assert len(set(first.values())) == len(first), r
    # 1028 without padding would see the multiples of 4 only
    assert tc.row_shifts((1028, 17, 0, 0, 1, 0)) == set(range(0, 32, 4))
    assert tc.row_shifts(by_width[1028]) == ALL_SHIFTS
    assert set(tc.ALIGNED_BANDS) == {0, 1, -1}


def test_aligned_cases_hit_the_edge_wave_test_on_both_sides():
    sides = set()
    for r in tc.ALIGNED_CASES:
        sides |= tc.edge_wave_sides(r)
    want = {(p, s) for p in ("first", "middle", "last") for s in ("below", "equal", "above")} - {("last", "below")}
    assert sides == want
    # wave_x + 256 == width (the one value `<` and `<=` part on) at the seam of every shape: first wave of a row
    # (256 + s) and a later one (512 + s, 1024 + s)
    for w in (258, 262, 286, 514, 518, 542, 1026, 1030):
        rows = [r for r in tc.ALIGNED_CASES if r[0] == w]
        assert any(s == "equal" for r in rows for _, s in tc.edge_wave_sides(r)), w
    # and the height sweep under the arm (pitch 4 w + 8) meets both sides as well
    for w in tc.HEIGHT_WIDTHS:
        got = {s for _, s in tc.edge_wave_sides((w, 67, 8, 0, 1, 0))}
        assert {"below", "above"} <= got or w < 512


# -- block orders ----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case", tc.PLAN_CASES, ids=lambda c: "%dx%dx%d-%s-band%d" % c)
def test_plan_cases_idle_blocks_and_mixed_bands(pkg, case):
    """mibayer_block_to_tile is the kernels' own map, pure host arithmetic"""
    w, h, n, name, band = case
    L = pkg.lib()
    tiles_x, tile_rows, eff, grid = tc.plan_geometry(*case)
    tiles_y = tile_rows // n
    tiles = [L.mibayer_block_to_tile(b, tiles_x, tile_rows, eff) for b in range(grid)]
    live = [t for t in tiles if t >= 0]
    # every tile exactly once, whatever the order
    assert sorted(live) == list(range(tiles_x * tile_rows))
    assert L.mibayer_block_to_tile(grid, tiles_x, tile_rows, eff) == -1
    if band == 0:
        assert eff == 0 and live == tiles       # the identity order has no block to spare
        return
    assert tile_rows % (tc.NUM_XCD * eff) != 0
    assert len(live) < len(tiles)               # trailing blocks idle
    frames_of = {}              # (xcd, band index of that XCD) -> frames of its tile rows
    for b, t in enumerate(tiles):
        if t >= 0:
            key = (b % tc.NUM_XCD, (b // tc.NUM_XCD) // (eff * tiles_x))
            frames_of.setdefault(key, set()).add((t // tiles_x) // tiles_y)
    if eff >= 2:                # one XCD's band holds tile rows of two frames
        assert any(len(f) >= 2 for f in frames_of.values())
    else:                       # a band of one tile row cannot: there one XCD walks tile rows of two frames
        per_xcd = {}
        for (xcd, _), f in frames_of.items():
            per_xcd.setdefault(xcd, set()).update(f)
        assert any(len(f) >= 2 for f in per_xcd.values())


def test_plan_cases_cover_every_band_and_name():
    assert {c[4] for c in tc.PLAN_CASES} == {0, 1, 3, -1}
    assert {c[3] for c in tc.PLAN_CASES} == set(tc.PRODUCTION_NAMES)
    assert {(c[0], c[1], c[2]) for c in tc.PLAN_CASES} >= {(1028, 19, 3), (262, 35, 5)}
    assert all(c[2] <= tc.MAX_LIST for c in tc.PLAN_CASES)
    for s in tc.SHAPES:         # every shape under a band map of more than one tile row
        assert any(tc.shape_of(c[3]) == s and tc.plan_geometry(*c)[2] >= 2 for c in tc.PLAN_CASES)
