"""What the tables of tests/band_cases.py reach, asserted without a GPU and without the library -- so that a later edit
of the heights cannot quietly lose a branch of the band cut (choose_host_bands / enqueue_frame_banded,
csrc/mibayer_abi.hip) that tests/test_gpu_band_seams.py is meant to run."""
import numpy as np
import pytest

import band_cases as bc
import colour_model as cm
import highbit_model as hm
import mhc_model as mm
import r2b_cases as rc
import strip_cases as sc
import tile_cases as tc

BIG = bc.BAND_MIN_BYTES
WANTS = tuple(bc.wanted(e) for e in bc.LAB_WANTS)       # 4, 2, 3, 8


def cuts(unit):
    """{(h, want): bands} over the table heights of a unit and every wanted count"""
    return {(h, want): bc.host_bands(want, BIG, h, unit) for h in bc.HEIGHTS[unit] for want in WANTS}


def lengths(nb, h, unit):
    return [y1 - y0 for y0, y1 in bc.band_rows(nb, h, unit)]


# -- the rule -----------------------------------------------------------------------------------------------------------

def test_the_rule_by_hand_at_unit_16():
    """choose_host_bands at the strip kernels' unit and the product's 4 wanted bands, worked out by hand: the cut is no
    smooth function of the height"""
    got = {h: bc.host_bands(4, BIG, h, 16) for h in (19, 20, 33, 36, 49, 51, 52, 68, 100, 116)}
    assert got == {19: 1, 20: 2, 33: 1, 36: 3, 49: 2, 51: 2, 52: 4, 68: 3, 100: 4, 116: 4}
    assert lengths(2, 20, 16) == [16, 4] and lengths(3, 36, 16) == [16, 16, 4] and lengths(4, 52, 16) == [16, 16, 16, 4]
    assert lengths(2, 49, 16) == [32, 17] and lengths(2, 51, 16) == [32, 19]
    assert lengths(3, 68, 16) == [32, 32, 4] and lengths(4, 100, 16) == [32, 32, 32, 4]
    assert bc.host_bands(8, BIG, 116, 16) == 8
    # clamps and the reasons for one band
    assert bc.host_bands(99, BIG, 116, 16) == 8 and bc.MAX_BANDS == 8
    assert bc.host_bands(1, BIG, 116, 16) == bc.host_bands(0, BIG, 116, 16) == bc.host_bands(-3, BIG, 116, 16) == 1
    assert bc.host_bands(4, BIG, 116, 16, persistent=True) == 1
    assert bc.host_bands(4, BIG - 1, 116, 16) == 1 and bc.host_bands(4, BIG, 116, 16) == 4


def test_bands_tile_the_frame():
    """whatever the cut: the bands are whole units, none is empty, and they cover every row once, in order"""
    for unit in bc.UNITS:
        for (h, want), nb in cuts(unit).items():
            rows = bc.band_rows(nb, h, unit)
            assert len(rows) == nb and rows[0][0] == 0 and rows[-1][1] == h, (unit, h, want)
            assert all(a[1] == b[0] for a, b in zip(rows, rows[1:])) and all(y1 > y0 for y0, y1 in rows)
            assert all(y0 % unit == 0 for y0, _ in rows)
            if nb > 1:
                assert h - rows[-1][0] >= bc.MIN_LAST_ROWS and rows[0][1] >= bc.MIN_BAND_ROWS
            for halo in (1, 2):
                up = bc.uploaded_rows(nb, h, unit, halo)
                assert up == sorted(up) and up[-1] == h
                assert all(u == min(y1 + halo, h) for u, (_, y1) in zip(up, rows))


@pytest.mark.parametrize("unit", bc.UNITS)
def test_every_band_count_occurs(unit):
    got = set(cuts(unit).values())
    assert got == set(range(1, 9)), (unit, sorted(got))


@pytest.mark.parametrize("unit", bc.UNITS)
def test_the_last_band_of_exactly_four_rows_and_the_height_below_it(unit):
    """h = k unit + 4 in k + 1 bands: the last band is the 4 rows the bottom rule needs.  One row less and the same wanted
    count falls back to fewer bands, whose last band holds a full unit and a short one"""
    hs = bc.HEIGHTS[unit]
    four = [(h, want) for (h, want), nb in cuts(unit).items() if nb == want and lengths(nb, h, unit)[-1] == 4]
    assert four, unit
    pairs = [(h, want) for h, want in four if h - 1 in hs and bc.host_bands(want, BIG, h - 1, unit) < want]
    assert pairs, (unit, four)
    if unit == 16:
        assert (52, 4) in pairs and bc.host_bands(4, BIG, 51, 16) == 2
    for h, want in pairs:
        nb = bc.host_bands(want, BIG, h - 1, unit)
        last = lengths(nb, h - 1, unit)[-1]
        assert last > unit and last % unit == 3, (unit, h, want, last)     # a full unit and a short one of 3 rows


@pytest.mark.parametrize("unit", bc.UNITS)
def test_a_height_where_every_count_is_rejected(unit):
    """two units, the second of fewer than 4 rows: no cut of 4, 3 or 2 bands holds, though the frame is big enough"""
    h = {4: 11, 8: 11, 16: 33, 32: 35}[unit]
    assert h in bc.HEIGHTS[unit]
    assert [bc.host_bands(want, BIG, h, unit) for want in (8, 4, 3, 2)] == [1, 1, 1, 1]
    # ... by the last-band rule: a third unit of 4 rows and the frame is cut again
    assert bc.host_bands(4, BIG, 2 * unit + 4, unit) > 1 and 2 * unit + 4 in bc.HEIGHTS[unit]


@pytest.mark.parametrize("unit", bc.UNITS)
def test_bands_of_one_unit_and_of_several(unit):
    one = several = mixed = False
    for (h, want), nb in cuts(unit).items():
        if nb == 1:
            continue
        n = [-(-length // unit) for length in lengths(nb, h, unit)]
        one |= n[0] == 1
        several |= n[0] > 1
        mixed |= n[0] > n[-1] >= 1 and n[0] > 1                             # the last band shorter, in units, too
    # at unit 4 a band of one unit is what per * unit >= 8 refuses
    assert one == (unit >= bc.MIN_BAND_ROWS) and several and mixed, unit


def test_the_minimum_band_height_bites_at_unit_4_only():
    """unit 4, height 8: two bands of one unit would be 4 rows each -- refused by per * unit >= 8, and by nothing else"""
    assert 8 in bc.HEIGHTS[4]
    assert bc.host_bands(4, BIG, 8, 4) == 1 and [bc.host_bands(w, BIG, 8, 4) for w in (2, 3, 8)] == [1, 1, 1]
    units, per = 2, 1
    assert -(-units // per) == 2 and 8 - per * 4 >= bc.MIN_LAST_ROWS and per * 4 < bc.MIN_BAND_ROWS
    for unit in (8, 16, 32):
        assert unit >= bc.MIN_BAND_ROWS                 # a band of one unit always passes
    assert bc.host_bands(4, BIG, 12, 4) == 2 and lengths(2, 12, 4) == [8, 4]            # per = 2: bands of 8 rows pass


def test_the_threshold_from_both_sides():
    """banded_stride gives the first stride of its residue at which the frame is banded"""
    for fam in bc.LAB_FAMILIES:
        for case in bc.product_cases(fam):
            sstride, dstride = bc.strides(fam, case.w, case.h)
            p = bc.planes(fam)
            fast = fam.kind == "tile" and case.w % 16 == 0
            assert dstride % 16 == (0 if fast else 8)
            assert sstride == bc.src_row_bytes(fam, case.w) + (0 if fast else 12) and sstride % (16 if fast else 4) == 0
            assert dstride >= bc.row_bytes(fam, case.w) and dstride % (8 if bc.pixel_bytes(fam) == 8 else 4) == 0
            assert p * dstride * case.h >= BIG > p * (dstride - 16) * case.h, (fam.name, case)
            above = bc.host_bands(4, p * dstride * case.h, case.h, fam.unit, fam.persistent)
            below = bc.host_bands(4, p * (dstride - 16) * case.h, case.h, fam.unit, fam.persistent)
            assert below == 1 and above == bc.expected_bands(fam, case)
            if not fam.persistent and bc.host_bands(4, BIG, case.h, fam.unit) > 1:
                assert above > 1
    assert bc.banded_stride(1064, 52) == 322640 and 322640 * 52 >= BIG > 322624 * 52
    assert bc.banded_stride(1064, 52, 3, 16, 8) == 107560 and bc.banded_stride(20 << 20, 52, 1, 16, 8) == (20 << 20) + 8


# -- the tables -----------------------------------------------------------------------------------------------------------

def test_families_and_their_units():
    assert [f.arm for f in bc.STRIP_FAMILIES] == list(sc.ARMS) and len(bc.STRIP_FAMILIES) == 15
    assert len(bc.RGB24_FAMILIES) == len(bc.PLANAR_FAMILIES) == 6
    assert [f.name for f in bc.TILE_FAMILIES] == list(tc.PRODUCTION_NAMES) and len(bc.TILE_FAMILIES) == 9
    assert {f.unit for f in bc.STRIP_FAMILIES + bc.RGB24_FAMILIES + bc.PLANAR_FAMILIES} == {sc.STRIP_ROWS} == {16}
    assert [f.unit for f in bc.TILE_FAMILIES] == [8, 16, 32] * 3
    assert (bc.UNIT4.unit, bc.PERSISTENT.unit, bc.PERSISTENT.persistent) == (4, 8, True)
    names = [f.name for f in bc.LAB_FAMILIES]
    assert len(set(names)) == len(names) == 38
    for f in bc.LAB_FAMILIES:
        if f.kind != "tile":
            assert f.halo == (2 if f.arm.method == "mhc" or f.arm.colour else 1)
    assert {f.halo for f in bc.STRIP_FAMILIES} == {1, 2}


def test_heights_are_the_ones_asked_for():
    assert set(bc.HEIGHTS[16]) >= {19, 20, 31, 32, 33, 36, 48, 49, 51, 52, 64, 68, 100, 116}
    assert set(bc.HEIGHTS[8]) >= {11, 12, 16, 17, 20, 32, 36, 52, 116}
    assert set(bc.HEIGHTS[32]) >= {35, 36, 64, 65, 68, 100, 132}
    assert set(bc.HEIGHTS[4]) >= {8, 11, 12, 20, 36}


def test_widths_and_strides():
    for fam in bc.LAB_FAMILIES:
        w0, w1 = bc.widths(fam)
        if fam.kind != "tile":
            assert (w0, w1) == (266, 268) == sc.SWEEP_WIDTHS
            assert sc.last_group(w0)["full"] is False and sc.last_group(w1)["full"] is True
            assert sc.last_group(w0)["wave"] == sc.last_group(w1)["wave"] == 1          # behind the first strip seam
            continue
        tw = bc.tile_w(fam)
        assert (w0, w1) == {256: (270, 272), 512: (522, 528), 1024: (1030, 1040)}[tw]
        for w, arm in ((w0, "generic"), (w1, "fast")):
            s, d = bc.strides(fam, w, 36)
            assert tc.expected_arm(tc.make_launch(w, 36, s, d)) == arm, (fam.name, w)
            assert -(-w // tw) == 2                      # a tile seam, and a partial last tile


def test_cases_rotate_and_lab_cases_are_product_cases():
    for fam in bc.LAB_FAMILIES:
        cases = bc.product_cases(fam)
        assert len(cases) == 2 * len(bc.HEIGHTS[fam.unit]) and len(set(cases)) == len(cases)
        halves = [bc.product_half(fam, k) for k in (0, 1)]
        assert sorted(halves[0] + halves[1]) == sorted(cases) and not set(halves[0]) & set(halves[1])
        if not fam.persistent:
            assert {bc.expected_bands(fam, c) for c in cases} == {1, 2, 3, 4}
            assert all(len({bc.expected_bands(fam, c) for c in h}) >= 3 for h in halves), fam.name
        assert {c.order for c in cases} == set(sc.ORDERS), fam.name
        if fam.kind == "strip":
            assert len({c.layout for c in cases}) == 4
            if fam.arm.bits:
                assert {c.sbe for c in cases} == {False, True}
            if fam.arm.out16:
                assert {c.dbe for c in cases} == {False, True}
        seen = set()
        for env in bc.LAB_WANTS:
            lab = bc.lab_cases(fam, env)
            assert [c.h for c in lab] == list(bc.HEIGHTS[fam.unit]) and set(lab) <= set(cases)
            assert {c.w for c in lab} == set(bc.widths(fam))
            seen |= set(lab)
        assert seen == set(cases), fam.name             # the four settings together run every product case


def test_single_cases():
    # C: the plan walk re-cuts the frame; with 8 bands wanted the count shrinks and grows again on the live slot
    w, h = bc.RECUT_SIZE
    units = [tc.shape_of(n).tile_h for n in bc.RECUT_PLANS]
    assert units == [32, 8, 16, 32, 8]
    assert [bc.host_bands(4, BIG, h, u) for u in units] == [4, 4, 4, 4, 4]
    assert [bc.band_rows(4, h, u) for u in units[:3]] == [[(0, 32), (32, 64), (64, 96), (96, 100)]] * 3
    # the first frame -- the one the slot's events are made for -- is cut into the FEWEST bands of the walk, so the
    # second plan needs events for bands the slot has none for yet
    for want, counts in ((8, [4, 7, 7, 4, 7]), (3, [2, 3, 3, 2, 3])):
        assert [bc.host_bands(want, BIG, h, u) for u in units] == counts
        assert counts[0] == min(counts) < counts[1] == max(counts)
    # D: w % 4 == 2 at the default stride, one width step below the threshold is not banded
    for name in bc.UNPADDED_FAMILIES:
        fam = bc.family(name)
        w = bc.unpadded_width(fam)
        size = lambda w: bc.planes(fam) * bc.default_dst_stride(fam, w) * bc.UNPADDED_HEIGHT     # noqa: E731
        assert w % 4 == 2 and size(w) >= BIG > size(w - 4) and w * bc.UNPADDED_HEIGHT < 5.7e6, (name, w)
        assert (bc.default_dst_stride(fam, w) == bc.row_bytes(fam, w)) == (fam.kind in ("strip", "tile"))    # 1-D, 2-D
    assert {bc.family(n).kind for n in bc.UNPADDED_FAMILIES} == {"strip", "rgb24", "planar", "tile"}
    assert {bc.pixel_bytes(bc.family(n)) for n in bc.UNPADDED_FAMILIES} == {1, 3, 4, 8}
    # E: a grid that does not divide the height and a window across two band seams
    for h in bc.ONCE_HEIGHTS:
        nb = bc.host_bands(4, BIG, h, 16)
        assert nb == 4
        zx, zy = bc.stats_grid(h)
        for w in sc.SWEEP_WIDTHS:
            x0, y0, ww, hh = bc.hist_window(nb, h, 16, w)
            seams = [y for y, _ in bc.band_rows(nb, h, 16)[1:]]
            assert sum(y0 < s < y0 + hh for s in seams) == 2 and y0 & 1 and x0 % 2 == 0 and ww % 2 == 0
            assert x0 + ww <= w and y0 + hh <= h and zx <= w // 2 and zy <= h // 2
    assert {bc.family(n).kind for n in bc.ONCE_FAMILIES} == {"strip", "planar"}
    assert [bc.family(n).arm.colour for n in bc.ONCE_FAMILIES] == [False, True, False]
    # F
    assert bc.host_bands(4, BIG, bc.STAGE_HEIGHT, 16) == 4 and all(bc.family(n).arm.colour for n in bc.STAGE_FAMILIES)


def test_one_rule_two_tables():
    """the rgb2bayer tables mirror the same rule at the inverse direction's unit of 16 rows"""
    assert rc.BAND_UNIT == 16 and rc.BAND_MIN_BYTES == bc.BAND_MIN_BYTES
    frames = [rc.resolved(g) for g in (rc.BANDED_FRAME, rc.BANDED_FRAME_PX8)]
    for g in frames:
        src_bytes = g.src_stride * g.h
        assert src_bytes >= BIG
        for want in (4,) + rc.HOST_BANDS + (1, 2, 5, 6, 7):
            assert rc.host_bands(want, src_bytes, g.h) == bc.host_bands(want, src_bytes, g.h, 16) > (1 if want > 1 else 0)
        assert rc.host_bands(4, BIG - 1, g.h) == bc.host_bands(4, BIG - 1, g.h, 16) == 1
    for h in bc.HEIGHTS[16]:
        for want in range(0, 9):
            assert rc.host_bands(want, BIG, h) == bc.host_bands(want, BIG, h, 16), (h, want)


# -- the halo against the models --------------------------------------------------------------------------------------

DEP_W = 8


def _model(name):
    """(halo, reach, f): the halo rows uploaded below a band of such a context, the rows below its own that an output
    row of the MODEL depends on (the colour kernel loads the MHC window whatever the method), and f, which maps
    (h, DEP_W) 8-bit samples to output bytes (h, ...)"""
    if name == "bilinear":
        return 1, 1, lambda S: hm.native_rgb(S, "grbg").reshape(S.shape[0], -1)
    if name == "mhc":
        return 2, 2, lambda S: mm.native_rgb(S, "grbg", 8).reshape(S.shape[0], -1)
    method = name.split("_")[1]
    return 2, 2 if method == "mhc" else 1, lambda S: cm.bayer2rgb_colour(sc.frame_bytes(S, 0, None), DEP_W, S.shape[0], "grbg", "RGBx", bits=0,
                                            out16=False, method=method)


def lowest_rows_read(name, h):
    """per output row y: the LAST source row whose change alters row y of the model's output (one source row perturbed
    at a time, all its samples)"""
    f = _model(name)[2]
    rng = np.random.default_rng(h)
    S = rng.integers(32, 224, (h, DEP_W))
    base = np.asarray(f(S)).reshape(h, -1)
    last = np.full(h, -1)
    for r in range(h):
        T = S.copy()
        T[r] = S[r] ^ 0x15                              # every sample of the row changes, by an odd amount
        changed = (np.asarray(f(T)).reshape(h, -1) != base).any(axis=1)
        last[changed] = r
    return last


@pytest.mark.parametrize("name", ["bilinear", "mhc", "colour_bilinear", "colour_mhc"])
def test_no_band_reads_below_its_upload(name):
    """The rows band b's output depends on, by the NumPy models ALONE, lie inside the rows uploaded when band b's kernel
    may start (band_cases.uploaded_rows: the mirror of enqueue_frame_banded's `up_to`) -- for every table height, every
    unit and every wanted count, the bottom rule dn (H - 1) = H - 4 and MHC's reflection included.  This checks the CUT
    RULE (rows per band + halo) against the models, not the C code: a halo that is too small in the library makes a
    band read rows whose upload is merely queued, which no deterministic GPU test can show."""
    halo, reach, _ = _model(name)
    heights = sorted({h for u in bc.UNITS for h in bc.HEIGHTS[u]})
    for h in heights:
        last = lowest_rows_read(name, h)
        assert (last >= 0).all()
        need = [min(y + reach, h - 1) for y in range(h)]
        assert (last <= need).all(), (name, h)
        assert last[:h - reach].tolist() == need[:h - reach], (name, h)     # the perturbation shows every row read
        for unit in bc.UNITS:
            if h not in bc.HEIGHTS[unit]:
                continue
            for want in WANTS:
                nb = bc.host_bands(want, BIG, h, unit)
                up = bc.uploaded_rows(nb, h, unit, halo)
                for b, (y0, y1) in enumerate(bc.band_rows(nb, h, unit)):
                    assert last[y0:y1].max() < up[b], (name, h, unit, want, b)
                    if reach == 2 and b < nb - 1:                            # one halo row would NOT do
                        assert last[y0:y1].max() >= bc.uploaded_rows(nb, h, unit, 1)[b]
