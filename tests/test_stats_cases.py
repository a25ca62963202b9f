"""The case tables of tests/stats_cases.py reach what they are meant to reach -- asserted from the tables and the mirror
of the launch geometry alone, so that the GPU tests built on them (tests/test_gpu_stats_geometry.py) cannot go vacuous
when a table is edited.  The frames of the segment table and of the 64 x 64 grid also run through both forms of the
model (tests/stats_model.py), the vectorised one against the pixel loop: about 150 000 pixels in all."""
import numpy as np
import pytest

import stats_cases as tc
import stats_model as sm


def seg_geometries():
    return {(H, zy): tc.geometry(tc.SEG_FORMATS[0][0], H, 0, 1, zy) for H, zy in tc.SEG_CASES}


def test_mirror_is_the_models_grid():
    """ch and cw as the library computes them are the model's cell(), and the segments tile every zone row once"""
    for W, H, bits, zx, zy in tc.ZONE_CASES + tuple((66, H, 0, 1, zy) for H, zy in tc.SEG_CASES):
        geo = tc.geometry(W, H, bits, zx, zy)
        assert geo.ch == sm.cell(H, zy) and geo.cw == sm.cell(W, zx)
        seen = np.zeros(H, int)
        for s in tc.segments(H, zy, geo):
            assert s.y0 % 2 == 0 and tc.AHEAD * s.full + 2 * s.pairs + s.single == tc.rows(s)
            assert all(y // geo.ch == s.zy for y in range(s.y0, s.y1))
            seen[s.y0:s.y1] += 1
        assert (seen == 1).all()


def test_segment_table_formats():
    """both formats: one zone column, 17 dwords of which the last is a half (8-bit) or full (12-bit), padded rows"""
    for W, bits, _ in tc.SEG_FORMATS:
        geo = tc.geometry(W, 64, bits, 1, 1)
        assert geo.row_dwords == 17 and geo.strips == 1 and tc.row_bytes(W, bits) == 68 and tc.SEG_STRIDE == 80
        S = tc.samples(tc.seg_frame((W, bits, False), 64, 1), W, 64, bits)
        (lo0, hi0), (lo1, hi1) = tc.SEG_RANGES[bits]
        # a phantom row of zeroes would be counted under the first range; the second leaves samples out below
        assert lo0 == 0 and (S > hi0).any() and hi0 < tc.vmax_of(bits)
        assert (S < lo1).any() and ((S >= lo1) & (S <= hi1)).any() and hi1 == tc.vmax_of(bits)
    assert {f[1] for f in tc.SEG_FORMATS} == {0, 12} and not any(f[2] for f in tc.SEG_FORMATS)


def test_last_segments_of_1_2_3_4_6_and_8_rows():
    last = {}
    for case, geo in seg_geometries().items():
        for s in tc.last_segments(*case, geo):
            last.setdefault(tc.rows(s), []).append((case, s))
    for n in (1, 2, 3, 4, 6, 8):
        assert n in last, n
    # the ones the table names: a single row, exactly one unrolled iteration and no tail, 4 and 2 rows at a zone seam
    assert [s for c, s in last[1] if c == (65, 1)] == [tc.Segment(0, 1, 64, 65, 0, 0, True)]
    assert [s for c, s in last[8] if c == (72, 1)] == [tc.Segment(0, 1, 64, 72, 1, 0, False)]
    assert [s for c, s in last[4] if c == (134, 2)] == [tc.Segment(0, 1, 64, 68, 0, 2, False)]
    assert [s for c, s in last[2] if c == (134, 2)] == [tc.Segment(1, 1, 132, 134, 0, 1, False)]
    # a tail behind a full iteration, third and fourth segments, and a frame of one full segment alone
    assert [s for s in tc.last_segments(74, 1, seg_geometries()[74, 1])] == [tc.Segment(0, 1, 64, 74, 1, 1, False)]
    assert tc.last_segments(129, 1, seg_geometries()[129, 1])[0].seg == 2
    assert tc.last_segments(193, 1, seg_geometries()[193, 1])[0].seg == 3
    assert [tc.rows(s) for s in tc.segments(64, 1, seg_geometries()[64, 1])] == [64]


def test_empty_segment_inside_a_non_empty_zone_row():
    geo = seg_geometries()[200, 3]
    segs = tc.segments(200, 3, geo)
    assert geo.ch == 68 and geo.segs == 2
    assert segs[4] == tc.Segment(2, 0, 136, 200, 8, 0, False) and tc.rows(segs[5]) == 0 and segs[5].seg == 1
    assert all(tc.rows(s) > 0 for s in segs[:4])


def test_segment_cut_by_an_odd_height():
    """y1 is the frame height, odd, and below both the segment's and the zone's end"""
    cut = {}
    for (H, zy), geo in seg_geometries().items():
        for s in tc.segments(H, zy, geo):
            if s.y1 == H and H % 2 == 1 and H < min(s.y0 + tc.SEG_ROWS, (s.zy + 1) * geo.ch):
                cut[H, zy] = s
    assert cut[199, 3] == tc.Segment(2, 0, 136, 199, 7, 3, True)
    assert cut[65, 1].single and cut[67, 1] == tc.Segment(0, 1, 64, 67, 0, 1, True)


def test_batch_table_splits_frames_and_strips():
    geos = {(W, bits, n): tc.geometry(W, tc.BATCH_HEIGHT, bits, 1, 1) for W, bits, n in tc.BATCH_CASES}
    assert all(g.strips >= 2 and n >= 2 for (_, _, n), g in geos.items())
    # strips == frames would hide a transposed split: both orders of the two occur
    assert any(g.strips < n for (_, _, n), g in geos.items()) and any(g.strips > n for (_, _, n), g in geos.items())
    # a last strip with exactly one live lane -- a half dword at 8 bits -- in both sample widths
    one = {bits: (W, g) for (W, bits, _), g in geos.items() if g.row_dwords % tc.STRIP_DWORDS == 1}
    assert one[0][0] % 4 == 2 and set(one) == {0, 16}
    assert geos[1026, 0, 3].row_dwords == 257 and geos[2050, 0, 2].strips == 3
    for zx, zy in tc.BATCH_ZONES:
        assert zy <= tc.BATCH_HEIGHT // 2 and all(zx <= W // 2 for W, _, _ in tc.BATCH_CASES)
    for W, bits, n in tc.BATCH_CASES:
        padded, raws = tc.batch_frames(W, bits, n)
        assert padded.shape == (n, raws[0].size + 64) and padded.shape[1] % 4 == 0 and (padded[:, -64:] == 0xFF).all()
        assert len({r.tobytes() for r in raws}) == n


def test_zone_table_fills_the_lds_table_and_sits_on_the_seams():
    W, H, bits, zx, zy = tc.ZONE_CASES[0]
    geo = tc.geometry(W, H, bits, zx, zy)
    assert (zx, zy, geo.cw, geo.ch, geo.segs, geo.strips) == (64, 64, 2, 2, 1, 1)
    lo, hi = tc.zone_range(bits)
    want = sm.zone_stats(tc.samples(tc.zone_frame(*tc.ZONE_CASES[0]), W, H, bits), zx, zy, lo, hi)
    # one sample per site in every one of the 4096 zones, each of them counted or clipped: zone column 63 and zone
    # row 63 are not empty, and a workgroup leaves none of its 256 table entries at zero
    assert want.shape == (64, 64) and (want["count"].astype(int) + want["clipped"] == 1).all()
    assert want["count"].any() and want["clipped"].any()
    # 64 zone columns over one wave of 16-bit samples: every lane a zone of its own
    W, H, bits, zx, zy = tc.ZONE_CASES[1]
    geo = tc.geometry(W, H, bits, zx, zy)
    assert (geo.cw, geo.ch, geo.row_dwords) == (2, 2, tc.WAVE_DWORDS) and zy == H // 2
    # a zone boundary between two waves and between two workgroups, 8-bit and deep
    seams = {(bits == 0, tuple(tc.zone_seam_dwords(W, bits, tc.geometry(W, H, bits, zx, zy))))
             for W, H, bits, zx, zy in tc.ZONE_CASES[2:]}
    assert seams == {(True, (tc.WAVE_DWORDS,)), (True, (tc.STRIP_DWORDS,)), (False, (tc.WAVE_DWORDS,)),
                     (False, (tc.STRIP_DWORDS,))}
    assert [tc.geometry(W, H, bits, zx, zy).cw for W, H, bits, zx, zy in tc.ZONE_CASES[2:]] == [256, 1024, 128, 512]
    for W, H, bits, zx, zy in tc.ZONE_CASES:
        assert 1 <= zx <= min(tc.MAX_ZONES, W // 2) and 1 <= zy <= min(tc.MAX_ZONES, H // 2)


@pytest.mark.parametrize("bits", tc.DEEP_BITS)
def test_deep_range_frames_plant_the_neighbours_of_both_ends(bits):
    W, H = tc.DEEP_SIZE
    vmax = tc.vmax_of(bits)
    assert tc.deep_ranges(bits) == ((0, 0), (vmax, vmax), (vmax // 2, vmax // 2), (1, vmax - 1))
    assert tc.planted(bits, 0, 0) == [0, 1] and tc.planted(bits, vmax, vmax) == [vmax - 1, vmax]
    assert tc.planted(bits, 1, vmax - 1) == [0, 1, vmax - 1, vmax] and len(tc.planted(bits, vmax // 2, vmax // 2)) == 3
    for big_endian in (False, True):
        for lo, hi in tc.deep_ranges(bits):
            raw = tc.deep_range_frame(bits, big_endian, lo, hi)
            plant = tc.planted(bits, lo, hi)
            words = raw.view(">u2" if big_endian else "<u2")
            assert raw.shape == (H, 2 * W) and (words[0, :len(plant)] & vmax).tolist() == plant
            assert bits == 16 or (words[0, :len(plant)] >> bits == (1 << (16 - bits)) - 1).all()
            S = tc.samples(raw, W, H, bits, big_endian)
            assert S[0, :len(plant)].tolist() == plant and S.max() <= vmax
            z = sm.zone_stats(S, *tc.DEEP_ZONES, lo, hi)
            assert z["count"].any() and (z["clipped"].any() or hi == vmax)
            assert int(z["count"].sum()) + int(z["clipped"].sum()) + int((S < lo).sum()) == W * H


def test_site_frame_sums_differ_and_pass_32_bits():
    """67 600 samples per site: the sums of the sites at 65535 and 65534 pass 2^32, the one at 32769 passes 2^31 (the
    sign of a 32-bit integer) and stays below 2^32 (32769 x 67600 = 2 215 184 400), the one at 3 is small; all differ"""
    W, H = tc.SITE_SIZE
    want = sm.zone_stats(tc.samples(tc.site_frame(), W, H, 16), 1, 1, 0, 65535)
    sums = want["sum"][0, 0].tolist()
    assert sums == [67600 * v for v in tc.SITE_PLANES] and len(set(sums)) == 4
    assert [s > 1 << 32 for s in sums] == [True, True, False, False] and sums[2] > 1 << 31
    assert len({s & 0xFFFFFFFF for s in sums}) == 4             # ... in their low halves too
    assert want["count"][0, 0].tolist() == [67600] * 4 and not want["clipped"].any()


@pytest.mark.parametrize("H,zones_y", tc.SEG_CASES)
def test_model_against_the_pixel_loop_on_the_segment_frames(H, zones_y):
    for fmt in tc.SEG_FORMATS:
        W, bits, big_endian = fmt
        raw = tc.seg_frame(fmt, H, zones_y)
        assert raw.shape == (H, tc.SEG_STRIDE) and (raw[:, tc.row_bytes(W, bits):] == 0xFF).all()
        S = tc.samples(raw, W, H, bits, big_endian)
        for lo, hi in tc.SEG_RANGES[bits]:
            fast, slow = sm.zone_stats(S, 1, zones_y, lo, hi), sm.zone_stats_slow(S, 1, zones_y, lo, hi)
            for f in ("sum", "count", "clipped"):
                assert np.array_equal(fast[f], slow[f]), (fmt, lo, hi, f)


def test_model_against_the_pixel_loop_on_the_64x64_grid():
    W, H, bits, zx, zy = tc.ZONE_CASES[0]
    S = tc.samples(tc.zone_frame(W, H, bits, zx, zy), W, H, bits)
    lo, hi = tc.zone_range(bits)
    fast, slow = sm.zone_stats(S, zx, zy, lo, hi), sm.zone_stats_slow(S, zx, zy, lo, hi)
    for f in ("sum", "count", "clipped"):
        assert np.array_equal(fast[f], slow[f]), f
