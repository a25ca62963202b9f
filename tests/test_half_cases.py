"""CPU tests of tests/half_cases.py: the table is the kernel's (its constants are read out of csrc/mibayer_internal.h) and
its cases reach the seams they are meant to reach -- every count of pixels in a row's last lane, a row that ends in a
full and in a partial wave, every place of the last lane in its quad, one and several waves and workgroups per row,
short last chunks and dropped last rows."""
import os
import re

import half_cases as hc
import half_model as hf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def kernel_constants():
    text = open(os.path.join(ROOT, "gst-plugins-bad_amd", "csrc", "mibayer_internal.h")).read()
    found = dict(re.findall(r"constexpr int (kHalf\w+|kMaxList) = ([^;]+);", text))
    env = {}
    for name in ("kHalfLanePixels", "kHalfWavePixels", "kHalfGroupPixels", "kHalfRows", "kMaxList"):
        env[name] = eval(found[name], {}, env)          # the header's own expressions over the earlier constants
    return env


def test_the_constants_are_the_kernels():
    k = kernel_constants()
    assert (hc.LANE_PIXELS, hc.WAVE_PIXELS, hc.GROUP_PIXELS, hc.ROWS, hc.MAX_LIST) == (
        k["kHalfLanePixels"], k["kHalfWavePixels"], k["kHalfGroupPixels"], k["kHalfRows"], k["kMaxList"])
    assert hc.WAVE_PIXELS == 64 * hc.LANE_PIXELS and hc.GROUP_PIXELS == 4 * hc.WAVE_PIXELS


def test_the_widths_are_the_extents_minus_one_zero_plus_one():
    for extent in (hc.LANE_PIXELS, 2 * hc.LANE_PIXELS, hc.WAVE_PIXELS, hc.GROUP_PIXELS):
        assert {extent - 1, extent, extent + 1} <= set(hc.OUT_WIDTHS), extent
    assert {2, 3, 4, 5, 7, 8, 9, 255, 256, 257, 1023, 1024, 1025} == set(hc.OUT_WIDTHS)
    assert min(hc.width_of(ow) for ow in hc.OUT_WIDTHS) == 4           # the smallest mosaic
    assert set(hc.HEIGHTS) == {3, 4, 5, 2 * hc.ROWS - 1, 2 * hc.ROWS, 2 * hc.ROWS + 1, 2 * hc.ROWS + 2}


def test_which_seam_every_width_reaches():
    ends = {ow: hc.row_end(ow) for ow in hc.OUT_WIDTHS}
    assert {e["n"] for e in ends.values()} == {1, 2, 3, 4}                      # every tail, and the full lane
    assert {ow for ow, e in ends.items() if e["wave_full"]} == {hc.WAVE_PIXELS, hc.GROUP_PIXELS}
    assert {e["quad_lane"] for e in ends.values()} == {0, 1, 2, 3}             # 8-byte pixels: every piece of a quad
    assert {e["wave"] for e in ends.values()} == {0, 1, 3, 4}                  # one wave, two, a workgroup, and one more
    # a tail of 1 and of 3 pixels (odd OW) in lane 0 of a wave behind a seam, and in the only lane of a row
    assert ends[257] == {"wave": 1, "lane": 0, "n": 1, "wave_full": False, "quad_lane": 0}
    assert ends[1025]["wave"] == 4 and ends[1025]["lane"] == 0 and ends[1025]["n"] == 1
    assert ends[3]["n"] == 3 and ends[7]["n"] == 3 and ends[7]["lane"] == 1
    assert ends[255]["lane"] == 63 and ends[255]["n"] == 3 and ends[1023]["lane"] == 63
    # the odd widths: a row of a 4-byte layout then ends off the 8-byte grid, of a 3-byte or planar one off the dword grid
    assert sum(ow & 1 for ow in hc.OUT_WIDTHS) == 8


def test_which_seam_every_height_reaches():
    got = {h: hc.chunks(h) for h in hc.HEIGHTS + (hc.SWEEP_HEIGHT,)}
    assert got[3] == (1, 1, True) and got[4] == (1, 2, False) and got[5] == (1, 2, True)
    assert got[2 * hc.ROWS - 1] == (1, hc.ROWS - 1, True)
    assert got[2 * hc.ROWS] == (1, hc.ROWS, False) and got[2 * hc.ROWS + 1] == (1, hc.ROWS, True)
    assert got[2 * hc.ROWS + 2] == (2, 1, False)
    assert got[hc.SWEEP_HEIGHT] == (2, 1, True)
    for h in got:
        assert hf.out_size(6, h)[1] == h >> 1 == hc.out_size(6, h)[1]


def test_every_family_meets_every_order_and_sample_format():
    assert len(hc.FAMILIES) == 4 + 2 + 2 + 3
    for i, fam in enumerate(hc.FAMILIES):
        cases = hc.cases(fam, i)
        assert len(cases) == 2 * (len(hc.OUT_WIDTHS) + len(hc.SWEEP_OUT_WIDTHS) * len(hc.HEIGHTS))
        assert {c.order for c in cases} == set(hc.ORDERS)
        assert {(c.bits, c.sbe) for c in cases} == set(hc.SAMPLES)
        # both sample widths at every size
        for in8 in (True, False):
            mine = [c for c in cases if (c.bits == 0) == in8]
            assert {(c.w, c.h) for c in mine} == set(hc.sizes()), (fam, in8)


def test_tails_are_written_in_stores_that_add_up_to_the_row_end():
    for fam in hc.FAMILIES:
        for n in (1, 2, 3, 4):
            stores = hc.tail_stores(fam, n)
            assert sum(stores) == fam.px * n, (fam, n)
        for ow in hc.OUT_WIDTHS:
            stride = hc.default_dst_stride(fam, ow)
            assert stride % 4 == 0 and 0 <= stride - hc.dst_row_bytes(fam, ow) < 4
            assert hc.padded_dst_stride(fam, ow) % (8 if fam.px == 8 else 4) == 0
            assert hf.default_stride(fam.fmt, ow) == stride
