"""TEST INFRASTRUCTURE: the case table of the focus-kernel geometry test (tests/test_gpu_focus.py::test_case_table), its
frames and a mirror of the kernel's LAUNCH GEOMETRY.  No GPU and no library here: tests/test_focus_cases.py asserts, from
this table, the mirror and the model (tests/focus_model.py) alone, that the shapes reach the seams they are meant to
reach.  The mirror is not a second model of the statistics.

mosaic_focus_kernel (csrc/mibayer_kernels.hip) has mosaic_stats_kernel's launch: a workgroup is 256 lanes = four waves
side by side on one strip of 256 dwords of a row (four 8-bit or two 16-bit samples per dword), walking one segment of at
most SEG_ROWS rows of ONE zone row.  A lane takes the samples two columns away from the dwords of its neighbour lanes --
of another wave at every 64th dword, of another workgroup at every 256th -- and the rows two above and below from its own
five-row window, which a segment starts with two halo rows of the segment (or zone row) above and ends with two of the
one below.  Seams, then, are lines between two columns or two rows across which a response reaches:
  lane     every dword boundary of a row                    wave     every 64th
  strip    every 256th                                       zone-x   every zone column's first pixel
  segment  the first row of every segment but a zone row's first
  zone-y   the first row of every zone row but the first
The 8-bit tail is a last dword of two columns (W = 2 mod 4); the frame's borders are where responses stop existing."""
import collections

import numpy as np

import focus_model as fm
import stats_cases as tc

SEG_ROWS = tc.SEG_ROWS
WAVE_DWORDS = tc.WAVE_DWORDS
STRIP_DWORDS = tc.STRIP_DWORDS

Case = collections.namedtuple("Case", "W H bits big_endian zones_x zones_y")

# 8-bit: one lane; a half dword and no rv; three dwords; past a wave; past a strip, whole and with a tail, past a segment;
# four strips and two zone rows of two segments; 64 x 64 zones with empty trailing ones.  Deep: three dwords; past a wave
# (big-endian); past a strip and a segment (16 bits: the widest responses); two strips; two strips and a tail of six
# dwords, two zone rows of two segments
CASES = (
    Case(4, 5, 0, False, 1, 1), Case(6, 3, 0, False, 1, 1), Case(10, 6, 0, False, 2, 3), Case(66, 18, 0, False, 3, 5),
    Case(258, 37, 0, False, 3, 5), Case(266, 70, 0, False, 3, 1), Case(1026, 133, 0, False, 3, 2),
    Case(1030, 4, 0, False, 5, 2), Case(258, 130, 0, False, 64, 64),
    Case(6, 5, 10, False, 1, 1), Case(130, 37, 12, True, 3, 5), Case(258, 70, 16, False, 2, 1),
    Case(514, 18, 12, False, 3, 5), Case(518, 133, 10, True, 3, 2),
)
# the kinds of case in which one direction has no response at all (include/mibayer.h): named, and no others
EXEMPT_H = tuple(c for c in CASES if c.W == 4)
EXEMPT_V = tuple(c for c in CASES if c.H in (3, 4))


def vmax_of(case):
    return tc.vmax_of(case.bits)


def threshold(case):
    """near max / 4: of random samples about half of the responses are above"""
    return vmax_of(case) // 4 + 1


def geometry(case):
    return tc.geometry(case.W, case.H, case.bits, case.zones_x, case.zones_y)


def column_seams(case):
    """{kind: [x, ...]}: the columns at which a new lane / wave / strip / zone column starts"""
    geo, spd = geometry(case), tc.samples_per_dword(case.bits)
    dwords = range(1, geo.row_dwords)
    return {"lane": [spd * g for g in dwords], "wave": [spd * g for g in dwords if g % WAVE_DWORDS == 0],
            "strip": [spd * g for g in dwords if g % STRIP_DWORDS == 0], "zone-x": list(range(geo.cw, case.W, geo.cw))}


def row_seams(case):
    """{kind: [y, ...]}: the rows at which a new segment of the same zone row / a new zone row starts"""
    geo = geometry(case)
    segs = [s for s in tc.segments(case.H, case.zones_y, geo) if tc.rows(s) > 0]
    return {"segment": [s.y0 for s in segs if s.seg > 0], "zone-y": [s.y0 for s in segs if s.seg == 0 and s.zy > 0]}


def frame(case):
    """(H, stride) bytes of the case's frame, from a seed of its own: random samples (junk above `bits`, 0xFF in the row
    padding) with two planted responses next to the first column seam of the row in the middle: |rh| = thr at x = 2 and
    thr - 1 at x = 3 where the frame is wide enough"""
    rng = np.random.default_rng(tc.case_seed(*case))
    W, H, bits = case.W, case.H, case.bits
    S = rng.integers(0, vmax_of(case) + 1, (H, W))
    if W >= 8:
        y, thr = H // 2, threshold(case)
        S[y, 0:8] = 0
        S[y, 2] = (thr + 1) // 2            # 2 c - 0 - 0 = thr or thr + 1 ...
        S[y, 4] = (thr + 1) // 2 * 2 - thr  # ... - that odd bit: |rh (2)| = thr
        S[y, 3] = thr // 2                  # 2 c = thr or thr - 1 ...
        S[y, 5] = thr // 2 * 2 - (thr - 1)  # ... |rh (3)| = thr - 1
    if bits == 0:
        raw = np.full((H, tc.row_bytes(W, 0)), 0xFF, np.uint8)
        raw[:, :W] = S
        return raw
    junk = rng.integers(0, 1 << 16, (H, W)) & ~vmax_of(case) & 0xFFFF
    return tc.pack_words((S | junk).astype(np.uint16), bits, case.big_endian)


def samples(case, raw):
    return tc.samples(raw, case.W, case.H, case.bits, case.big_endian)


def expected(case, raw, thr=None):
    return fm.zone_focus(samples(case, raw), case.zones_x, case.zones_y, threshold(case) if thr is None else thr,
                         vmax_of(case))
