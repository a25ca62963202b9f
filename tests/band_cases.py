"""TEST INFRASTRUCTURE: the case tables of the host-path band tests (tests/test_gpu_band_seams.py) and a mirror of the
BAND CUT of the host path.  No GPU and no library here: tests/test_band_cases.py asserts, from these tables, the mirror
and the NumPy models alone, what the heights reach.

choose_host_bands / enqueue_frame_banded (csrc/mibayer_abi.hip): a host-path frame whose big side is 16 MiB or more and
that has the link to itself is cut into bands of whole UNITS -- a tile row of the tile kernels (8, 16 or 32 rows by
shape), a chunk of 16 rows of the strip kernels.  Band b gets an upload that ends `halo` rows below it, a launch over
its units and a download of its rows.  The cut depends on the frame's BYTES, not on its width: a destination stride far
above the row makes a frame of a few dozen rows a banded one (banded_stride), which is what every case here does."""
import collections

import strip_cases as sc
import tile_cases as tc
from test_gpu_planar import ARMS as PLANAR_ARMS, rotate as planar_rotate
from test_gpu_rgb24 import ARMS as RGB24_ARMS, rotate as rgb24_rotate

BAND_MIN_BYTES = 16 << 20       # choose_host_bands: smaller frames are not banded
MAX_BANDS = 8                   # kMaxHostBands
PRODUCT_WANT = 4                # the bands the product build asks for
LAB_WANTS = (None, 2, 3, 8)     # MIBAYER_HOST_BANDS of the lab build; None: unset
MIN_LAST_ROWS = 4               # dn (H - 1) = H - 4: the last band holds at least 4 rows
MIN_BAND_ROWS = 8               # per * unit >= 8


def wanted(env):
    return PRODUCT_WANT if env is None else env


# -- the mirror ---------------------------------------------------------------------------------------------------------

def host_bands(want, big_side_bytes, h, unit, persistent=False):
    """choose_host_bands: the bands a frame of h rows, cut in units of `unit` rows, is converted in"""
    want = min(want, MAX_BANDS)
    if want < 2 or persistent or big_side_bytes < BAND_MIN_BYTES:
        return 1
    units = -(-h // unit)
    while want > 1:
        per = -(-units // want)
        nb = -(-units // per)
        if nb == want and per * unit >= MIN_BAND_ROWS and h - (nb - 1) * per * unit >= MIN_LAST_ROWS:
            return want
        want -= 1
    return 1


def band_units(nb, h, unit):
    """enqueue_frame_banded: the [t0, t1) units of each band"""
    units = -(-h // unit)
    per = -(-units // nb)
    return [(b * per, min((b + 1) * per, units)) for b in range(nb)]


def band_rows(nb, h, unit):
    """the [y0, y1) rows of each band"""
    return [(t0 * unit, min(t1 * unit, h)) for t0, t1 in band_units(nb, h, unit)]


def uploaded_rows(nb, h, unit, halo):
    """per band: the source rows [0, n) queued for upload by the time the band's kernel may start"""
    out, up = [], 0
    for _, y1 in band_rows(nb, h, unit):
        up = max(up, min(y1 + halo, h))
        out.append(up)
    return out


def banded_stride(row_bytes, h, planes=1, align=16, extra=0):
    """the smallest stride >= row_bytes that is `extra` mod `align` and makes planes * stride * h >= 16 MiB"""
    need = max(row_bytes, -(-BAND_MIN_BYTES // (planes * h)))
    return need + (extra - need) % align


# -- families ---------------------------------------------------------------------------------------------------------------

# kind: "strip" (strip_cases.ARMS), "rgb24", "planar" (the arms of their GPU tests) or "tile" (arm: the variant's name);
# halo: rows below a band its kernel reads -- 1 for plain bilinear, 2 for MHC and for every colour context
Family = collections.namedtuple("Family", "name kind unit arm halo persistent")


def _halo(arm):
    return 2 if arm.method == "mhc" or arm.colour else 1


STRIP_FAMILIES = tuple(Family(a.name, "strip", sc.STRIP_ROWS, a, _halo(a), False) for a in sc.ARMS)
RGB24_FAMILIES = tuple(Family(a.name, "rgb24", sc.STRIP_ROWS, a, _halo(a), False) for a in RGB24_ARMS)
PLANAR_FAMILIES = tuple(Family(a.name, "planar", sc.STRIP_ROWS, a, _halo(a), False) for a in PLANAR_ARMS)
TILE_FAMILIES = tuple(Family(n, "tile", tc.shape_of(n).tile_h, n, 1, False) for n in tc.PRODUCTION_NAMES)   # ids 1 .. 9
PRODUCT_FAMILIES = STRIP_FAMILIES + RGB24_FAMILIES + PLANAR_FAMILIES + TILE_FAMILIES
# the lab build only: 256 x 4 tiles (the one unit at which per * unit >= 8 bites) and a persistent arm (never banded)
UNIT4 = Family("lds_1x1_r4_dpp_nt", "tile", 4, "lds_1x1_r4_dpp_nt", 1, False)
PERSISTENT = Family("persist_4x2_r4_nt", "tile", 8, "persist_4x2_r4_nt", 1, True)
LAB_FAMILIES = PRODUCT_FAMILIES + (UNIT4, PERSISTENT)
LAB_TILE_W = {UNIT4.name: 256, PERSISTENT.name: 1024}

# per unit: the heights around one, two, three and four units at which choose_host_bands changes its answer (a last band
# of 3, 4 and 5 rows, a full and a short unit in the last band), and -- behind the gap -- the ones that six bands (and,
# at units 4 and 32, four, seven and eight) need: k units and a last band of 4 rows.  tests/test_band_cases.py asserts
# what they reach; profiles/2026-10-20_band_seam_tests.md lists the second group
HEIGHTS = {
    16: (19, 20, 31, 32, 33, 36, 48, 49, 51, 52, 64, 68, 100, 116,  84),
    8: (11, 12, 16, 17, 20, 32, 36, 52, 116,  44),
    32: (35, 36, 64, 65, 68, 100, 132,  164, 196, 228),
    4: (8, 11, 12, 20, 36,  28, 44, 56, 60),
}
UNITS = tuple(sorted(HEIGHTS))


def family_id(fam):
    return fam.name


def tile_w(fam):
    return LAB_TILE_W.get(fam.name) or tc.shape_of(fam.name).tile_w


def widths(fam):
    """strip families: a tail group and a full group behind the first strip seam (the strip height sweep's widths);
    tile variants: a partial last tile (270 / 522 / 1030: the generic arm, on a stride that is 8 mod 16) and a last tile
    of one 16-byte chunk (272 / 528 / 1040: the fast arm, both strides on 16)"""
    if fam.kind != "tile":
        return sc.SWEEP_WIDTHS
    return {256: 270, 512: 522, 1024: 1030}[tile_w(fam)], tile_w(fam) + 16


def planes(fam):
    return 3 if fam.kind == "planar" else 1


def pixel_bytes(fam):
    return {"strip": 8 if fam.kind == "strip" and fam.arm.out16 else 4, "rgb24": 3, "planar": 1, "tile": 4}[fam.kind]


def row_bytes(fam, w):
    """the bytes of a destination row that are written"""
    return pixel_bytes(fam) * w


def src_row_bytes(fam, w):
    return (w + 3) & ~3 if fam.kind == "tile" else sc.src_row_bytes(w, fam.arm.bits)


def strides(fam, w, h):
    """(source stride, destination stride) of a banded case.  The source rows carry the 12 bytes of padding the
    families' own sweeps use (dword-aligned rows) but for the fast arm of a tile variant, whose strides are both on 16;
    the destination stride is 8 mod 16 likewise"""
    fast = fam.kind == "tile" and w % 16 == 0
    sstride = src_row_bytes(fam, w) + (0 if fast else 12)
    return sstride, banded_stride(row_bytes(fam, w), h, planes(fam), 16, 0 if fast else 8)


def rotate(fam, i, w, h):
    """case i of a family, by the family's own rotation of Bayer order, layout and byte orders"""
    if fam.kind == "strip":
        return sc.rotate(fam.arm, i, w, h)
    if fam.kind == "rgb24":
        return rgb24_rotate(i, w, h)
    if fam.kind == "planar":
        return planar_rotate(i, w, h)
    return tc.rotate(i, w, h)


def product_cases(fam):
    """section A: every height of the family's unit at both widths"""
    k = LAB_FAMILIES.index(fam)
    sizes = [(w, h) for w in widths(fam) for h in HEIGHTS[fam.unit]]
    return [rotate(fam, i + k, w, h) for i, (w, h) in enumerate(sizes)]


def product_half(fam, half):
    """the cases of every other height of the unit's list (half 0: the 1st, 3rd, ...), at both widths: a per-family
    test of all heights runs longer than the suite's slowest banded test did, so it is two tests"""
    hs = HEIGHTS[fam.unit]
    return [c for c in product_cases(fam) if hs.index(c.h) % 2 == half]


def lab_cases(fam, env):
    """section B: every height once, the two widths in turn; which height gets which width changes with the family and
    with MIBAYER_HOST_BANDS.  The cases are a subset of product_cases (same rotation), so a frame and its expectation
    are computed once"""
    k = LAB_FAMILIES.index(fam)
    hs = HEIGHTS[fam.unit]
    out = []
    for j, h in enumerate(hs):
        wi = (j + k + LAB_WANTS.index(env)) % 2
        out.append(rotate(fam, wi * len(hs) + j + k, widths(fam)[wi], h))
    return out


def expected_bands(fam, case, env=None):
    """the band count of a banded case of the tables (the destination is at or above the threshold by construction)"""
    _, dstride = strides(fam, case.w, case.h)
    return host_bands(wanted(env), planes(fam) * dstride * case.h, case.h, fam.unit, fam.persistent)


# -- single cases -----------------------------------------------------------------------------------------------------------

RECUT_SIZE = (1030, 100)                        # section C: one context, the plan walks through the three tile heights
# variant 3 first, then 1, 2, 3 and back to 1: units 32, 8, 16, 32, 8.  The slot's ring is made at the FIRST frame, with
# band events for the count of that moment: it has to be the small one for a later plan to need events the slot lacks
RECUT_PLANS = tc.NT_NAMES[2:] + tc.NT_NAMES + tc.NT_NAMES[:1]
UNPADDED_HEIGHT = 52                            # section D: default strides; 1-D downloads where stride == row bytes
ONCE_HEIGHTS = (52, 116)                        # section E: statistics and histogram behind the last band
STAGE_HEIGHT = 100                              # section F


def default_dst_stride(fam, w):
    """validate (): ROUND_UP_4 of the written bytes (16-bit output: 8 w)"""
    return (row_bytes(fam, w) + 3) & ~3


def unpadded_width(fam, h=UNPADDED_HEIGHT):
    """the smallest even width with w % 4 == 2 whose frame reaches the threshold at the default destination stride"""
    w = 6
    while planes(fam) * default_dst_stride(fam, w) * h < BAND_MIN_BYTES:
        w += 4
    return w


def family(name):
    return next(f for f in LAB_FAMILIES if f.name == name)


UNPADDED_FAMILIES = ("deep_10_to_8", "mhc_16_to_16", "deep_12_to_24", "mhc_8_to_planar", tc.NT_NAMES[0])
ONCE_FAMILIES = ("deep_10_to_8", "colour_mhc_10_to_8", "mhc_8_to_planar")
STAGE_FAMILIES = ("colour_bilinear_12_to_8", "colour_mhc_14_to_16")


def stats_grid(h):
    """a zone grid that does not divide the height: (zones_x, zones_y, lo, hi as fractions of the range are the
    test's)"""
    zy = 3 if h % 3 else 5
    assert h % zy and (2 * -(-((h + 1) // 2) // zy)) * zy != h
    return 5, zy


def hist_window(nb, h, unit, w):
    """(x0, y0, w, h): rows from the middle of band 0 to the middle of band 2 -- across two band seams"""
    rows = band_rows(nb, h, unit)
    assert len(rows) >= 3
    y0 = (rows[0][0] + rows[0][1]) // 2 | 1                 # an odd first row
    y1 = (rows[2][0] + rows[2][1]) // 2
    return 2, y0, w - 6, y1 - y0
