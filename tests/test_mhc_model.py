"""CPU tests of the Malvar-He-Cutler model (tests/mhc_model.py), the arithmetic the GPU tests hold the kernel to:
a worked example per site kind, constant colour fields, and the image-quality gain over the bilinear model."""
import numpy as np
import pytest

import highbit_model as hm
import mhc_model as mm

ORDERS = ("bggr", "gbrg", "grbg", "rggb")


def test_filters_are_the_stated_ones():
    """spot taps of the x16 filters (include/mibayer.h, MIBAYER_FLAG_MHC), each summing to 16"""
    c = 2
    assert mm.F_G[c, c] == 8 and mm.F_G[c, c + 1] == 4 and mm.F_G[c + 2, c] == -2 and mm.F_G[c + 1, c + 1] == 0
    assert mm.F_ROW[c, c] == 10 and mm.F_ROW[c, c - 1] == 8 and mm.F_ROW[c, c + 2] == -2
    assert mm.F_ROW[c - 1, c + 1] == -2 and mm.F_ROW[c + 2, c] == 1 and mm.F_ROW[c + 1, c] == 0
    assert mm.F_COL[c - 1, c] == 8 and mm.F_COL[c, c - 2] == 1
    assert mm.F_DIAG[c, c] == 12 and mm.F_DIAG[c + 1, c - 1] == 4 and mm.F_DIAG[c - 2, c] == -3
    for k in (mm.F_G, mm.F_ROW, mm.F_COL, mm.F_DIAG):
        assert k.sum() == 16


def test_known_answer_each_site_kind():
    """bggr (B G / G R), 8-bit, background 100 with one R sample of 180 at (3,3): every output is 100 + 5 * the tap
    the impulse sits under ((16*100 + 80*tap + 8) >> 4), worked by hand from the filter table"""
    S = np.full((8, 8), 100, np.uint8)
    S[3, 3] = 180
    rgb = mm.native_rgb(S, "bggr", 8)
    want = {
        (3, 3): (180, 140, 160),        # R site: R = S, G = F_G centre 8, B = F_diag centre 12
        (3, 5): (100, 90, 85),          # R site, impulse at (0,-2): F_G -2, F_diag -3
        (3, 4): (140, 100, 100),        # G in an R row: R = F_row (0,-1) 8, B = F_col (0,-1) 0
        (4, 3): (140, 100, 100),        # G in a B row: R = F_col (-1,0) 8, B = F_row (-1,0) 0
        (3, 2): (140, 100, 100),        # G in an R row, impulse at (0,1): R = F_row 8
        (2, 3): (140, 100, 100),        # G in a B row, impulse at (1,0): R = F_col 8, B = F_row 0
        (4, 4): (120, 100, 100),        # B site: R = F_diag (-1,-1) 4, G = F_G (-1,-1) 0, B = S
        (2, 4): (120, 100, 100),        # B site, impulse at (1,-1): F_diag 4
        (5, 3): (100, 90, 85),          # R site, impulse at (-2,0): F_G -2, F_diag -3
        (4, 2): (120, 100, 100),        # B site, impulse at (-1,1): F_diag 4
        (1, 1): (100, 100, 100),        # R site two rows and columns away: F_diag / F_G have no (2,2) tap
    }
    for (y, x), rgb_want in want.items():
        assert tuple(int(v) for v in rgb[y, x]) == rgb_want, (y, x)


def test_known_answer_clamps_and_rounds():
    """a dark field with one bright sample: negative taps clamp to 0; the top of the range clamps to 2^depth - 1"""
    S = np.zeros((6, 6), np.int64)
    S[2, 2] = 255                                   # bggr: a B site
    rgb = mm.native_rgb(S, "bggr", 8)
    assert tuple(rgb[2, 4]) == (0, 0, 0)              # B site two columns right: F_G -2 * 255 -> < 0 -> 0
    assert rgb[2, 2, 0] == (12 * 255 + 8) >> 4      # R at the B site: F_diag centre, 191
    assert rgb[2, 3, 2] == (8 * 255 + 8) >> 4       # G in a B row, B = F_row (0,-1): 128 (rounded up from 127.5)
    S = np.full((6, 6), 4095, np.int64)
    S[2, 2] = 0
    rgb = mm.native_rgb(S, "bggr", 12)
    assert rgb[2, 4, 1] == 4095                      # 16*4095 + 2*4095 > 16*4095: clamped


def test_reflect_101_borders():
    """the model pads by reflection without repeating the edge sample: column -1 is column 1, -2 is 2, W is W-2"""
    rng = np.random.default_rng(3)
    S = rng.integers(0, 256, (7, 10))
    P = np.pad(S, 2, mode="reflect")
    assert (P[2:-2, 1] == S[:, 1]).all() and (P[2:-2, 0] == S[:, 2]).all()
    assert (P[2:-2, -2] == S[:, -2]).all() and (P[2:-2, -1] == S[:, -3]).all()
    assert (P[1, 2:-2] == S[1]).all() and (P[-1, 2:-2] == S[-3]).all()
    # F_G at (0,0) of a bggr frame (a B site) written out with the reflected indices
    acc = (8 * S[0, 0] + 4 * (S[0, 1] + S[0, 1] + S[1, 0] + S[1, 0]) - 2 * (S[0, 2] + S[0, 2] + S[2, 0] + S[2, 0]))
    assert mm.native_rgb(S, "bggr", 8)[0, 0, 1] == np.clip((acc + 8) >> 4, 0, 255)


@pytest.mark.parametrize("pattern", ORDERS)
@pytest.mark.parametrize("shape", [(3, 4), (5, 6), (8, 8), (11, 38)])
def test_constant_colour_field_comes_back(pattern, shape):
    """R=a, G=b, B=c everywhere, mosaicked with the rgb2bayer site map: demosaiced exactly, borders included"""
    H, W = shape
    sites = mm.site_map(pattern, H, W)
    for depth, (a, b, c) in ((8, (200, 17, 99)), (8, (0, 255, 128)), (12, (4095, 1000, 3)), (16, (65535, 0, 40000))):
        S = np.where(sites == "R", a, np.where(sites == "G", b, c))
        rgb = mm.native_rgb(S, pattern, depth)
        assert (rgb[..., 0] == a).all() and (rgb[..., 1] == b).all() and (rgb[..., 2] == c).all(), (depth, a, b, c)


def test_site_map_is_rgb2bayers():
    """the model's site map is the one of the oracle's rgb2bayer (raster order of the top-left 2x2)"""
    oracle = pytest.importorskip("oracle")
    W, H = 6, 4
    px = np.zeros((H, W, 4), np.uint8)
    px[..., 1], px[..., 2], px[..., 3] = 1, 2, 3                 # ARGB: R = 1, G = 2, B = 3
    for pattern in ORDERS:
        mosaic = np.asarray(oracle.rgb2bayer(px.reshape(H, 4 * W), W, pattern))[:, :W]
        sites = mm.site_map(pattern, H, W)
        assert (mosaic == np.vectorize({"R": 1, "G": 2, "B": 3}.get)(sites)).all(), pattern


def smooth_test_image(H=96, W=128, seed=11):
    """a luminance pattern (oriented sinusoids, fine enough to alias bilinearly) times slowly varying chroma, 8-bit"""
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W].astype(np.float64)
    lum = 0.5 + 0.2 * np.sin(2 * np.pi * (x * 0.11 + y * 0.04) + rng.uniform(0, 6)) \
        + 0.15 * np.sin(2 * np.pi * (x * 0.03 - y * 0.13) + rng.uniform(0, 6))
    chroma = [0.8 + 0.15 * np.sin(2 * np.pi * (x / W * f1 + y / H * f2) + ph)
              for f1, f2, ph in rng.uniform(0.3, 1.2, (3, 3))]
    return np.stack([np.clip(np.round(255 * lum * c), 0, 255) for c in chroma], axis=-1).astype(np.int64)


def psnr(a, b):
    mse = np.mean((a.astype(np.float64) - b.astype(np.float64)) ** 2)
    return 10 * np.log10(255.0 ** 2 / mse)


# The models give 38.1 dB (MHC) against 31.6 dB (bilinear) on this image for every order, borders included (6.5 dB:
# less than a quarter of the error power); a 5 dB margin is met by MHC and by nothing close to bilinear.
MHC_PSNR_MARGIN_DB = 5.0


@pytest.mark.parametrize("pattern", ORDERS)
def test_mhc_beats_bilinear_on_a_smooth_image(pattern):
    rgb = smooth_test_image()
    H, W, _ = rgb.shape
    sites = mm.site_map(pattern, H, W)
    S = np.where(sites == "R", rgb[..., 0], np.where(sites == "G", rgb[..., 1], rgb[..., 2]))
    p_mhc = psnr(mm.native_rgb(S, pattern, 8), rgb)
    p_bil = psnr(hm.native_rgb(S, pattern), rgb)
    assert p_mhc >= p_bil + MHC_PSNR_MARGIN_DB, (p_mhc, p_bil)


def test_bytes_in_bytes_out():
    """the frame-level entry: 8-bit mosaic -> BGRx and 12-bit big-endian words -> ARGB64 little-endian, through
    highbit_model's unpack / to_output"""
    rgb = smooth_test_image(12, 16)
    sites = mm.site_map("grbg", 12, 16)
    S = np.where(sites == "R", rgb[..., 0], np.where(sites == "G", rgb[..., 1], rgb[..., 2]))
    out = mm.bayer2rgb_mhc(S.astype(np.uint8), 16, 12, "grbg", "BGRx")
    native = mm.native_rgb(S, "grbg", 8)
    px = out.reshape(12, 16, 4)
    assert (px[..., 2] == native[..., 0]).all() and (px[..., 0] == native[..., 2]).all() and (px[..., 3] == 255).all()
    words = hm.pack(S << 4, big_endian=True)
    out16 = mm.bayer2rgb_mhc(words, 16, 12, "grbg", "ARGB64", bits=12, out16=True, src_big_endian=True)
    px16 = out16.reshape(12, 16, 8).view("<u2")
    assert (px16[..., 0] == 0xFFFF).all()
    assert (px16[..., 1:] == (mm.native_rgb(S << 4, "grbg", 12) << 4)).all()
