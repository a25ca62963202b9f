"""CPU tests of the histogram entry points at the boundaries: struct mibayer_hist and group `hist` in include/mibayer.h
and the harness, and the two pure host helpers against the NumPy model."""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import hist_model as hm
from test_colour_abi import prop_block
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: F401  (fixture)
from test_highbit_abi import inspect
from test_stats_abi import STATS as STATS_NAMES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HIST = ["mibayer_hist_device", "mibayer_set_hist", "mibayer_frame_hist", "mibayer_pool_set_hist",
        "mibayer_pool_frame_hist", "mibayer_hist_percentile", "mibayer_hist_exposure"]
COLOUR_NAMES = ["mibayer_colour_init", "mibayer_set_colour", "mibayer_get_colour", "mibayer_pool_set_colour",
                "mibayer_colour_matrix", "mibayer_colour_tone"]
PATTERNS = ["bggr", "gbrg", "grbg", "rggb"]


def random_hist(rng, top):
    hist = rng.integers(0, top, (4, 256)).astype(np.uint32)
    hist[rng.random((4, 256)) < 0.6] = 0
    return hist


def test_header_struct_and_group(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    assert re.search(r"#define MIBAYER_HIST_BINS 256\b", text)
    m = re.search(r"typedef struct mibayer_hist \{(.*?)\} mibayer_hist;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == ["uint32_t bin[4][MIBAYER_HIST_BINS]"]
    assert ctypes.sizeof(pkg.Hist) == 4096 == int(np.prod(pkg.HIST_SHAPE)) * pkg.HIST_DTYPE.itemsize
    assert pkg.HIST_SHAPE == (4, 256) and pkg.HIST_DTYPE == np.uint32
    names = lambda a, b: sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", text[text.index(a):text.index(b)])))  # noqa: E731
    assert names("* group hist:", "* group stats:") == sorted(HIST)
    assert names("* group stats:", "* group colour:") == sorted(STATS_NAMES)
    assert names("* group colour:", "END OF MIBAYER ABI GROUPS") == sorted(COLOUR_NAMES)
    assert "5, later additive: mosaic histogram" in text


def test_symbols_in_both_libraries_and_the_harness(pkg, lab_pkg):
    for p in (pkg, lab_pkg):
        assert all(name in p.ABI and hasattr(p.lib(), name) for name in HIST)
    for name in ("Hist", "HIST_DTYPE", "hist_percentile", "hist_exposure"):
        assert hasattr(pkg, name)
    for name in ("hist_device", "set_hist", "frame_hist", "hist_batch_via_device"):
        assert hasattr(pkg.Context, name)
    for name in ("set_hist", "frame_hist"):
        assert hasattr(pkg.Pool, name)


def test_null_handles_and_pointers(pkg):
    L = pkg.lib()
    hist = np.zeros((4, 256), np.uint32)
    hist[:, 7] = 1
    b, x = ctypes.c_int(0), ctypes.c_double(0.0)
    assert L.mibayer_set_hist(None, 1, 0, 0, 0, 0) == pkg.ERR_ARG
    assert L.mibayer_frame_hist(None, hist.ctypes.data) == pkg.ERR_ARG
    assert L.mibayer_pool_set_hist(None, 1, 0, 0, 0, 0) == pkg.ERR_ARG
    assert L.mibayer_pool_frame_hist(None, hist.ctypes.data) == pkg.ERR_ARG
    assert L.mibayer_hist_device(None, hist.ctypes.data, 0, 1, 0, 0, 0, 0, hist.ctypes.data, None) == pkg.ERR_ARG
    assert L.mibayer_hist_percentile(hist.ctypes.data, 3, 1, 0.5, ctypes.byref(b)) == 1 and b.value == 7
    assert L.mibayer_hist_percentile(None, 3, 1, 0.5, ctypes.byref(b)) == pkg.ERR_ARG
    assert L.mibayer_hist_percentile(hist.ctypes.data, 3, 1, 0.5, None) == pkg.ERR_ARG
    for pattern in (-1, 4):
        assert L.mibayer_hist_percentile(hist.ctypes.data, pattern, 1, 0.5, ctypes.byref(b)) == pkg.ERR_ARG
    for colour in (-1, 4):
        assert L.mibayer_hist_percentile(hist.ctypes.data, 3, colour, 0.5, ctypes.byref(b)) == pkg.ERR_ARG
    ok = lambda **kw: L.mibayer_hist_exposure(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("hist", hist.ctypes.data), ("pattern", 3), ("depth", 8), ("black", None), ("gains", None),
        ("fraction", ctypes.c_double(0.99)), ("target", ctypes.c_double(0.9)), ("max_gain", ctypes.c_double(4.0)),
        ("out", ctypes.byref(x)))])
    assert ok() == 1 and x.value == 4.0
    assert ok(hist=None) == pkg.ERR_ARG and ok(out=None) == pkg.ERR_ARG
    for depth in (0, 7, 9, 11, 15, 17, 18):
        assert ok(depth=depth) == pkg.ERR_ARG
    for depth in (8, 10, 12, 14, 16):
        assert ok(depth=depth) == 1
    for target in (0.0, -0.5, 1.0001, math.nan):
        assert ok(target=ctypes.c_double(target)) == pkg.ERR_ARG
    assert ok(target=ctypes.c_double(1.0)) == 1
    for max_gain in (0.99, 16.0, math.nan):
        assert ok(max_gain=ctypes.c_double(max_gain)) == pkg.ERR_ARG
    assert ok(max_gain=ctypes.c_double(1.0)) == 1 and ok(max_gain=ctypes.c_double(15.99)) == 1
    for fraction in (-0.01, 1.01, math.nan):
        assert ok(fraction=ctypes.c_double(fraction)) == pkg.ERR_ARG
    assert ok(pattern=4) == pkg.ERR_ARG


@pytest.mark.parametrize("pattern", PATTERNS)
def test_percentile_matches_the_model(pkg, pattern):
    rng = np.random.default_rng(PATTERNS.index(pattern) + 40)
    for trial in range(20):
        hist = random_hist(rng, (10, 70000, 1 << 32)[trial % 3])
        for colour in range(4):
            for fraction in (0.0, 1.0, 0.5, 0.99, float(rng.random())):
                assert pkg.hist_percentile(hist, pattern, colour, fraction) \
                    == hm.percentile_bin(hist, pattern, colour, fraction), (trial, colour, fraction)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_exposure_matches_the_model(pkg, pattern):
    rng = np.random.default_rng(PATTERNS.index(pattern) + 50)
    for trial in range(40):
        depth = (8, 10, 12, 14, 16)[trial % 5]
        hist = random_hist(rng, 5000)
        if trial % 4 == 0:
            hist[:, 128:] = 0           # a dark frame: the factor is above 1
        black = None if trial % 2 else tuple(rng.uniform(0, (1 << depth) / 8, 3))
        gains = None if trial % 3 else tuple(rng.uniform(0.2, 4, 3))
        args = (float(rng.uniform(0.5, 1)), float(rng.uniform(0.1, 1)), float(rng.uniform(1, 15.99)))
        # the same doubles in the same order: equal to the last bit
        assert pkg.hist_exposure(hist, pattern, depth, black, gains, *args) \
            == hm.exposure(hist, pattern, depth, black, gains, *args), (trial, depth)


def test_fraction_edges_and_nan(pkg):
    hist = np.zeros((4, 256), np.uint32)
    hist[0, 5], hist[0, 9], hist[0, 200] = 3, 1, 1
    assert pkg.hist_percentile(hist, "rggb", 0, 0.0) == (1, 5)          # rank max (1, 0) = 1
    assert pkg.hist_percentile(hist, "rggb", 0, 0.6) == (1, 5) and pkg.hist_percentile(hist, "rggb", 0, 0.61) == (1, 9)
    assert pkg.hist_percentile(hist, "rggb", 0, 1.0) == (1, 200)
    with pytest.raises(pkg.MibayerError):
        pkg.hist_percentile(hist, "rggb", 0, math.nan)


def test_an_empty_colour(pkg):
    hist = np.zeros((4, 256), np.uint32)
    hist[0, 100] = hist[1, 100] = hist[2, 100] = 10      # rggb: no blue
    assert pkg.hist_percentile(hist, "rggb", 2, 0.5) == (0, -1)
    assert pkg.hist_percentile(hist, "rggb", 1, 0.5) == (1, 100) and pkg.hist_percentile(hist, "rggb", 3, 0.5) == (1, 100)
    assert pkg.hist_exposure(hist, "rggb", 8, None, None, 0.99, 0.9, 4.0) == (0, 1.0)
    # gbrg reads the same table as G B R G: the empty site is a green one, and the other green site carries G
    assert pkg.hist_exposure(hist, "gbrg", 8, None, None, 0.99, 0.9, 4.0) == (1, 0.9 / (100.0 / 255.0))
    hist[3, 100] = 1
    assert pkg.hist_exposure(hist, "rggb", 8, None, None, 0.99, 0.9, 4.0) == (1, 0.9 / (100.0 / 255.0))


def test_black_at_the_percentile_value_and_at_max(pkg):
    hist = np.zeros((4, 256), np.uint32)
    hist[:, 64] = 100                   # 12-bit: v = 65 * 16 - 1 = 1039
    expo = lambda black: pkg.hist_exposure(hist, "grbg", 12, black, None, 0.99, 0.5, 8.0)  # noqa: E731
    assert expo((1038, 1039, 2000)) == (1, 0.5 / (1.0 / (4095.0 - 1038.0)))[:1] + (8.0,)       # clamped above
    assert expo((1039, 1039, 1039)) == (0, 1.0) and expo((1040, 3000, 1039)) == (0, 1.0)        # level 0
    assert expo((0, 0, 4095)) == (0, 1.0) and expo((4096, 0, 0)) == (0, 1.0)                    # black >= max
    assert expo((0, 0, 4094)) == (1, 0.5 / (1039.0 / 4095.0))
    for black in ((1038, 1039, 2000), (1039, 1039, 1039), (0, 0, 4095), (0, 0, 4094)):
        assert expo(black) == hm.exposure(hist, "grbg", 12, black, None, 0.99, 0.5, 8.0)


def test_both_clamps(pkg):
    hist = np.zeros((4, 256), np.uint32)
    hist[:, 0] = 1                      # level 0 at depth 8 (v = 0): no answer
    assert pkg.hist_exposure(hist, "rggb", 8, None, None, 0.99, 0.9, 4.0) == (0, 1.0)
    hist[:, 0], hist[:, 1] = 0, 1       # level 1 / 255: far above max_gain
    assert pkg.hist_exposure(hist, "rggb", 8, None, None, 0.99, 0.9, 15.99) == (1, 15.99)
    assert pkg.hist_exposure(hist, "rggb", 8, None, None, 0.99, 0.9, 1.0) == (1, 1.0)
    hist[:, 1], hist[:, 255] = 0, 1     # level gains * 1: 0.01 / 15 is under 1 / 16
    assert pkg.hist_exposure(hist, "rggb", 8, None, (15.0, 1.0, 1.0), 0.99, 0.01, 4.0) == (1, 1.0 / 16)
    assert pkg.hist_exposure(hist, "rggb", 8, None, None, 0.99, 0.5, 4.0) == (1, 0.5)


def test_counts_above_2_to_the_31(pkg):
    hist = np.zeros((4, 256), np.uint32)
    hist[1, 10], hist[2, 10] = 0xFFFFFFFF, 0xFFFFFFFF    # rggb G: 2^33 - 2 pooled, past 32 bits
    hist[1, 20] = 0x80000001
    hist[0, 3], hist[3, 4] = 0xFFFFFFFF, 0x80000000
    for colour in range(4):
        for fraction in (0.0, 0.5, 0.79, 0.81, 1.0):
            got = pkg.hist_percentile(hist, "rggb", colour, fraction)
            assert got == hm.percentile_bin(hist, "rggb", colour, fraction), (colour, fraction)
    assert pkg.hist_percentile(hist, "rggb", 1, 0.79) == (1, 10) and pkg.hist_percentile(hist, "rggb", 1, 0.81) == (1, 20)
    assert pkg.hist_percentile(hist, "rggb", 3, 0.2) == (1, 3)


@needs_gst
def test_inspect_lists_the_exposure_properties(plugin, tmp_path):  # noqa: F811
    for element in ("bayer2rgb", "hipbayer2rgb"):
        out = inspect(tmp_path, element)
        expo = prop_block(out, "exposure")
        assert expo is not None and 'Default: 0, "manual"' in expo and "(0): manual" in expo and "(1): auto" in expo, expo
        target, speed, ceiling = (" ".join(prop_block(out, name).split()) for name in ("ae-target", "ae-speed", "ae-max-gain"))
        assert re.search(r"Double\. Range: \S+ - 1 Default: 0\.9\b", target), target
        assert re.search(r"Double\. Range: \S+ - 1 Default: 0\.25\b", speed), speed
        assert re.search(r"Double\. Range: 1 - 15\.99 Default: 4\b", ceiling), ceiling
        for name in ("ae-target", "ae-speed"):
            lo = float(re.search(r"Range: (\S+) - 1 ", " ".join(prop_block(out, name).split())).group(1))
            assert 0.0 < lo < 1e-300           # (0, 1]
        for block in (expo, target, speed, ceiling):
            assert "changeable only in NULL or READY state" in block
    r2b = inspect(tmp_path, "rgb2bayer")
    for name in ("exposure", "ae-target", "ae-speed", "ae-max-gain"):
        assert prop_block(r2b, name) is None, name


@needs_gst
def test_mock_rig_defaults_convert_and_auto_exposure_fails_cleanly(rig, tmp_path):  # noqa: F811
    """The mock library has no histogram entry points.  With default properties -- spelled out or not -- the elements
    call none of them and convert as before; exposure=auto ends in an element error, not in a crash."""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=7).tofile(inp)
    defaults = "exposure=manual ae-target=0.5 ae-speed=1 ae-max-gain=8"
    for launch in ("bayer2rgb", "bayer2rgb " + defaults, "bayer2rgb inflight=3 devices=0,0 " + defaults,
                   "hipupload ! hipbayer2rgb " + defaults + " ! hipdownload"):
        kv = run(rig, "convert", launch, B2R % ("gbrg", w, h), inp, 260 * h, outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n) and kv["errors"] == "0", (launch, kv)
        seq, fill = stamps(outp, n, 4 * w * h)
        assert fill == list(range(7, 7 + n)) and seq == list(range(n)), launch
    for launch in ("bayer2rgb exposure=auto", "bayer2rgb inflight=3 devices=0,0 exposure=auto",
                   "hipupload ! hipbayer2rgb exposure=auto ! hipdownload"):
        kv = run(rig, "caps", launch, B2R % ("gbrg", w, h), 260 * h)
        assert int(kv["errors"]) >= 1 and kv["caps_accepted"] == "0", (launch, kv)
