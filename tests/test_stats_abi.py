"""CPU tests of the statistics entry points at the boundaries: struct mibayer_stats_zone and group `stats` in
include/mibayer.h and the harness, and the pure host helper mibayer_stats_grey_world against the NumPy model."""
import ctypes
import os
import re

import numpy as np
import pytest

import stats_model as sm
from test_colour_abi import prop_block
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_highbit_abi import inspect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STATS = ["mibayer_stats_device", "mibayer_set_stats", "mibayer_frame_stats", "mibayer_pool_set_stats",
         "mibayer_pool_frame_stats", "mibayer_stats_grey_world"]


def zones(*per_zone):
    """per_zone: (sums[4], counts[4])"""
    z = np.zeros(len(per_zone), sm.STATS_DTYPE)
    for i, (s, n) in enumerate(per_zone):
        z["sum"][i], z["count"][i] = s, n
    return z


def test_header_struct_and_group(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    m = re.search(r"typedef struct mibayer_stats_zone \{(.*?)\} mibayer_stats_zone;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == [
        "uint64_t sum[4]", "uint32_t count[4]", "uint32_t clipped[4]"]
    assert ctypes.sizeof(pkg.StatsZone) == 64 == pkg.STATS_DTYPE.itemsize == sm.STATS_DTYPE.itemsize
    assert pkg.STATS_DTYPE == sm.STATS_DTYPE
    block = text[text.index("* group stats:"):text.index("* group colour:")]
    assert sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block))) == sorted(STATS)
    assert all(name in pkg.ABI and hasattr(pkg.lib(), name) for name in STATS)
    for name in ("StatsZone", "stats_grey_world"):
        assert hasattr(pkg, name)
    for name in ("stats_device", "set_stats", "frame_stats"):
        assert hasattr(pkg.Context, name)
    for name in ("set_stats", "frame_stats"):
        assert hasattr(pkg.Pool, name)


@pytest.mark.parametrize("pattern", ["bggr", "gbrg", "grbg", "rggb"])
def test_grey_world_matches_the_model(pkg, pattern):
    rng = np.random.default_rng(sm.SITE_COLOUR[pattern][0] + 10)
    for trial in range(20):
        z = np.zeros(int(rng.integers(1, 40)), sm.STATS_DTYPE)
        z["count"] = rng.integers(0, 70000, z["count"].shape)
        z["sum"] = z["count"].astype(np.uint64) * rng.integers(1, 65536, z["count"].shape).astype(np.uint64)
        black = (0.0, 0.0, 0.0) if trial % 2 else tuple(rng.uniform(0, 300, 3))
        ok, gains = pkg.stats_grey_world(z, pattern, None if trial % 2 else black)
        want_ok, want = sm.grey_world(z, pattern, black)
        assert ok == want_ok and gains == pytest.approx(want, rel=1e-12), (trial, gains, want)
        assert gains[1] == 1.0


def test_grey_world_sums_past_32_bits(pkg):
    z = zones(([3 << 40, 5 << 40, 5 << 40, 9 << 40], [1 << 24] * 4))
    ok, gains = pkg.stats_grey_world(z, "rggb")
    assert ok == 1 and gains == pytest.approx((5.0 / 3.0, 1.0, 5.0 / 9.0), rel=1e-12)


def test_grey_world_refuses_empty_and_dark_colours(pkg):
    # rggb: no blue samples at all
    assert pkg.stats_grey_world(zones(([100, 100, 100, 0], [1, 1, 1, 0])), "rggb") == (0, (1.0, 1.0, 1.0))
    # one green site empty is fine: the other one carries G
    ok, gains = pkg.stats_grey_world(zones(([100, 0, 50, 25], [1, 0, 1, 1])), "rggb")
    assert ok == 1 and gains == pytest.approx((0.5, 1.0, 2.0), rel=1e-12)
    # a mean at or under the black level
    z = zones(([100, 100, 100, 100], [1, 1, 1, 1]))
    assert pkg.stats_grey_world(z, "rggb", (100, 0, 0)) == (0, (1.0, 1.0, 1.0))
    assert pkg.stats_grey_world(z, "rggb", (0, 0, 101)) == (0, (1.0, 1.0, 1.0))
    assert pkg.stats_grey_world(z, "rggb", (0, 200, 0)) == (0, (1.0, 1.0, 1.0))
    assert pkg.stats_grey_world(z, "rggb", (99, 0, 0))[0] == 1


def test_grey_world_clamps(pkg):
    ok, gains = pkg.stats_grey_world(zones(([1, 1000, 1000, 100000], [1, 1, 1, 1])), "rggb")
    assert ok == 1 and gains == (15.99, 1.0, 1.0 / 16)
    ok, gains = pkg.stats_grey_world(zones(([100000, 1000, 1000, 1], [1, 1, 1, 1])), "rggb")
    assert ok == 1 and gains == (1.0 / 16, 1.0, 15.99)
    ok, gains = pkg.stats_grey_world(zones(([1000, 15990, 15990, 16000], [1, 1, 1, 1])), "rggb")
    assert ok == 1 and gains == pytest.approx((15.99, 1.0, 15990.0 / 16000.0), rel=1e-12)


def test_grey_world_argument_errors(pkg):
    L = pkg.lib()
    z = zones(([1, 1, 1, 1], [1, 1, 1, 1]))
    gains = (ctypes.c_double * 3)()
    assert L.mibayer_stats_grey_world(z.ctypes.data, 1, 3, None, gains) == 1
    assert L.mibayer_stats_grey_world(None, 1, 3, None, gains) == pkg.ERR_ARG
    assert L.mibayer_stats_grey_world(z.ctypes.data, 1, 3, None, None) == pkg.ERR_ARG
    assert L.mibayer_stats_grey_world(z.ctypes.data, 0, 3, None, gains) == pkg.ERR_ARG
    for pattern in (-1, 4, 100):
        assert L.mibayer_stats_grey_world(z.ctypes.data, 1, pattern, None, gains) == pkg.ERR_ARG


def test_null_handles(pkg):
    L = pkg.lib()
    out = np.zeros(1, sm.STATS_DTYPE)
    assert L.mibayer_set_stats(None, 1, 1, 0, 255) == pkg.ERR_ARG
    assert L.mibayer_frame_stats(None, out.ctypes.data, 1) == pkg.ERR_ARG
    assert L.mibayer_pool_set_stats(None, 1, 1, 0, 255) == pkg.ERR_ARG
    assert L.mibayer_pool_frame_stats(None, out.ctypes.data, 1) == pkg.ERR_ARG
    assert L.mibayer_stats_device(None, out.ctypes.data, 0, 1, 1, 1, 0, 255, out.ctypes.data, None) == pkg.ERR_ARG


@needs_gst
def test_inspect_lists_white_balance_and_awb_speed(plugin, tmp_path):  # noqa: F811
    for element in ("bayer2rgb", "hipbayer2rgb"):
        out = inspect(tmp_path, element)
        wb = prop_block(out, "white-balance")
        assert wb is not None and 'Default: 0, "manual"' in wb and "(0): manual" in wb and "(1): grey-world" in wb, wb
        speed = " ".join(prop_block(out, "awb-speed").split())
        assert re.search(r"Double\. Range: \S+ - 1 Default: 0\.25\b", speed), speed
        for block in (wb, speed):
            assert "changeable only in NULL or READY state" in block
    r2b = inspect(tmp_path, "rgb2bayer")
    assert prop_block(r2b, "white-balance") is None and prop_block(r2b, "awb-speed") is None
