"""CPU tests of the focus entry points at the boundaries: struct mibayer_focus_zone and group `focus` in
include/mibayer.h and the harness, the argument errors that need no device, and the pure host helper
mibayer_focus_score against the NumPy model to the last bit."""
import ctypes
import math
import os
import re
import subprocess

import numpy as np
import pytest

import focus_model as fm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FOCUS = ["mibayer_focus_device", "mibayer_set_focus", "mibayer_frame_focus", "mibayer_pool_set_focus",
         "mibayer_pool_frame_focus", "mibayer_focus_score"]
PATTERNS = ["bggr", "gbrg", "grbg", "rggb"]


def test_header_struct_and_group(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    m = re.search(r"typedef struct mibayer_focus_zone \{(.*?)\} mibayer_focus_zone;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == [
        "uint64_t h[4]", "uint64_t v[4]", "uint32_t nh[4]", "uint32_t nv[4]"]
    assert ctypes.sizeof(pkg.FocusZone) == 96 == pkg.FOCUS_DTYPE.itemsize == fm.FOCUS_DTYPE.itemsize
    assert pkg.FOCUS_DTYPE == fm.FOCUS_DTYPE
    block = text[text.index("* group focus:"):text.index("* group nr:")]
    assert sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block))) == sorted(FOCUS)
    assert "5, later additive: mosaic focus statistics" in text


def test_symbols_in_both_libraries_and_the_harness(pkg, lab_pkg):
    for p in (pkg, lab_pkg):
        assert all(name in p.ABI and hasattr(p.lib(), name) for name in FOCUS)
    for name in ("FocusZone", "FOCUS_DTYPE", "focus_score"):
        assert hasattr(pkg, name)
    for name in ("focus_device", "set_focus", "frame_focus", "focus_batch_via_device"):
        assert hasattr(pkg.Context, name)
    for name in ("set_focus", "frame_focus"):
        assert hasattr(pkg.Pool, name)


def test_the_export_list(pkg):
    """the six entry points are dynamic symbols of the product library, and the ABI is 123 functions: the header's
    groups, the harness' table and the library's symbol table"""
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split()[-1].startswith("mibayer_"))
    assert set(FOCUS) <= set(exported)
    assert len(exported) == 123 == len(pkg.ABI) and exported == sorted(pkg.ABI)
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    block = text[text.index("MIBAYER ABI GROUPS"):text.index("END OF MIBAYER ABI GROUPS")]
    grouped = set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block)) - {"mibayer_internal_"}
    assert sorted(n for n in grouped if n in pkg.ABI) == exported


def test_null_handles_and_pointers(pkg):
    L = pkg.lib()
    out = np.zeros(1, fm.FOCUS_DTYPE)
    assert L.mibayer_set_focus(None, 1, 1, 0) == pkg.ERR_ARG
    assert L.mibayer_set_focus(None, 0, 0, 0) == pkg.ERR_ARG
    assert L.mibayer_frame_focus(None, out.ctypes.data, 1) == pkg.ERR_ARG
    assert L.mibayer_pool_set_focus(None, 1, 1, 0) == pkg.ERR_ARG
    assert L.mibayer_pool_frame_focus(None, out.ctypes.data, 1) == pkg.ERR_ARG
    assert L.mibayer_focus_device(None, out.ctypes.data, 0, 1, 1, 1, 0, out.ctypes.data, None) == pkg.ERR_ARG


def test_score_argument_errors(pkg):
    L = pkg.lib()
    z = np.zeros(2, fm.FOCUS_DTYPE)
    z["h"][:], z["nh"][:] = 6, 2
    x = ctypes.c_double(-1.0)
    ok = lambda **kw: L.mibayer_focus_score(*[kw.get(k, d) for k, d in (  # noqa: E731
        ("zones", z.ctypes.data), ("nzones", 2), ("pattern", 3), ("colour", 1), ("weights", None),
        ("score", ctypes.byref(x)))])
    assert ok() == 1 and x.value == 3.0
    assert ok(zones=None) == pkg.ERR_ARG and ok(score=None) == pkg.ERR_ARG
    for nzones in (0, -1):
        assert ok(nzones=nzones) == pkg.ERR_ARG
    for pattern in (-1, 4, 100):
        assert ok(pattern=pattern) == pkg.ERR_ARG
    for colour in (-1, 4):
        assert ok(colour=colour) == pkg.ERR_ARG
    for colour in range(4):
        assert ok(colour=colour) == 1 and x.value == 3.0
    for bad in (-1.0, -0.0001, math.nan, math.inf, -math.inf):
        for where in (0, 1):
            w = np.ones(2)
            w[where] = bad
            assert ok(weights=w.ctypes.data) == pkg.ERR_ARG, bad
    w = np.array([0.0, 2.5])
    assert ok(weights=w.ctypes.data) == 1 and x.value == 3.0
    w = np.zeros(2)
    x.value = -1.0
    assert ok(weights=w.ctypes.data) == 0 and x.value == 0.0
    with pytest.raises(pkg.MibayerError):
        pkg.focus_score(z, "rggb", 7)


def test_score_of_empty_zones_is_zero(pkg):
    z = np.zeros(5, fm.FOCUS_DTYPE)
    assert pkg.focus_score(z, "rggb") == (0, 0.0)
    z["h"][2, 0], z["nh"][2, 0] = 10, 4                  # rggb: red only
    assert pkg.focus_score(z, "rggb", 1) == (0, 0.0) and pkg.focus_score(z, "rggb", 2) == (0, 0.0)
    assert pkg.focus_score(z, "rggb", 0) == (1, 2.5) and pkg.focus_score(z, "rggb", 3) == (1, 2.5)
    assert pkg.focus_score(z, "bggr", 2) == (1, 2.5)


@pytest.mark.parametrize("pattern", PATTERNS)
def test_score_matches_the_model_to_the_last_bit(pkg, pattern):
    rng = np.random.default_rng(PATTERNS.index(pattern) + 60)
    for trial in range(40):
        z = np.zeros(int(rng.integers(1, 50)), fm.FOCUS_DTYPE)
        top = (50, 70000, 1 << 32)[trial % 3]
        z["nh"] = rng.integers(0, top, z["nh"].shape)
        z["nv"] = rng.integers(0, top, z["nv"].shape)
        z["h"] = z["nh"].astype(np.uint64) * rng.integers(0, 2 * 65535 + 1, z["nh"].shape).astype(np.uint64)
        z["v"] = z["nv"].astype(np.uint64) * rng.integers(0, 2 * 65535 + 1, z["nv"].shape).astype(np.uint64)
        if trial % 5 == 0:
            z["nh"][rng.random(z["nh"].shape) < 0.7] = 0
        for colour in range(4):
            weights = None if trial % 2 else rng.uniform(0, 3, z.size) * (rng.random(z.size) < 0.8)
            got, want = pkg.focus_score(z, pattern, colour, weights), fm.score(z, pattern, colour, weights)
            assert got == want, (trial, colour, got, want)


def test_score_from_a_frame(pkg):
    """through the whole model: the score of a sharp frame is above that of its blurred copy, in both"""
    rng = np.random.default_rng(7)
    S = rng.integers(0, 256, (37, 66))
    B = S.copy()
    B[:, 2:-2] = (S[:, :-4] + 2 * S[:, 2:-2] + S[:, 4:] + 2) // 4       # a same-site blur
    zs, zb = fm.zone_focus(S, 3, 5, 0, 255), fm.zone_focus(B, 3, 5, 0, 255)
    for colour in range(4):
        s, b = pkg.focus_score(zs, "grbg", colour), pkg.focus_score(zb, "grbg", colour)
        assert s == fm.score(zs, "grbg", colour) and b == fm.score(zb, "grbg", colour)
        assert s[0] == b[0] == 1 and b[1] < s[1]


# -- the elements (no device: gst-inspect, and the mock library of tests/check) -----------------------------------------

from test_colour_abi import prop_block  # noqa: E402
from test_gst_element import needs_gst, plugin  # noqa: E402,F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: E402,F401  (fixture)
from test_highbit_abi import inspect  # noqa: E402


@needs_gst
def test_inspect_lists_the_focus_properties(plugin, tmp_path):  # noqa: F811
    out = inspect(tmp_path, "bayer2rgb")
    for name in ("focus-zones-x", "focus-zones-y"):
        block = " ".join(prop_block(out, name).split())
        assert re.search(r"Integer\. Range: 0 - 64 Default: 0\b", block), block
        assert "changeable only in NULL or READY state" in block
    thr = " ".join(prop_block(out, "focus-threshold").split())
    assert re.search(r"Unsigned Integer\. Range: 0 - 4294967295 Default: 0\b", thr), thr
    r2b = inspect(tmp_path, "rgb2bayer")
    for name in ("focus-zones-x", "focus-zones-y", "focus-threshold"):
        assert prop_block(r2b, name) is None, name


@needs_gst
def test_mock_rig_defaults_convert_and_a_focus_request_fails_cleanly(rig, tmp_path):  # noqa: F811
    """The mock library has no focus entry points.  With default properties -- spelled out or not -- the element calls
    none of them and converts as before; a focus grid ends in an element error, not in a crash."""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=7).tofile(inp)
    defaults = "focus-zones-x=0 focus-zones-y=0 focus-threshold=0"
    for launch in ("bayer2rgb", "bayer2rgb " + defaults, "bayer2rgb focus-zones-x=4 focus-threshold=9",
                   "bayer2rgb inflight=3 devices=0,0 " + defaults):
        kv = run(rig, "convert", launch, B2R % ("gbrg", w, h), inp, 260 * h, outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n) and kv["errors"] == "0", (launch, kv)
        seq, fill = stamps(outp, n, 4 * w * h)
        assert fill == list(range(7, 7 + n)) and seq == list(range(n)), launch
    for launch in ("bayer2rgb focus-zones-x=3 focus-zones-y=5", "bayer2rgb inflight=3 devices=0,0 focus-zones-x=1 focus-zones-y=1"):
        kv = run(rig, "caps", launch, B2R % ("gbrg", w, h), 260 * h)
        assert int(kv["errors"]) >= 1 and kv["caps_accepted"] == "0", (launch, kv)
