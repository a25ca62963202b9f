"""CPU tests of the fused colour stage at the boundaries: MIBAYER_FLAG_COLOUR and struct mibayer_colour in
include/mibayer.h and the harness, what mibayer_create makes of the flag, the two pure host helpers
(mibayer_colour_matrix / mibayer_colour_tone), the argument errors of the entry points, and the elements' seven
properties (gst-inspect, and the mock rig of test_gst_element_logic.py, whose test double has no colour stage)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: F401  (fixture)
from test_highbit_abi import create, inspect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROPS = ("black-level", "red-gain", "green-gain", "blue-gain", "ccm", "tone-curve", "gamma")


def test_header_defines_the_flag_and_the_struct(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_FLAG_COLOUR \(1u << 19\)", text)
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    for name, value in (("LINEAR", 0), ("SRGB", 1), ("GAMMA", 2)):
        assert re.search(r"#define MIBAYER_TONE_%s %d\b" % (name, value), text), name
    m = re.search(r"typedef struct mibayer_colour \{(.*?)\} mibayer_colour;", text, re.S)
    assert m
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    fields = [" ".join(f.split()) for f in body.split(";") if f.strip()]
    assert fields == ["uint32_t struct_size", "int32_t black[3]", "int32_t matrix[9]", "int32_t has_tone",
                      "uint32_t tone[257]"]
    assert ctypes.sizeof(pkg.Colour) == 4 + 12 + 36 + 4 + 4 * 257
    assert pkg.FLAG_COLOUR == 1 << 19 and (pkg.TONE_LINEAR, pkg.TONE_SRGB, pkg.TONE_GAMMA) == (0, 1, 2)
    assert pkg.make_cfg(64, 48, colour=True).flags == pkg.FLAG_COLOUR
    assert pkg.make_cfg(64, 48, colour=pkg.Colour()).flags == pkg.FLAG_COLOUR
    assert pkg.make_cfg(64, 48).flags == 0 and pkg.make_cfg(64, 48, colour=False).flags == 0
    assert pkg.make_cfg(64, 48, "bggr", "ARGB64", bits=12, method="mhc", colour=True).flags \
        == pkg.FLAG_COLOUR | pkg.FLAG_MHC | pkg.FLAG_SRC_BITS(12) | pkg.FLAG_DST_16BIT
    # the group of the ABI comment
    block = text[text.index("* group colour:"):text.index("END OF MIBAYER ABI GROUPS")]
    assert sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block))) == sorted(
        ["mibayer_colour_init", "mibayer_set_colour", "mibayer_get_colour", "mibayer_pool_set_colour",
         "mibayer_colour_matrix", "mibayer_colour_tone"])


def test_colour_cfg_validation(pkg):
    ok_or_nodev = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    for method in ("bilinear", "mhc"):
        for fmt in ("RGBx", "BGRx", "xRGB", "xBGR"):
            assert create(pkg, mk(64, 48, "gbrg", fmt, method=method, colour=True)) in ok_or_nodev, fmt
        for bits in (0, 10, 12, 14, 16):
            for sbe in ((False,) if bits == 0 else (False, True)):
                for out16, dbe in ((False, False), (True, False), (True, True)):
                    fmt = "ARGB64" if out16 else "BGRx"
                    cfg = mk(64, 48, "rggb", fmt, bits=bits, src_big_endian=sbe, out16=out16, dst_big_endian=dbe,
                             method=method, colour=True)
                    assert create(pkg, cfg) in ok_or_nodev, (method, bits, sbe, out16, dbe)
        assert create(pkg, mk(64, 48, flags=pkg.FLAG_HIPGRAPH, method=method, colour=True)) in ok_or_nodev
        assert create(pkg, mk(4, 3, method=method, colour=True)) in ok_or_nodev
        # geometry, strides and layouts: those of the same cfg without the flag
        assert create(pkg, mk(66, 48, src_stride=68, dst_stride=264, method=method, colour=True)) in ok_or_nodev
        assert create(pkg, mk(66, 48, bits=12, src_stride=136, out16=True, dst_stride=536, method=method,
                              colour=True)) in ok_or_nodev
        for kw in (dict(src_stride=66), dict(dst_stride=260), dict(width=63), dict(width=2), dict(height=2)):
            w = kw.pop("width", 66)
            h = kw.pop("height", 48)
            assert create(pkg, mk(w, h, method=method, colour=True, **kw)) == pkg.ERR_GEOMETRY, (w, h, kw)
        assert create(pkg, mk(64, 48, fmt=(0, 2, 1), method=method, colour=True)) == pkg.ERR_LAYOUT
        # refused: a kernel variant
        for v in (1, 2, 3):
            assert create(pkg, mk(64, 48, variant=v, method=method, colour=True)) == pkg.ERR_ARG, v
            assert create(pkg, mk(64, 48, variant=v, bits=12, method=method, colour=True)) == pkg.ERR_ARG, v
    # refused: rgb2bayer
    assert create(pkg, mk(64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER, colour=True)) == pkg.ERR_ARG
    # the neighbouring bits stay unknown
    for bit in (17, 18, 20, 24):
        assert create(pkg, mk(64, 48, flags=1 << bit)) == pkg.ERR_ARG, bit
        assert create(pkg, mk(64, 48, flags=1 << bit, colour=True)) == pkg.ERR_ARG, bit
    # the plan selectors describe the bilinear 8-bit kernel only
    sel, swap = (ctypes.c_uint32 * 4)(), ctypes.c_int()
    cfg = mk(64, 48, colour=True)
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.ERR_ARG


def test_colour_init_is_the_identity(pkg):
    c = pkg.Colour(black=(7, 8, 9), matrix=range(9), tone=range(257))
    pkg.lib().mibayer_colour_init(ctypes.byref(c))
    assert c.struct_size == ctypes.sizeof(pkg.Colour)
    assert c.black[:] == [0, 0, 0] and c.matrix[:] == [4096, 0, 0, 0, 4096, 0, 0, 0, 4096] and c.has_tone == 0
    assert not any(c.tone[:])
    pkg.lib().mibayer_colour_init(None)


def test_colour_matrix_rounds_like_the_formula(pkg):
    assert pkg.colour_matrix() == [4096, 0, 0, 0, 4096, 0, 0, 0, 4096]
    assert pkg.colour_matrix((1.5, 1.0, 0.75)) == [6144, 0, 0, 0, 4096, 0, 0, 0, 3072]
    ccm = (1.5, -0.25, -0.25, -0.5, 1.75, -0.25, 0.0, -0.5, 1.5)                   # rows sum to 1: greys stay grey
    assert pkg.colour_matrix((1.0, 1.0, 1.0), ccm) == [6144, -1024, -1024, -2048, 7168, -1024, 0, -2048, 6144]
    # gains scale the COLUMNS (ccm x diag(gains)): input channel j is multiplied by gains[j] first
    assert pkg.colour_matrix((1.5, 1.0, 0.75), ccm) == [9216, -1024, -768, -3072, 7168, -768, 0, -2048, 4608]
    # rounding to nearest, halves away from zero
    assert pkg.colour_matrix((1.0, 1.0, 1.0), (0.5 / 4096, -0.5 / 4096, 1.4 / 4096, -1.6 / 4096, 0, 0, 0, 0, 0))[:4] \
        == [1, -1, 1, -2]
    rng = np.random.default_rng(2)
    for _ in range(20):
        g, m = rng.uniform(0, 3, 3), rng.uniform(-2, 2, 9)
        want = np.round(m.reshape(3, 3) * g[None, :] * 4096).astype(int).reshape(-1)
        got = np.array(pkg.colour_matrix(g, m))
        assert np.abs(got - want).max() <= 1 and (got == want).mean() > 0.8       # numpy rounds halves to even
    # the range: |entry| <= 65535 / 4096 = 15.9998
    assert pkg.colour_matrix((15.99, 15.99, 15.99))[0] == round(15.99 * 4096)
    L = pkg.lib()
    out = (ctypes.c_int32 * 9)(*([77] * 9))
    for gains, m in (((16.0, 1, 1), None), ((4.0, 1, 1), (4.0, 0, 0, 0, 1, 0, 0, 0, 1)), ((1, 1, 1), (0, 0, -16.0, 0, 1, 0, 0, 0, 1)),
                     ((float("nan"), 1, 1), None), ((1, 1, 1), (float("inf"),) + (0,) * 8)):
        g = (ctypes.c_double * 3)(*gains)
        c = None if m is None else (ctypes.c_double * 9)(*m)
        assert L.mibayer_colour_matrix(g, c, out) == pkg.ERR_ARG, (gains, m)
        assert out[:] == [77] * 9                                                  # nothing written on failure
    assert L.mibayer_colour_matrix(None, None, out) == pkg.ERR_ARG
    assert L.mibayer_colour_matrix((ctypes.c_double * 3)(1, 1, 1), None, None) == pkg.ERR_ARG


def test_colour_tone_tables(pkg):
    assert pkg.colour_tone(pkg.TONE_LINEAR) == [256 * i for i in range(257)]
    x = np.arange(257) / 256.0
    srgb = np.where(x <= 0.0031308, 12.92 * x, 1.055 * np.power(x, 1 / 2.4) - 0.055)
    got = np.array(pkg.colour_tone(pkg.TONE_SRGB), np.int64)
    assert got[0] == 0 and got[256] == 65536
    assert (np.diff(got) > 0).all()
    assert np.abs(got - np.round(srgb * 65536)).max() <= 1
    for gamma in (1.0, 1.8, 2.2, 0.5):
        got = np.array(pkg.colour_tone(pkg.TONE_GAMMA, gamma), np.int64)
        assert got[0] == 0 and got[256] == 65536 and (np.diff(got) >= 0).all()
        assert np.abs(got - np.round(np.power(x, 1 / gamma) * 65536)).max() <= 1
    assert pkg.colour_tone(pkg.TONE_GAMMA, 1.0) == [256 * i for i in range(257)]
    L = pkg.lib()
    buf = (ctypes.c_uint32 * 257)()
    for curve, gamma in ((-1, 2.2), (3, 2.2), (pkg.TONE_GAMMA, 0.0), (pkg.TONE_GAMMA, -1.0), (pkg.TONE_GAMMA, float("nan"))):
        assert L.mibayer_colour_tone(curve, gamma, buf) == pkg.ERR_ARG, (curve, gamma)
    assert L.mibayer_colour_tone(pkg.TONE_SRGB, 2.2, None) == pkg.ERR_ARG
    assert L.mibayer_colour_tone(pkg.TONE_SRGB, float("nan"), buf) == pkg.OK        # gamma is read by TONE_GAMMA only


def test_set_get_colour_refuse_null_handles(pkg):
    """what can be said without a context; the checks on a context are GPU tests (tests/test_gpu_colour.py)"""
    L = pkg.lib()
    col = pkg.Colour()
    assert L.mibayer_set_colour(None, ctypes.byref(col)) == pkg.ERR_ARG
    assert L.mibayer_get_colour(None, ctypes.byref(col)) == pkg.ERR_ARG
    assert L.mibayer_pool_set_colour(None, ctypes.byref(col)) == pkg.ERR_ARG


def prop_block(out, name):
    """the block of property `name` in gst-inspect's property list, or None"""
    m = re.search(r"^\s+%s\s+: .*?(?=^\s+[a-z-]+\s+: |\Z)" % re.escape(name), out, re.M | re.S)
    return m.group(0) if m else None


@needs_gst
def test_inspect_lists_the_seven_properties(plugin, tmp_path):  # noqa: F811
    for element in ("bayer2rgb", "hipbayer2rgb"):
        out = inspect(tmp_path, element)
        for name in PROPS:
            block = prop_block(out, name)
            assert block is not None, (element, name)
            assert "changeable only in NULL or READY state" in block, block
        assert "Unsigned Integer. Range: 0 - 65535 Default: 0" in prop_block(out, "black-level")
        for name in ("red-gain", "green-gain", "blue-gain"):
            b = " ".join(prop_block(out, name).split())
            assert re.search(r"Double\. Range: 0 - 15\.99 Default: 1\b", b), b
        assert 'String. Default: ""' in prop_block(out, "ccm")
        tone = prop_block(out, "tone-curve")
        assert 'Default: 0, "linear"' in tone and "(1): srgb" in tone and "(2): gamma" in tone and "(0): linear" in tone
        assert re.search(r"Default: 2\.2\b", " ".join(prop_block(out, "gamma").split()))
    r2b = inspect(tmp_path, "rgb2bayer")
    assert "Availability: Always" in r2b
    for name in PROPS:
        assert prop_block(r2b, name) is None, name


@needs_gst
def test_mock_rig_defaults_convert_and_colour_requests_fail_cleanly(rig, tmp_path):  # noqa: F811
    """The mock library has no colour entry points.  With default properties -- spelled out or not -- the elements call
    none of them and convert as before; a non-default one ends in an element error, not in a crash (the harness runs
    under AddressSanitizer and must exit 0)."""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=7).tofile(inp)
    defaults = "black-level=0 red-gain=1 green-gain=1 blue-gain=1 ccm=\"\" tone-curve=linear gamma=1.8"
    for launch in ("bayer2rgb", "bayer2rgb " + defaults, "bayer2rgb inflight=3 devices=0,0 " + defaults,
                   "hipupload ! hipbayer2rgb " + defaults + " ! hipdownload"):
        kv = run(rig, "convert", launch, B2R % ("gbrg", w, h), inp, 260 * h, outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n) and kv["errors"] == "0", (launch, kv)
        seq, fill = stamps(outp, n, 4 * w * h)
        assert fill == list(range(7, 7 + n)) and seq == list(range(n)), launch
    for prop in ("red-gain=2.0", "black-level=16", "tone-curve=srgb", "ccm=1,0,0,0,1,0,0,0,1", "tone-curve=gamma gamma=2.0"):
        for launch in ("bayer2rgb %s" % prop, "bayer2rgb inflight=3 devices=0,0 %s" % prop,
                       "hipupload ! hipbayer2rgb %s ! hipdownload" % prop):
            kv = run(rig, "caps", launch, B2R % ("gbrg", w, h), 260 * h)
            assert int(kv["errors"]) >= 1 and kv["caps_accepted"] == "0", (launch, kv)
