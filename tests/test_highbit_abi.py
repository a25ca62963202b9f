"""CPU tests of deep samples at the boundaries: the cfg flags of include/mibayer.h and what mibayer_create makes of
them, the element's second caps structures (gst-inspect, and the mock rig of test_gst_element_logic.py)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from test_gst_element import GST_INSPECT, gst_env, needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, rig, run  # noqa: F401  (fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def create(pkg, cfg):
    h = ctypes.c_void_p()
    rc = pkg.lib().mibayer_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == pkg.OK:
        pkg.lib().mibayer_destroy(h)
    return rc


def test_header_defines_the_deep_flags(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    want = {"MIBAYER_FLAG_SRC_BITS(n)": r"\(\(uint32_t\) \(n\) << 8\)", "MIBAYER_FLAG_SRC_BITS_MASK": r"\(0x1fu << 8\)",
            "MIBAYER_FLAG_SRC_BIG_ENDIAN": r"\(1u << 13\)", "MIBAYER_FLAG_DST_16BIT": r"\(1u << 14\)",
            "MIBAYER_FLAG_DST_BIG_ENDIAN": r"\(1u << 15\)"}
    for name, value in want.items():
        assert re.search(r"#define %s %s" % (re.escape(name), value), text), name
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    assert pkg.FLAG_SRC_BITS(12) == 12 << 8 and pkg.FLAG_SRC_BITS_MASK == 0x1F << 8
    assert (pkg.FLAG_SRC_BIG_ENDIAN, pkg.FLAG_DST_16BIT, pkg.FLAG_DST_BIG_ENDIAN) == (1 << 13, 1 << 14, 1 << 15)


def test_deep_cfg_validation(pkg):
    ok_or_nodev = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    # valid: every depth, both byte orders, both output depths, an 8-bit mosaic with 16-bit output
    for bits in (10, 12, 14, 16):
        for sbe in (False, True):
            for out16, dbe in ((False, False), (True, False), (True, True)):
                fmt = "ARGB64" if out16 else "BGRx"
                assert create(pkg, mk(64, 48, "rggb", fmt, bits=bits, src_big_endian=sbe, out16=out16,
                                      dst_big_endian=dbe)) in ok_or_nodev, (bits, sbe, out16, dbe)
    assert create(pkg, mk(64, 48, fmt="ARGB64")) in ok_or_nodev
    assert create(pkg, mk(64, 48, fmt="RGBA64", bits=12, flags=pkg.FLAG_HIPGRAPH)) in ok_or_nodev
    for r, g, b in ((0, 1, 2), (2, 1, 0), (1, 2, 3), (3, 2, 1)):
        assert create(pkg, mk(64, 48, fmt=(r, g, b), bits=12, out16=True)) in ok_or_nodev
    # strides: 16-bit samples >= 2*width and a multiple of 4; 16-bit output >= 8*width and a multiple of 8
    assert create(pkg, mk(66, 48, bits=12, src_stride=132)) in ok_or_nodev
    assert create(pkg, mk(66, 48, bits=12, src_stride=136, out16=True, dst_stride=536)) in ok_or_nodev
    for kw in (dict(src_stride=126), dict(src_stride=130), dict(src_stride=64), dict(out16=True, dst_stride=508),
               dict(out16=True, dst_stride=516), dict(out16=True, dst_stride=256), dict(width=63),
               dict(width=2), dict(height=2)):
        w = kw.pop("width", 64)
        h = kw.pop("height", 48)
        assert create(pkg, mk(w, h, bits=12, **kw)) == pkg.ERR_GEOMETRY, (w, h, kw)
    # an 8-bit mosaic with 16-bit output keeps the 8-bit source stride rule
    assert create(pkg, mk(66, 48, out16=True, src_stride=66)) == pkg.ERR_GEOMETRY
    assert create(pkg, mk(66, 48, out16=True, src_stride=68)) in ok_or_nodev
    # layouts: the four of the 8-bit path, counted in channels
    for r, g, b in ((0, 2, 1), (1, 1, 1), (0, 1, 3), (4, 1, 0)):
        assert create(pkg, mk(64, 48, fmt=(r, g, b), bits=16, out16=True)) == pkg.ERR_LAYOUT, (r, g, b)
    # arguments: depths outside {0, 10, 12, 14, 16}, an endianness without its depth, rgb2bayer, variants
    for bits in (1, 8, 9, 11, 15, 17, 31):
        assert create(pkg, mk(64, 48, flags=pkg.FLAG_SRC_BITS(bits))) == pkg.ERR_ARG, bits
    assert create(pkg, mk(64, 48, flags=pkg.FLAG_SRC_BIG_ENDIAN)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, flags=pkg.FLAG_SRC_BIG_ENDIAN | pkg.FLAG_DST_16BIT)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, bits=12, flags=pkg.FLAG_DST_BIG_ENDIAN)) == pkg.ERR_ARG
    for deep in (dict(bits=12), dict(out16=True), dict(bits=10, src_big_endian=True)):
        assert create(pkg, mk(64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER, **deep)) == pkg.ERR_ARG, deep
    assert create(pkg, mk(64, 48, bits=12, variant=1)) == pkg.ERR_ARG
    # the 8-bit path is what it was: SRC_BITS(0) without DST_16BIT is no flag at all
    assert create(pkg, mk(64, 48, flags=pkg.FLAG_SRC_BITS(0))) in ok_or_nodev
    # plan selectors describe the 8-bit kernel only
    sel, swap = (ctypes.c_uint32 * 4)(), ctypes.c_int()
    cfg = mk(64, 48, bits=12)
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.ERR_ARG


def inspect(tmp_path, what="bayer2rgb"):
    return subprocess.run([GST_INSPECT, what], capture_output=True, text=True, env=gst_env(tmp_path),
                          timeout=120).stdout


@needs_gst
def test_inspect_lists_the_second_structures(plugin, tmp_path):  # noqa: F811
    out = inspect(tmp_path)
    first_sink = "format: { (string)bggr, (string)grbg, (string)gbrg, (string)rggb }"
    first_src = ("format: { (string)RGBx, (string)xRGB, (string)BGRx, (string)xBGR, (string)RGBA, "
                 "(string)ARGB, (string)BGRA, (string)ABGR }")
    assert first_sink in out and first_src in out
    assert out.count("Availability: Always") == 2
    deep = ["(string)%s%d%s" % (o, b, e) for o in ("bggr", "grbg", "gbrg", "rggb") for b in (10, 12, 14, 16)
            for e in ("le", "be")]
    line = [ln for ln in out.splitlines() if "bggr10le" in ln]
    assert len(line) == 1 and line[0].strip() == "format: { %s }" % ", ".join(deep)
    assert out.index(first_sink) < out.index("bggr10le")           # after the pinned first structure
    assert re.search(r"format: ARGB64\n", out) and out.index(first_src) < out.index("ARGB64")
    assert len(re.findall(r"^\s+video/x-bayer$", out, re.M)) == 2
    assert len(re.findall(r"^\s+video/x-raw$", out, re.M)) == 2
    # rgb2bayer keeps its 8-bit templates (it shares the caps functions, not the templates)
    r2b = inspect(tmp_path, "rgb2bayer")
    assert "Availability: Always" in r2b and "10le" not in r2b and "ARGB64" not in r2b


@needs_gst
@pytest.mark.parametrize("fmt,bpp", [("ARGB64", 8), ("BGRx", 4)])
def test_mock_rig_negotiates_deep_caps(rig, tmp_path, fmt, bpp):  # noqa: F811
    """bggr12le -> ARGB64 / BGRx on the element's own logic (mock library): accepted, the mosaic takes 2 bytes per
    sample, the output 8 / 4 per pixel, frames leave once each, in order, in both modes"""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    mosaic = 2 * w * h
    kv = run(rig, "caps", "bayer2rgb ! capsfilter caps=\"video/x-raw,format=%s\"" % fmt, B2R % ("bggr12le", w, h), mosaic)
    assert kv["caps_accepted"] == "1" and kv["errors"] == "0", kv
    np.repeat(np.arange(7, 7 + n, dtype=np.uint8), mosaic).tofile(inp)
    for launch in ("bayer2rgb", "bayer2rgb inflight=3 devices=0,0"):
        kv = run(rig, "convert", "%s ! capsfilter caps=\"video/x-raw,format=%s\"" % (launch, fmt), B2R % ("bggr12le", w, h), inp, mosaic,
                 outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n), kv
        got = np.fromfile(outp, np.uint8)
        assert got.size == n * bpp * w * h
        got = got.reshape(n, -1)
        assert [int.from_bytes(bytes(got[i, :4]), "little") for i in range(n)] == list(range(n))
        assert [int(got[i, 4]) for i in range(n)] == list(range(7, 7 + n))
    # a short mosaic (8-bit sized) is an error, not a read past the buffer
    kv = run(rig, "caps", "bayer2rgb ! capsfilter caps=\"video/x-raw,format=%s\"" % fmt, B2R % ("bggr12le", w, h), w * h)
    assert kv["caps_accepted"] == "0"


@needs_gst
def test_mock_rig_refuses_an_odd_deep_width(rig):  # noqa: F811
    for w, h in ((63, 48), (2, 48), (64, 2)):
        kv = run(rig, "caps", "bayer2rgb ! capsfilter caps=\"video/x-raw,format=ARGB64\"", B2R % ("rggb16be", w, h), 2 * (w + 1) * h)
        assert kv["caps_accepted"] == "0" and kv["flow"] == "not-negotiated", (w, h, kv)
