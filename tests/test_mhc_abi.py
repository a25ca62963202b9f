"""CPU tests of the Malvar-He-Cutler demosaic at the boundaries: MIBAYER_FLAG_MHC in include/mibayer.h and the
harness, what mibayer_create makes of it, and the elements' `method` property (gst-inspect, and the mock rig of
test_gst_element_logic.py)."""
import ctypes
import os
import re

import numpy as np
import pytest

from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, rig, run  # noqa: F401  (fixture)
from test_highbit_abi import create, inspect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_header_defines_the_mhc_flag(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_FLAG_MHC \(1u << 16\)", text)
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    assert pkg.FLAG_MHC == 1 << 16
    assert pkg.make_cfg(64, 48, method="mhc").flags == pkg.FLAG_MHC
    assert pkg.make_cfg(64, 48, method="bilinear").flags == 0
    assert pkg.make_cfg(64, 48, "bggr", "ARGB64", bits=12, method="mhc").flags \
        == pkg.FLAG_MHC | pkg.FLAG_SRC_BITS(12) | pkg.FLAG_DST_16BIT
    with pytest.raises(ValueError):
        pkg.make_cfg(64, 48, method="vng")


def test_mhc_cfg_validation(pkg):
    ok_or_nodev = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    # valid: the 8-bit mosaic, every depth and byte order, both output depths, HIPGRAPH (and its chain mode)
    for fmt in ("RGBx", "BGRx", "xRGB", "xBGR"):
        assert create(pkg, mk(64, 48, "gbrg", fmt, method="mhc")) in ok_or_nodev, fmt
    for bits in (0, 10, 12, 14, 16):
        for sbe in ((False,) if bits == 0 else (False, True)):
            for out16, dbe in ((False, False), (True, False), (True, True)):
                fmt = "ARGB64" if out16 else "BGRx"
                assert create(pkg, mk(64, 48, "rggb", fmt, bits=bits, src_big_endian=sbe, out16=out16,
                                      dst_big_endian=dbe, method="mhc")) in ok_or_nodev, (bits, sbe, out16, dbe)
    assert create(pkg, mk(64, 48, flags=pkg.FLAG_HIPGRAPH, method="mhc")) in ok_or_nodev
    assert create(pkg, mk(64, 48, flags=pkg.FLAG_HIPGRAPH | pkg.FLAG_HIPGRAPH_CHAIN, method="mhc")) in ok_or_nodev
    assert create(pkg, mk(4, 3, method="mhc")) in ok_or_nodev
    # strides and geometry: those of the same cfg without the flag
    assert create(pkg, mk(66, 48, src_stride=68, dst_stride=264, method="mhc")) in ok_or_nodev
    assert create(pkg, mk(66, 48, bits=12, src_stride=136, out16=True, dst_stride=536, method="mhc")) in ok_or_nodev
    for kw in (dict(src_stride=66), dict(dst_stride=260), dict(width=63), dict(width=2), dict(height=2)):
        w = kw.pop("width", 66)
        h = kw.pop("height", 48)
        assert create(pkg, mk(w, h, method="mhc", **kw)) == pkg.ERR_GEOMETRY, (w, h, kw)
    assert create(pkg, mk(64, 48, fmt=(0, 2, 1), method="mhc")) == pkg.ERR_LAYOUT
    # refused: rgb2bayer, a kernel variant
    assert create(pkg, mk(64, 48, "bggr", "ARGB", flags=pkg.FLAG_RGB2BAYER, method="mhc")) == pkg.ERR_ARG
    for v in (1, 2, 3):
        assert create(pkg, mk(64, 48, variant=v, method="mhc")) == pkg.ERR_ARG, v
        assert create(pkg, mk(64, 48, variant=v, bits=12, method="mhc")) == pkg.ERR_ARG, v
    # plan selectors describe the bilinear 8-bit kernel only
    sel, swap = (ctypes.c_uint32 * 4)(), ctypes.c_int()
    cfg = mk(64, 48, method="mhc")
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.ERR_ARG


def test_unknown_flags_are_still_refused(pkg):
    for bit in (17, 18, 24, 31):
        assert create(pkg, pkg.make_cfg(64, 48, flags=1 << bit)) == pkg.ERR_ARG, bit


def method_property(out):
    """the `method` block of gst-inspect's property list, or None"""
    m = re.search(r"^\s+method\s+: .*?(?=^\s+[a-z-]+\s+: |\Z)", out, re.M | re.S)
    return m.group(0) if m else None


@needs_gst
def test_inspect_lists_method(plugin, tmp_path):  # noqa: F811
    for element in ("bayer2rgb", "hipbayer2rgb"):
        block = method_property(inspect(tmp_path, element))
        assert block is not None, element
        assert 'Default: 0, "bilinear"' in block, block
        assert '(1): mhc' in block and '(0): bilinear' in block, block
        assert "changeable only in NULL or READY state" in block, block
    r2b = inspect(tmp_path, "rgb2bayer")
    assert "Availability: Always" in r2b and method_property(r2b) is None


@needs_gst
def test_mock_rig_converts_with_method_mhc(rig, tmp_path):  # noqa: F811
    """bayer2rgb method=mhc on the element's own logic (mock library), 8-bit and deep caps, synchronous and queued on
    two shards: negotiated, every frame leaves once, in order"""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    for fmt, bpp, sink, mosaic in (("BGRx", 4, "gbrg", 260 * h), ("ARGB64", 8, "bggr12le", 2 * w * h)):
        np.repeat(np.arange(7, 7 + n, dtype=np.uint8), mosaic).tofile(inp)
        for launch in ("bayer2rgb method=mhc", "bayer2rgb method=mhc inflight=3 devices=0,0"):
            pipe = "%s ! capsfilter caps=\"video/x-raw,format=%s\"" % (launch, fmt)
            kv = run(rig, "caps", pipe, B2R % (sink, w, h), mosaic)
            assert kv["caps_accepted"] == "1" and kv["errors"] == "0", kv
            kv = run(rig, "convert", pipe, B2R % (sink, w, h), inp, mosaic, outp)
            assert kv["pushed"] == str(n) and kv["pulled"] == str(n), (launch, fmt, kv)
            got = np.fromfile(outp, np.uint8)
            assert got.size == n * bpp * w * h
            got = got.reshape(n, -1)
            assert [int.from_bytes(bytes(got[i, :4]), "little") for i in range(n)] == list(range(n))
            assert [int(got[i, 4]) for i in range(n)] == list(range(7, 7 + n))
