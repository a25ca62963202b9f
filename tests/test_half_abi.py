"""CPU tests of the half-size demosaic at the boundary: MIBAYER_FLAG_HALF in include/mibayer.h, what mibayer_create
makes of a cfg that carries it (validation comes before the device is looked for, so the answers are the same without a
GPU: MIBAYER_OK there reads MIBAYER_ERR_NO_DEVICE here).  What needs a context
-- the deep-context refusals, the frames -- is in tests/test_gpu_half.py."""
import ctypes
import os
import re
import subprocess

import pytest

import half_cases as hc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mibayer.h")


def create(pkg, cfg, default_stride=None):
    """mibayer_create's answer; where a device is there the context exists for a moment and shows the resolved cfg:
    the mosaic's size, and the stride asked for or -- where the caller knows it -- the default"""
    h = ctypes.c_void_p()
    rc = pkg.lib().mibayer_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == pkg.OK:
        got = pkg.Cfg()
        assert pkg.lib().mibayer_get_cfg(h, ctypes.byref(got)) == pkg.OK
        assert (got.width, got.height, got.flags) == (cfg.width, cfg.height, cfg.flags)       # the mosaic's
        if cfg.dst_stride or default_stride:
            assert got.dst_stride == (cfg.dst_stride or default_stride)
        pkg.lib().mibayer_destroy(h)
    return rc


def half_cfg(pkg, w, h, fam=None, **kw):
    fam = fam or hc.FAMILIES[0]
    return pkg.make_cfg(w, h, kw.pop("pattern", "grbg"), fam.fmt, method="half", dst_big_endian=fam.dbe, **kw)


def test_the_flag_is_accepted(pkg):
    """bit 23 was an unknown flag (MIBAYER_ERR_ARG) before the feature"""
    assert create(pkg, pkg.make_cfg(64, 48, flags=1 << 23)) in (pkg.OK, pkg.ERR_NO_DEVICE)
    assert create(pkg, pkg.make_cfg(6, 3, method="half")) in (pkg.OK, pkg.ERR_NO_DEVICE)


def test_header_and_harness_define_the_flag(pkg):
    text = open(HEADER).read()
    m = re.search(r"#define MIBAYER_FLAG_HALF \(1u << (\d+)\)", text)
    assert m and int(m.group(1)) == 23 and pkg.FLAG_HALF == 1 << 23 and pkg.METHODS["half"] == pkg.FLAG_HALF
    others = (pkg.FLAG_HIPGRAPH | pkg.FLAG_RGB2BAYER | pkg.FLAG_HIPGRAPH_CHAIN | pkg.FLAG_SRC_BITS_MASK
              | pkg.FLAG_SRC_BIG_ENDIAN | pkg.FLAG_DST_16BIT | pkg.FLAG_DST_BIG_ENDIAN | pkg.FLAG_DST_24BIT
              | pkg.FLAG_DST_PLANAR | pkg.FLAG_MHC | pkg.FLAG_COLOUR)
    assert pkg.FLAG_HALF & others == 0
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text) and pkg.lib().mibayer_abi_version() == 5
    assert "5, later additive: half-size demosaic" in text
    doc = text[text.index("/* One RGB pixel per CFA quad"):text.index("#define MIBAYER_FLAG_HALF")]
    assert "CENTRE" in doc and "half an output pixel" in doc           # where the pixel sits is part of the contract
    assert pkg.make_cfg(64, 48).flags == 0 and pkg.make_cfg(64, 48, method="bilinear").flags == 0
    assert pkg.make_cfg(64, 48, method="half").flags == pkg.FLAG_HALF
    with pytest.raises(ValueError):
        pkg.make_cfg(64, 48, method="quarter")


def test_bits_17_18_20_24_and_31_are_still_unknown_flags(pkg):
    for bit in (17, 18, 20, 24, 31):
        assert create(pkg, pkg.make_cfg(64, 48, flags=1 << bit)) == pkg.ERR_ARG, bit
        assert create(pkg, pkg.make_cfg(64, 48, method="half", flags=1 << bit)) == pkg.ERR_ARG, bit


def test_flag_combinations(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    for fam in hc.FAMILIES:
        for bits, sbe in hc.SAMPLES + ((14, False),):
            for colour in (None, True):
                for extra in (0, pkg.FLAG_HIPGRAPH, pkg.FLAG_HIPGRAPH | pkg.FLAG_HIPGRAPH_CHAIN):
                    cfg = half_cfg(pkg, 66, 49, fam, bits=bits, src_big_endian=sbe, colour=colour, flags=extra)
                    assert create(pkg, cfg) in ok, (fam, bits, sbe, colour, extra)
    mk = pkg.make_cfg
    H = pkg.FLAG_HALF
    # refused: nothing to interpolate, the inverse direction, a kernel variant -- alone and with other flags on top
    assert create(pkg, mk(64, 48, method="mhc", flags=H)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, method="mhc", flags=H, bits=12, colour=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", method="mhc", flags=H)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, flags=H | pkg.FLAG_RGB2BAYER)) == pkg.ERR_ARG
    for v in (1, 2, 3):
        assert create(pkg, mk(64, 48, method="half", variant=v)) == pkg.ERR_ARG, v
    # the other flags keep their own rules under it
    assert create(pkg, mk(64, 48, method="half", dst_big_endian=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, method="half", src_big_endian=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", method="half", out16=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="GBR", method="half", flags=pkg.FLAG_DST_24BIT)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, method="half", bits=11)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt=(2, 0, 1), method="half")) == pkg.ERR_LAYOUT
    assert create(pkg, mk(64, 48, fmt=(1, 2, 3), method="half", flags=pkg.FLAG_DST_PLANAR)) == pkg.ERR_LAYOUT
    # the plan selectors describe the production kernels only
    sel, swap = (ctypes.c_uint32 * 4)(), ctypes.c_int()
    cfg = mk(64, 48, method="half")
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.ERR_ARG
    cfg = mk(64, 48)
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.OK


def test_geometry_is_the_mosaics(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    for w, h in ((4, 3), (6, 3), (6, 4), (6, 5), (1 << 26, 3)):
        assert create(pkg, half_cfg(pkg, w, h)) in ok, (w, h)
    for w, h in ((2, 18), (5, 18), (63, 18), (64, 2), (64, 0), ((1 << 26) + 2, 4)):
        assert create(pkg, half_cfg(pkg, w, h)) == pkg.ERR_GEOMETRY, (w, h)
    # the source keeps its own rules
    assert create(pkg, half_cfg(pkg, 66, 48, src_stride=66)) == pkg.ERR_GEOMETRY
    assert create(pkg, half_cfg(pkg, 66, 48, src_stride=68)) in ok
    assert create(pkg, half_cfg(pkg, 66, 48, bits=12, src_stride=132)) in ok
    assert create(pkg, half_cfg(pkg, 66, 48, bits=12, src_stride=128)) == pkg.ERR_GEOMETRY


@pytest.mark.parametrize("fam", hc.FAMILIES, ids=lambda f: f.fmt + ("be" if f.dbe else ""))
def test_stride_default_and_limits(pkg, fam):
    """strides count OUTPUT pixels: default ROUND_UP_4 (px * OW), at least px * OW, a multiple of 4 (8 for 16-bit
    channels) -- for even and odd OW"""
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    unit = 8 if fam.px == 8 else 4
    for ow in (2, 3, 4, 5, 7, 8, 9, 33, 129, 130):
        w, row = 2 * ow, fam.px * ow
        default = (row + 3) & ~3
        assert default == hc.default_dst_stride(fam, ow)
        assert create(pkg, half_cfg(pkg, w, 19, fam), default) in ok, (fam, ow)
        assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=default)) in ok, (fam, ow)
        assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=default + 8)) in ok, (fam, ow)
        # the bytes of a row themselves only where they are a multiple of the unit; below them never
        assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=row)) in (ok if row % unit == 0 else (pkg.ERR_GEOMETRY,))
        assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=row - 1)) == pkg.ERR_GEOMETRY, (fam, ow)
        if default > unit:              # (a stride of 0 asks for the default)
            assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=default - unit)) == pkg.ERR_GEOMETRY, (fam, ow)
        for off in (1, 2, 3) + ((4,) if unit == 8 else ()):
            assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=default + off)) == pkg.ERR_GEOMETRY, (fam, ow, off)
        # what the full-resolution cfg's default would be is far more than needed, and allowed
        assert create(pkg, half_cfg(pkg, w, 19, fam, dst_stride=(fam.px * w + 7) & ~7)) in ok


def test_header_groups_still_partition_the_symbols(pkg, lab_pkg):
    """the flag adds no entry point: the header's groups, the harness' table and the library's symbol table are one
    list, as they were"""
    text = open(HEADER).read()
    block = text[text.index("MIBAYER ABI GROUPS"):text.index("END OF MIBAYER ABI GROUPS")]
    groups = re.split(r"\* group ([a-z-]+):", block)[1:]
    names = {}
    for name, body in zip(groups[0::2], groups[1::2]):
        names[name] = re.findall(r"\b(mibayer_[a-z0-9_]+)\b", body)
    every = [n for g in names.values() for n in g]
    assert len(every) == len(set(every)), "a symbol is in two groups"
    assert sorted(every) == sorted(pkg.ABI)
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = sorted(ln.split()[-1].split("@")[0] for ln in out.splitlines() if ln.split()[-1].startswith("mibayer_"))
    assert exported == sorted(every)
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"\b%d (exported )?(functions|entry points|symbols)" % len(every), readme)


def test_pool_cfg_takes_the_method(pkg):
    """mibayer_pool_create validates the stream cfg like mibayer_create"""
    pc = pkg.PoolCfg()
    pc.struct_size = ctypes.sizeof(pkg.PoolCfg)
    pc.ndevices = 1
    pc.devices[0] = 0
    h = ctypes.c_void_p()
    pc.stream = pkg.make_cfg(66, 48, method="mhc", flags=pkg.FLAG_HALF)
    assert pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h)) == pkg.ERR_ARG
    pc.stream = pkg.make_cfg(66, 48, method="half", fmt="RGB", dst_stride=98)
    assert pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h)) == pkg.ERR_GEOMETRY
    pc.stream = pkg.make_cfg(66, 48, method="half", fmt="RGB")
    rc = pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h))
    assert rc in (pkg.OK, pkg.ERR_NO_DEVICE)
    if rc == pkg.OK:
        pkg.lib().mibayer_pool_destroy(h)
