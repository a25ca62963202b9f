"""CPU tests of packed 24-bit output at the boundary: MIBAYER_FLAG_DST_24BIT in include/mibayer.h and what
mibayer_create makes of a cfg that carries it (validation comes before the device is looked for, so the answers are the
same without a GPU: MIBAYER_OK there reads MIBAYER_ERR_NO_DEVICE here).  What needs a context -- the mibayer_get_cfg
round trip, the deep-context refusals -- is in tests/test_gpu_rgb24.py."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def create(pkg, cfg):
    """mibayer_create's answer.  Where a device is there (the whole suite on a GPU machine) the context exists for a
    moment and the mibayer_get_cfg round trip is checked too; without one the answer is all there is"""
    h = ctypes.c_void_p()
    rc = pkg.lib().mibayer_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == pkg.OK:
        got = pkg.Cfg()
        assert pkg.lib().mibayer_get_cfg(h, ctypes.byref(got)) == pkg.OK
        # the round trip: what was asked for, with the defaults filled in
        assert (got.width, got.height, got.flags) == (cfg.width, cfg.height, cfg.flags)
        assert (got.r_off, got.g_off, got.b_off) == (cfg.r_off, cfg.g_off, cfg.b_off)
        px = 3 if cfg.flags & pkg.FLAG_DST_24BIT else 4
        assert got.dst_stride == (cfg.dst_stride or (px * cfg.width + 3) & ~3)
        pkg.lib().mibayer_destroy(h)
    return rc


def test_header_and_harness_define_the_flag(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    m = re.search(r"#define MIBAYER_FLAG_DST_24BIT \(1u << (\d+)\)", text)
    assert m and pkg.FLAG_DST_24BIT == 1 << int(m.group(1))
    others = (pkg.FLAG_HIPGRAPH | pkg.FLAG_RGB2BAYER | pkg.FLAG_HIPGRAPH_CHAIN | pkg.FLAG_SRC_BITS_MASK
              | pkg.FLAG_SRC_BIG_ENDIAN | pkg.FLAG_DST_16BIT | pkg.FLAG_DST_BIG_ENDIAN | pkg.FLAG_MHC | pkg.FLAG_COLOUR)
    assert pkg.FLAG_DST_24BIT & others == 0
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text) and pkg.lib().mibayer_abi_version() == 5
    assert pkg.FORMATS24 == {"RGB": (0, 1, 2), "BGR": (2, 1, 0)}
    for fmt, off in pkg.FORMATS24.items():
        cfg = pkg.make_cfg(64, 48, fmt=fmt)
        assert cfg.flags == pkg.FLAG_DST_24BIT and (cfg.r_off, cfg.g_off, cfg.b_off) == off
    assert pkg.make_cfg(64, 48, fmt="BGRx").flags == 0            # a cfg without the flag is what it was


def test_stride_default_and_limits(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    for w in (4, 6, 20, 22, 258, 260):
        assert create(pkg, mk(w, 18, fmt="RGB")) in ok, w                         # default: ROUND_UP_4 (3 w)
        assert create(pkg, mk(w, 18, fmt="RGB", dst_stride=(3 * w + 3) & ~3)) in ok, w
        assert create(pkg, mk(w, 18, fmt="BGR", dst_stride=((3 * w + 3) & ~3) + 8)) in ok, w
        # 3 w itself only where it is a multiple of 4; 3 w - 1 never (too short, whatever its residue)
        assert create(pkg, mk(w, 18, fmt="RGB", dst_stride=3 * w)) in (ok if (3 * w) % 4 == 0 else (pkg.ERR_GEOMETRY,)), w
        assert create(pkg, mk(w, 18, fmt="RGB", dst_stride=3 * w - 1)) == pkg.ERR_GEOMETRY, w
        assert create(pkg, mk(w, 18, fmt="RGB", dst_stride=((3 * w + 3) & ~3) - 4)) == pkg.ERR_GEOMETRY, w
        assert create(pkg, mk(w, 18, fmt="RGB", dst_stride=((3 * w + 3) & ~3) + 2)) == pkg.ERR_GEOMETRY, w
    # the stride of 4-byte pixels is no longer needed, and the source keeps its own rules
    assert create(pkg, mk(64, 48, fmt="RGB", dst_stride=192)) in ok
    assert create(pkg, mk(66, 48, fmt="RGB", src_stride=66)) == pkg.ERR_GEOMETRY
    assert create(pkg, mk(66, 48, fmt="RGB", bits=12, src_stride=132)) in ok
    # geometry: that of the 8-bit path, and the deep flags' width limit
    for w, h in ((2, 18), (63, 18), (64, 2)):
        assert create(pkg, mk(w, h, fmt="RGB")) == pkg.ERR_GEOMETRY, (w, h)
    assert create(pkg, mk((1 << 26) + 2, 4, fmt="RGB")) == pkg.ERR_GEOMETRY


def test_layouts(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    F = pkg.FLAG_DST_24BIT
    for off in ((0, 1, 2), (2, 1, 0)):
        assert create(pkg, pkg.make_cfg(64, 48, fmt=off, flags=F)) in ok, off
        assert create(pkg, pkg.make_cfg(64, 48, fmt=off, flags=F, bits=14, method="mhc", colour=True)) in ok, off
    # the 4-byte layouts with a leading pad byte do not exist in 3 bytes, nor does anything else
    for off in ((1, 2, 3), (3, 2, 1), (0, 2, 1), (1, 1, 1), (0, 1, 3), (2, 1, 2), (-1, 1, 2)):
        assert create(pkg, pkg.make_cfg(64, 48, fmt=off, flags=F)) == pkg.ERR_LAYOUT, off
    assert create(pkg, pkg.make_cfg(64, 48, fmt=(1, 2, 3))) in ok                 # xRGB is still xRGB


def test_flag_combinations(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    for bits in (0, 10, 12, 14, 16):
        for sbe in ((False, True) if bits else (False,)):
            for method in ("bilinear", "mhc"):
                for colour in (None, True):
                    for extra in (0, pkg.FLAG_HIPGRAPH, pkg.FLAG_HIPGRAPH | pkg.FLAG_HIPGRAPH_CHAIN):
                        cfg = mk(66, 48, "grbg", "BGR", bits=bits, src_big_endian=sbe, method=method, colour=colour,
                                 flags=extra)
                        assert create(pkg, cfg) in ok, (bits, sbe, method, colour, extra)
    # refused: 16-bit channels, their byte order, the inverse direction, a kernel variant
    assert create(pkg, mk(64, 48, fmt="RGB", out16=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", out16=True, dst_big_endian=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", dst_big_endian=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", bits=12, out16=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", flags=pkg.FLAG_RGB2BAYER)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", src_big_endian=True)) == pkg.ERR_ARG        # no depth to go with it
    for v in (1, 2, 3):
        assert create(pkg, mk(64, 48, fmt="RGB", variant=v)) == pkg.ERR_ARG, v
    # the plan selectors describe the production kernels only
    sel, swap = (ctypes.c_uint32 * 4)(), ctypes.c_int()
    cfg = mk(64, 48, fmt="RGB")
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.ERR_ARG
    cfg = mk(64, 48, fmt="RGBx")
    assert pkg.lib().mibayer_plan_selectors(ctypes.byref(cfg), sel, ctypes.byref(swap)) == pkg.OK


def test_pool_cfg_takes_the_format_names(pkg):
    """mibayer_pool_create validates the stream cfg like mibayer_create"""
    pc = pkg.PoolCfg()
    pc.struct_size = ctypes.sizeof(pkg.PoolCfg)
    pc.ndevices = 1
    pc.devices[0] = 0
    h = ctypes.c_void_p()
    pc.stream = pkg.make_cfg(66, 48, fmt="BGR", out16=True)
    assert pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h)) == pkg.ERR_ARG
    pc.stream = pkg.make_cfg(66, 48, fmt=(1, 2, 3), flags=pkg.FLAG_DST_24BIT)
    assert pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h)) == pkg.ERR_LAYOUT
    pc.stream = pkg.make_cfg(66, 48, fmt="BGR")
    rc = pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h))
    assert rc in (pkg.OK, pkg.ERR_NO_DEVICE)
    if rc == pkg.OK:
        pkg.lib().mibayer_pool_destroy(h)
