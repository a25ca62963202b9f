"""CPU tests of planar 8-bit output at the boundary: MIBAYER_FLAG_DST_PLANAR in include/mibayer.h and what
mibayer_create makes of a cfg that carries it (validation comes before the device is looked for, so the answers are the
same without a GPU: MIBAYER_OK there reads MIBAYER_ERR_NO_DEVICE here).  What needs a context -- the deep-context
refusals, the frames -- is in tests/test_gpu_planar.py."""
import ctypes
import itertools
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def create(pkg, cfg):
    """mibayer_create's answer.  Where a device is there (the whole suite on a GPU machine) the context exists for a
    moment and mibayer_get_cfg shows the resolved stride; without one the answer is all there is"""
    h = ctypes.c_void_p()
    rc = pkg.lib().mibayer_create(ctypes.byref(cfg), ctypes.byref(h))
    if rc == pkg.OK:
        got = pkg.Cfg()
        assert pkg.lib().mibayer_get_cfg(h, ctypes.byref(got)) == pkg.OK
        assert (got.width, got.height, got.flags) == (cfg.width, cfg.height, cfg.flags)
        assert (got.r_off, got.g_off, got.b_off) == (cfg.r_off, cfg.g_off, cfg.b_off)
        assert got.dst_stride == (cfg.dst_stride or (cfg.width + 3) & ~3)
        pkg.lib().mibayer_destroy(h)
    return rc


def test_header_and_harness_define_the_flag(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    m = re.search(r"#define MIBAYER_FLAG_DST_PLANAR \(1u << (\d+)\)", text)
    assert m and int(m.group(1)) == 22 and pkg.FLAG_DST_PLANAR == 1 << 22
    others = (pkg.FLAG_HIPGRAPH | pkg.FLAG_RGB2BAYER | pkg.FLAG_HIPGRAPH_CHAIN | pkg.FLAG_SRC_BITS_MASK
              | pkg.FLAG_SRC_BIG_ENDIAN | pkg.FLAG_DST_16BIT | pkg.FLAG_DST_BIG_ENDIAN | pkg.FLAG_DST_24BIT
              | pkg.FLAG_MHC | pkg.FLAG_COLOUR)
    assert pkg.FLAG_DST_PLANAR & others == 0
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text) and pkg.lib().mibayer_abi_version() == 5
    assert pkg.FORMATS_PLANAR == {"RGBP": (0, 1, 2), "BGRP": (2, 1, 0), "GBR": (2, 0, 1)}
    for fmt, off in pkg.FORMATS_PLANAR.items():
        cfg = pkg.make_cfg(64, 48, fmt=fmt)
        assert cfg.flags == pkg.FLAG_DST_PLANAR and (cfg.r_off, cfg.g_off, cfg.b_off) == off
    assert pkg.make_cfg(64, 48, fmt="RGBx").flags == 0            # a cfg without the flag is what it was
    assert pkg.make_cfg(64, 48, fmt="RGB").flags == pkg.FLAG_DST_24BIT


def test_bits_17_18_20_24_and_31_are_still_unknown_flags(pkg):
    for bit in (17, 18, 20, 24, 31):
        assert create(pkg, pkg.make_cfg(64, 48, flags=1 << bit)) == pkg.ERR_ARG, bit
        assert create(pkg, pkg.make_cfg(64, 48, fmt="RGBP", flags=1 << bit)) == pkg.ERR_ARG, bit


def test_stride_default_and_limits(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    for w in (4, 6, 20, 22, 258, 260):
        r4 = (w + 3) & ~3
        assert create(pkg, mk(w, 18, fmt="RGBP")) in ok, w                              # default: ROUND_UP_4 (w)
        assert create(pkg, mk(w, 18, fmt="GBR", dst_stride=r4)) in ok, w
        assert create(pkg, mk(w, 18, fmt="BGRP", dst_stride=r4 + 8)) in ok, w
        # w itself only where it is a multiple of 4; below w never, whatever its residue
        assert create(pkg, mk(w, 18, fmt="RGBP", dst_stride=w)) in (ok if w % 4 == 0 else (pkg.ERR_GEOMETRY,)), w
        assert create(pkg, mk(w, 18, fmt="RGBP", dst_stride=w - 1)) == pkg.ERR_GEOMETRY, w
        if r4 > 4:                      # (a stride of 0 asks for the default)
            assert create(pkg, mk(w, 18, fmt="RGBP", dst_stride=r4 - 4)) == pkg.ERR_GEOMETRY, w
        assert create(pkg, mk(w, 18, fmt="RGBP", dst_stride=r4 + 2)) == pkg.ERR_GEOMETRY, w
        assert create(pkg, mk(w, 18, fmt="RGBP", dst_stride=r4 + 1)) == pkg.ERR_GEOMETRY, w
    # the source keeps its own rules
    assert create(pkg, mk(66, 48, fmt="RGBP", src_stride=66)) == pkg.ERR_GEOMETRY
    assert create(pkg, mk(66, 48, fmt="RGBP", bits=12, src_stride=132)) in ok
    # geometry: that of the 8-bit path, and the deep flags' width limit
    for w, h in ((2, 18), (63, 18), (64, 2)):
        assert create(pkg, mk(w, h, fmt="RGBP")) == pkg.ERR_GEOMETRY, (w, h)
    assert create(pkg, mk((1 << 26) + 2, 4, fmt="RGBP")) == pkg.ERR_GEOMETRY


def test_plane_indices(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    F = pkg.FLAG_DST_PLANAR
    for off in itertools.permutations((0, 1, 2)):
        assert create(pkg, pkg.make_cfg(64, 48, fmt=off, flags=F)) in ok, off
        assert create(pkg, pkg.make_cfg(64, 48, fmt=off, flags=F, bits=14, method="mhc", colour=True)) in ok, off
    # anything that is no permutation of (0, 1, 2): the byte offsets of xRGB / xBGR among them
    for off in ((1, 2, 3), (3, 2, 1), (0, 0, 1), (1, 1, 1), (0, 1, 3), (2, 1, 2), (-1, 1, 2), (0, 1, 1), (0, 1, 4)):
        assert create(pkg, pkg.make_cfg(64, 48, fmt=off, flags=F)) == pkg.ERR_LAYOUT, off
    assert create(pkg, pkg.make_cfg(64, 48, fmt=(1, 2, 3))) in ok                 # xRGB is still xRGB
    assert create(pkg, pkg.make_cfg(64, 48, fmt=(2, 0, 1))) == pkg.ERR_LAYOUT     # and (2, 0, 1) no 4-byte layout


def test_flag_combinations(pkg):
    ok = (pkg.OK, pkg.ERR_NO_DEVICE)
    mk = pkg.make_cfg
    for bits in (0, 10, 12, 14, 16):
        for sbe in ((False, True) if bits else (False,)):
            for method in ("bilinear", "mhc"):
                for colour in (None, True):
                    for extra in (0, pkg.FLAG_HIPGRAPH, pkg.FLAG_HIPGRAPH | pkg.FLAG_HIPGRAPH_CHAIN):
                        cfg = mk(66, 48, "grbg", "GBR", bits=bits, src_big_endian=sbe, method=method, colour=colour,
                                 flags=extra)
                        assert create(pkg, cfg) in ok, (bits, sbe, method, colour, extra)
    # refused: 16-bit channels, their byte order, 3-byte pixels, the inverse direction, a kernel variant
    assert create(pkg, mk(64, 48, fmt="RGBP", out16=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGBP", out16=True, dst_big_endian=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGBP", dst_big_endian=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGBP", bits=12, out16=True)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGBP", flags=pkg.FLAG_DST_24BIT)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGB", flags=pkg.FLAG_DST_PLANAR)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGBP", flags=pkg.FLAG_RGB2BAYER)) == pkg.ERR_ARG
    assert create(pkg, mk(64, 48, fmt="RGBP", src_big_endian=True)) == pkg.ERR_ARG       # no depth to go with it
    for v in (1, 2, 3):
        assert create(pkg, mk(64, 48, fmt="RGBP", variant=v)) == pkg.ERR_ARG, v
    # the plan selectors describe the production kernels only
    sel, swap = (ctypes.c_uint32 * 4)(), ctypes.c_int()
    cfg = mk(64, 48, fmt="RGBP")
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
    pc.stream = pkg.make_cfg(66, 48, fmt="BGRP", out16=True)
    assert pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h)) == pkg.ERR_ARG
    pc.stream = pkg.make_cfg(66, 48, fmt=(1, 2, 3), flags=pkg.FLAG_DST_PLANAR)
    assert pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h)) == pkg.ERR_LAYOUT
    pc.stream = pkg.make_cfg(66, 48, fmt="GBR")
    rc = pkg.lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(h))
    assert rc in (pkg.OK, pkg.ERR_NO_DEVICE)
    if rc == pkg.OK:
        pkg.lib().mibayer_pool_destroy(h)


def test_planes_helper_is_a_view_of_numpy_and_torch_frames(pkg):
    """pkg.planes: (3, H, dst_stride)[:, :, :W] of the same memory, a numpy array or a torch uint8 tensor alike"""
    import numpy as np
    import torch
    w, h, stride = 22, 5, 32
    frame = np.arange(3 * h * stride, dtype=np.uint32).astype(np.uint8)
    v = pkg.planes(frame, w, h, stride)
    assert v.shape == (3, h, w) and np.shares_memory(v, frame)
    assert np.array_equal(v, frame.reshape(3, h, stride)[:, :, :w])
    assert pkg.planes(frame[:3 * h * 24], w, h).shape == (3, h, w)                # the default stride: ROUND_UP_4 (w)
    t = torch.from_numpy(frame)
    tv = pkg.planes(t, w, h, stride)
    assert tuple(tv.shape) == (3, h, w) and tv.dtype == torch.uint8 and tv.data_ptr() == t.data_ptr()
    assert np.array_equal(tv.numpy(), v)
