"""gst-plugins-bad_amd -- MI355X-native `bayer2rgb` (hot path of gst-plugins-bad's bayer plugin).

The product is native code:

  libmibayer.so   hand-written HIP kernels for gfx950 + the C ABI of include/mibayer.h
                  (csrc/mibayer_kernels.hip, csrc/mibayer_abi.hip)
  libgstbayer.so  GStreamer plugin `bayer`, element `bayer2rgb`: registration, pad templates and
                  caps negotiation identical to reference gst/bayer/gstbayer2rgb.c, `transform`
                  calling the C ABI (gst/gstmibayerelement.c)

This Python module is only the ctypes harness that tests/ and bench.py use to drive the C ABI
(the directory name is not an importable identifier; load it through
`__graft_entry__.load_package()`, which registers it as `gst_plugins_bad_amd`).  There is no Python
or CPU compute path here: every compute call goes to libmibayer.so and raises `MibayerError` if the
library or a GPU is missing.
"""
import ctypes
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
LIB_PATH = os.environ.get("MIBAYER_LIB_PATH") or os.path.join(HERE, "libmibayer.so")   # override: A/B of two builds
LAB_LIB_PATH = os.path.join(HERE, "libmibayer_lab.so")      # `make lab`: + experiment arms and tuning environment
PLUGIN_PATH = os.path.join(HERE, "libgstbayer.so")
HEADER_PATH = os.path.join(ROOT, "include", "mibayer.h")

# Bayer orders, numbering of reference gstbayer2rgb.c:95-101
PATTERNS = {"bggr": 0, "gbrg": 1, "grbg": 2, "rggb": 3}
# (r_off, g_off, b_off) = GST_VIDEO_INFO_COMP_OFFSET of the 8 src-template formats,
# reference gstbayer2rgb.c:134-135, :268-271
FORMATS = {
    "RGBx": (0, 1, 2), "xRGB": (1, 2, 3), "BGRx": (2, 1, 0), "xBGR": (3, 2, 1),
    "RGBA": (0, 1, 2), "ARGB": (1, 2, 3), "BGRA": (2, 1, 0), "ABGR": (3, 2, 1),
}

# 16-bit-per-channel output (MIBAYER_FLAG_DST_16BIT): (r_off, g_off, b_off) in 16-bit CHANNELS of the 8-byte pixel.
# ARGB64 is the one the GStreamer video library of the element knows; the other three are the same layouts as above
FORMATS16 = {"ARGB64": (1, 2, 3), "RGBA64": (0, 1, 2), "BGRA64": (2, 1, 0), "ABGR64": (3, 2, 1)}
# packed 24-bit output (MIBAYER_FLAG_DST_24BIT): byte offsets inside the 3-byte pixel -- RGBx / BGRx without byte 3
FORMATS24 = {"RGB": (0, 1, 2), "BGR": (2, 1, 0)}
# planar 8-bit output (MIBAYER_FLAG_DST_PLANAR): the PLANE INDICES of R, G, B; the other three permutations of (0, 1, 2)
# go in as a tuple with flags=FLAG_DST_PLANAR
FORMATS_PLANAR = {"RGBP": (0, 1, 2), "BGRP": (2, 1, 0), "GBR": (2, 0, 1)}
SRC_BITS = (10, 12, 14, 16)     # MIBAYER_FLAG_SRC_BITS(n) values besides 0 (the 8-bit mosaic)

PLAN_DEFAULT, PLAN_MEASURED, PLAN_CACHED, PLAN_SET = 0, 1, 2, 3
FRAME_QUEUES = 4                # MIBAYER_FRAME_QUEUES
OK = 0
ERR_ARG, ERR_GEOMETRY, ERR_LAYOUT, ERR_NO_DEVICE, ERR_HIP, ERR_NOMEM, ERR_BUSY, ERR_EMPTY, ERR_TIMEOUT = (
    -1, -2, -3, -4, -5, -6, -7, -8, -9)


class MibayerError(RuntimeError):
    def __init__(self, status, where=""):
        self.status = status
        msg = "mibayer status %d" % status
        try:
            L = lib()
            msg = L.mibayer_strerror(status).decode()
            hip = L.mibayer_last_hip_error().decode()
            if status == ERR_HIP and hip:
                msg += " [" + hip + "]"
        except Exception:  # pragma: no cover - library itself unavailable
            pass
        super().__init__(("%s: " % where if where else "") + msg)


class Cfg(ctypes.Structure):
    """struct mibayer_cfg (include/mibayer.h)."""
    _fields_ = [
        ("struct_size", ctypes.c_uint32),
        ("width", ctypes.c_int32), ("height", ctypes.c_int32),
        ("src_stride", ctypes.c_int32), ("dst_stride", ctypes.c_int32),
        ("pattern", ctypes.c_int32),
        ("r_off", ctypes.c_int32), ("g_off", ctypes.c_int32), ("b_off", ctypes.c_int32),
        ("device", ctypes.c_int32), ("inflight", ctypes.c_int32), ("variant", ctypes.c_int32),
        ("flags", ctypes.c_uint32),
    ]


MAX_SHARDS = 16
FLAG_HIPGRAPH = 1
FLAG_RGB2BAYER = 2
FLAG_HIPGRAPH_CHAIN = 4
FLAG_SRC_BITS_MASK = 0x1F << 8
FLAG_SRC_BIG_ENDIAN = 1 << 13
FLAG_DST_16BIT = 1 << 14
FLAG_DST_BIG_ENDIAN = 1 << 15
FLAG_DST_24BIT = 1 << 21        # 3-byte pixels, RGB / BGR; dst_stride defaults to ROUND_UP_4(3 * width)
FLAG_DST_PLANAR = 1 << 22       # three planes of dst_stride x height bytes; dst_stride defaults to ROUND_UP_4(width)
FLAG_MHC = 1 << 16              # Malvar-He-Cutler demosaic instead of the reference's bilinear one
FLAG_HALF = 1 << 23             # half-size demosaic: one RGB pixel per CFA quad, output W / 2 x H >> 1
METHODS = {"bilinear": 0, "mhc": FLAG_MHC, "half": FLAG_HALF}   # the `method` keyword of make_cfg / Context / Pool
FLAG_COLOUR = 1 << 19           # fused colour stage: black level, Q12 matrix, tone curve (struct mibayer_colour)
TONE_LINEAR, TONE_SRGB, TONE_GAMMA = 0, 1, 2


def FLAG_SRC_BITS(n):
    """MIBAYER_FLAG_SRC_BITS(n): 16-bit-word samples with n significant bits (n = 0: the 8-bit mosaic)."""
    return (int(n) << 8) & 0xFFFFFFFF


def deep_flags(bits=0, src_big_endian=False, out16=False, dst_big_endian=False):
    """cfg.flags of a deep context (include/mibayer.h, MIBAYER_FLAG_SRC_BITS); no validation here, the library does it."""
    return (FLAG_SRC_BITS(bits) | (FLAG_SRC_BIG_ENDIAN if src_big_endian else 0)
            | (FLAG_DST_16BIT if out16 else 0) | (FLAG_DST_BIG_ENDIAN if dst_big_endian else 0))


class HostStats(ctypes.Structure):
    """struct mibayer_host_stats (include/mibayer.h)."""
    _fields_ = [("submits", ctypes.c_uint64), ("waits", ctypes.c_uint64), ("polls", ctypes.c_uint64),
                ("naps", ctypes.c_uint64), ("submit_cpu_ms", ctypes.c_double), ("wait_cpu_ms", ctypes.c_double),
                ("wait_wall_ms", ctypes.c_double)]

    def as_dict(self):
        return {k: getattr(self, k) for k, _ in self._fields_}


class Colour(ctypes.Structure):
    """struct mibayer_colour (include/mibayer.h): the parameters of a FLAG_COLOUR context.  Colour() is the identity;
    Colour.make() builds one with the library's helpers (mibayer_colour_matrix / mibayer_colour_tone)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("black", ctypes.c_int32 * 3), ("matrix", ctypes.c_int32 * 9),
                ("has_tone", ctypes.c_int32), ("tone", ctypes.c_uint32 * 257)]

    def __init__(self, black=(0, 0, 0), matrix=(4096, 0, 0, 0, 4096, 0, 0, 0, 4096), tone=None):
        super().__init__()
        self.struct_size = ctypes.sizeof(Colour)
        self.black[:] = [int(v) for v in (black if np.ndim(black) else (black,) * 3)]
        self.matrix[:] = [int(v) for v in np.asarray(matrix).reshape(-1)]
        self.has_tone = 0 if tone is None else 1
        if tone is not None:
            self.tone[:] = [int(v) for v in tone]

    @classmethod
    def make(cls, black=0, gains=(1.0, 1.0, 1.0), ccm=None, curve=None, gamma=2.2):
        """curve: None (no tone curve) or TONE_LINEAR / TONE_SRGB / TONE_GAMMA"""
        return cls(black, colour_matrix(gains, ccm), None if curve is None else colour_tone(curve, gamma))

    def tone_table(self):
        return np.array(self.tone[:], np.int64) if self.has_tone else None


def colour_matrix(gains=(1.0, 1.0, 1.0), ccm=None):
    """mibayer_colour_matrix: round(ccm x diag(gains) x 4096) as 9 ints (no device needed)"""
    out = (ctypes.c_int32 * 9)()
    g = (ctypes.c_double * 3)(*[float(v) for v in gains])
    c = None if ccm is None else (ctypes.c_double * 9)(*[float(v) for v in np.asarray(ccm).reshape(-1)])
    _check(lib().mibayer_colour_matrix(g, c, out), "mibayer_colour_matrix")
    return list(out)


def colour_tone(curve, gamma=2.2):
    """mibayer_colour_tone: the 257-entry table of TONE_LINEAR / TONE_SRGB / TONE_GAMMA (no device needed)"""
    out = (ctypes.c_uint32 * 257)()
    _check(lib().mibayer_colour_tone(int(curve), float(gamma), out), "mibayer_colour_tone")
    return list(out)


class StatsZone(ctypes.Structure):
    """struct mibayer_stats_zone (include/mibayer.h): per CFA site s = 2 (y & 1) + (x & 1) of one zone"""
    _fields_ = [("sum", ctypes.c_uint64 * 4), ("count", ctypes.c_uint32 * 4), ("clipped", ctypes.c_uint32 * 4)]


# numpy view of an array of StatsZone
STATS_DTYPE = np.dtype([("sum", np.uint64, 4), ("count", np.uint32, 4), ("clipped", np.uint32, 4)])
STATS_MAX_ZONES = 64


def stats_grey_world(zones, pattern, black=None):
    """mibayer_stats_grey_world: (ok, (gain_r, 1, gain_b)) from a STATS_DTYPE array of zones (no device needed)"""
    zones = np.ascontiguousarray(zones, STATS_DTYPE).reshape(-1)
    gains = (ctypes.c_double * 3)()
    b = None if black is None else (ctypes.c_double * 3)(*[float(v) for v in black])
    pat = PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    rc = lib().mibayer_stats_grey_world(_ptr(zones), zones.size, pat, b, gains)
    if rc < 0:
        raise MibayerError(rc, "mibayer_stats_grey_world")
    return rc, tuple(gains)


class FocusZone(ctypes.Structure):
    """struct mibayer_focus_zone (include/mibayer.h): per CFA site s = 2 (y & 1) + (x & 1) of one zone"""
    _fields_ = [("h", ctypes.c_uint64 * 4), ("v", ctypes.c_uint64 * 4), ("nh", ctypes.c_uint32 * 4),
                ("nv", ctypes.c_uint32 * 4)]


# numpy view of an array of FocusZone
FOCUS_DTYPE = np.dtype([("h", np.uint64, 4), ("v", np.uint64, 4), ("nh", np.uint32, 4), ("nv", np.uint32, 4)])


def focus_score(zones, pattern, colour=1, weights=None):
    """mibayer_focus_score: (ok, score) from a FOCUS_DTYPE array of zones; colour 0 / 1 / 2 = R / G / B, 3 = all sites;
    weights: None or one double per zone (no device needed)"""
    zones = np.ascontiguousarray(zones, FOCUS_DTYPE).reshape(-1)
    w = None
    if weights is not None:
        w = np.ascontiguousarray(weights, np.float64).reshape(-1)
        assert w.size == zones.size
    pat = PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    score = ctypes.c_double(-1.0)
    rc = lib().mibayer_focus_score(_ptr(zones), zones.size, pat, int(colour), None if w is None else _ptr(w),
                                   ctypes.byref(score))
    if rc < 0:
        raise MibayerError(rc, "mibayer_focus_score")
    return rc, score.value


SHADING_MAX_NODES = 129


class Shading(ctypes.Structure):
    """struct mibayer_shading (include/mibayer.h): cells of (1 << kx) x (1 << ky) pixels, a black level per CFA site
    and the Q12 gain table g[site][ny][nx] (host memory; the library copies it).  Shading(kx, ky, table, black) keeps
    the array alive as long as the structure lives."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("cell_log2_x", ctypes.c_int32), ("cell_log2_y", ctypes.c_int32),
                ("black", ctypes.c_uint32 * 4), ("table", ctypes.c_void_p)]

    def __init__(self, kx=4, ky=4, table=None, black=(0, 0, 0, 0)):
        super().__init__()
        self.struct_size = ctypes.sizeof(Shading)
        self.cell_log2_x, self.cell_log2_y = int(kx), int(ky)
        self.black[:] = [int(v) for v in black]
        self._table = None if table is None else np.ascontiguousarray(table, np.uint16)
        self.table = None if table is None else self._table.ctypes.data


def shading_nodes(width, height, kx, ky):
    """mibayer_shading_nodes: (nx, ny) of a width x height frame (no device needed)"""
    nx, ny = ctypes.c_int(0), ctypes.c_int(0)
    _check(lib().mibayer_shading_nodes(int(width), int(height), int(kx), int(ky), ctypes.byref(nx), ctypes.byref(ny)),
           "mibayer_shading_nodes")
    return nx.value, ny.value


def stats_shading(zones, width, height, black, kx, ky, max_gain):
    """mibayer_stats_shading: (ok, (4, ny, nx) uint16 Q12 table) from the (zones_y, zones_x) STATS_DTYPE zones of a flat
    field; black may be None (no device needed)"""
    zones = np.ascontiguousarray(zones, STATS_DTYPE)
    zones_y, zones_x = zones.shape
    nx, ny = shading_nodes(width, height, kx, ky)
    out = np.zeros((4, ny, nx), np.uint16)
    b = None if black is None else (ctypes.c_uint32 * 4)(*[int(v) for v in black])
    rc = lib().mibayer_stats_shading(_ptr(zones), zones_x, zones_y, int(width), int(height), b, int(kx), int(ky),
                                     float(max_gain), _ptr(out))
    if rc < 0:
        raise MibayerError(rc, "mibayer_stats_shading")
    return rc, out


DPC_MAX_DEFECTS = 65536


class Dpc(ctypes.Structure):
    """struct mibayer_dpc (include/mibayer.h): the hot and cold thresholds (-1 = off) and the list of known defects,
    (n, 2) of (x, y) in host memory (the library copies it).  Dpc(hot, cold, defects) keeps the array alive as long as
    the structure lives."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("hot", ctypes.c_int32), ("cold", ctypes.c_int32),
                ("ndefects", ctypes.c_uint32), ("defects", ctypes.c_void_p)]

    def __init__(self, hot=-1, cold=-1, defects=None):
        super().__init__()
        self.struct_size = ctypes.sizeof(Dpc)
        self.hot, self.cold = int(hot), int(cold)
        self._list = None if defects is None else np.ascontiguousarray(defects, np.uint32).reshape(-1, 2)
        self.ndefects = 0 if defects is None else len(self._list)
        self.defects = None if defects is None or not len(self._list) else self._list.ctypes.data


NR_NODES = 17


class Nr(ctypes.Structure):
    """struct mibayer_nr (include/mibayer.h): the threshold curve of the noise reduction, 17 nodes at the levels
    i << (depth - 4).  Nr(curve): a sequence of 17 thresholds, or one number for a constant curve."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("curve", ctypes.c_uint16 * NR_NODES), ("reserved", ctypes.c_uint16)]

    def __init__(self, curve=0):
        super().__init__()
        self.struct_size = ctypes.sizeof(Nr)
        nodes = [int(curve)] * NR_NODES if np.isscalar(curve) else [int(v) for v in curve]
        if len(nodes) != NR_NODES:
            raise ValueError("a noise reduction curve has %d nodes" % NR_NODES)
        self.curve[:] = nodes

    def nodes(self):
        return list(self.curve)


def nr_curve(bits, black=0.0, read_noise=2.0, shot_noise=0.0, strength=1.0):
    """mibayer_nr_curve: the Nr of a sensor's noise model at depth `bits`"""
    out = Nr()
    _check(lib().mibayer_nr_curve(int(bits), float(black), float(read_noise), float(shot_noise), float(strength),
                                  ctypes.byref(out)), "mibayer_nr_curve")
    return out


HIST_BINS = 256


class Hist(ctypes.Structure):
    """struct mibayer_hist (include/mibayer.h): bin[site][b], site s = 2 (y & 1) + (x & 1)"""
    _fields_ = [("bin", (ctypes.c_uint32 * HIST_BINS) * 4)]


# numpy view of one Hist: a (4, 256) array of HIST_DTYPE
HIST_DTYPE = np.dtype(np.uint32)
HIST_SHAPE = (4, HIST_BINS)


def _hist_arg(hist):
    hist = np.ascontiguousarray(hist, HIST_DTYPE)
    assert hist.shape == HIST_SHAPE
    return hist


def hist_percentile(hist, pattern, colour, fraction):
    """mibayer_hist_percentile: (ok, bin) of colour 0 / 1 / 2 = R / G / B or 3 = all sites (no device needed)"""
    hist = _hist_arg(hist)
    b = ctypes.c_int(0)
    pat = PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    rc = lib().mibayer_hist_percentile(_ptr(hist), pat, int(colour), float(fraction), ctypes.byref(b))
    if rc < 0:
        raise MibayerError(rc, "mibayer_hist_percentile")
    return rc, b.value


def hist_exposure(hist, pattern, depth, black, gains, fraction, target, max_gain):
    """mibayer_hist_exposure: (ok, exposure factor); black / gains may be None (no device needed)"""
    hist = _hist_arg(hist)
    x = ctypes.c_double(0.0)
    b = None if black is None else (ctypes.c_double * 3)(*[float(v) for v in black])
    g = None if gains is None else (ctypes.c_double * 3)(*[float(v) for v in gains])
    pat = PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    rc = lib().mibayer_hist_exposure(_ptr(hist), pat, int(depth), b, g, float(fraction), float(target),
                                     float(max_gain), ctypes.byref(x))
    if rc < 0:
        raise MibayerError(rc, "mibayer_hist_exposure")
    return rc, x.value


class PoolCfg(ctypes.Structure):
    """struct mibayer_pool_cfg (include/mibayer.h)."""
    _fields_ = [("struct_size", ctypes.c_uint32), ("stream", Cfg), ("ndevices", ctypes.c_int32),
                ("devices", ctypes.c_int32 * MAX_SHARDS)]


_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p
_lib = None

# every symbol include/mibayer.h declares: name -> (restype, argtypes)
ABI = {
    "mibayer_abi_version": (ctypes.c_int, []),
    "mibayer_device_pci_bus_id": (ctypes.c_int, [ctypes.c_int, ctypes.c_char_p, ctypes.c_size_t]),
    "mibayer_is_lab_build": (ctypes.c_int, []),
    "mibayer_device_count": (ctypes.c_int, []),
    "mibayer_strerror": (ctypes.c_char_p, [ctypes.c_int]),
    "mibayer_last_hip_error": (ctypes.c_char_p, []),
    "mibayer_create": (ctypes.c_int, [ctypes.POINTER(Cfg), ctypes.POINTER(_vp)]),
    "mibayer_destroy": (None, [_vp]),
    "mibayer_get_cfg": (ctypes.c_int, [_vp, ctypes.POINTER(Cfg)]),
    "mibayer_process_host": (ctypes.c_int, [_vp, _vp, _vp]),
    "mibayer_submit": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "mibayer_wait": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "mibayer_pending": (ctypes.c_int, [_vp]),
    "mibayer_set_wait_timeout": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mibayer_pool_set_wait_timeout": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mibayer_set_wait_spin": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mibayer_pool_set_wait_spin": (ctypes.c_int, [_vp, ctypes.c_int]),
    "mibayer_get_host_stats": (ctypes.c_int, [_vp, ctypes.POINTER(HostStats)]),
    "mibayer_pool_get_host_stats": (ctypes.c_int, [_vp, ctypes.POINTER(HostStats)]),
    "mibayer_pool_reclaim": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "mibayer_pool_lost": (ctypes.c_int, [_vp]),
    "mibayer_deferred_frees": (ctypes.c_int, []),
    "mibayer_wedged_contexts": (ctypes.c_int, []),
    "mibayer_pool_inject_stall": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int]),
    "mibayer_pool_create": (ctypes.c_int, [ctypes.POINTER(PoolCfg), ctypes.POINTER(_vp)]),
    "mibayer_pool_destroy": (None, [_vp]),
    "mibayer_pool_capacity": (ctypes.c_int, [_vp]),
    "mibayer_pool_pending": (ctypes.c_int, [_vp]),
    "mibayer_pool_submit": (ctypes.c_int, [_vp, _vp, _vp, _vp]),
    "mibayer_pool_wait": (ctypes.c_int, [_vp, ctypes.POINTER(_vp)]),
    "mibayer_pool_alive": (ctypes.c_int, [_vp]),
    "mibayer_pool_take_failure": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                                 ctypes.c_char_p, ctypes.c_size_t]),
    "mibayer_pool_inject_fault": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_longlong]),
    "mibayer_process_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                              ctypes.c_int, _vp]),
    "mibayer_process_device_list": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.c_int, _vp]),
    "mibayer_ctx_stream": (_vp, [_vp]),
    "mibayer_sync": (ctypes.c_int, [_vp]),
    "mibayer_time_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t,
                                           ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.POINTER(ctypes.c_float)]),
    "mibayer_autotune": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int,
                                        ctypes.c_char_p, ctypes.c_size_t]),
    "mibayer_autotune_list": (ctypes.c_int, [_vp, ctypes.POINTER(_vp), ctypes.POINTER(_vp), ctypes.c_int,
                                             ctypes.c_char_p, ctypes.c_size_t]),
    "mibayer_copy_plan": (ctypes.c_int, [_vp, _vp]),
    "mibayer_get_plan": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                        ctypes.POINTER(ctypes.c_int)]),
    "mibayer_set_plan": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mibayer_get_plan_for": (ctypes.c_int, [_vp, ctypes.c_int] + [ctypes.POINTER(ctypes.c_int)] * 4),
    "mibayer_set_plan_for": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mibayer_ctx_frame_queue": (_vp, [_vp, ctypes.c_int]),
    "mibayer_plan_source": (ctypes.c_int, [_vp]),
    "mibayer_plan_from_cache": (ctypes.c_int, [_vp]),
    "mibayer_plan_cache_clear": (None, []),
    "mibayer_host_alloc": (_vp, [ctypes.c_size_t]),
    "mibayer_host_free": (None, [_vp]),
    "mibayer_host_alloc_near": (_vp, [ctypes.c_int, ctypes.c_size_t]),
    "mibayer_device_numa_node": (ctypes.c_int, [ctypes.c_int]),
    "mibayer_host_numa_node": (ctypes.c_int, [_vp]),
    "mibayer_host_is_pinned": (ctypes.c_int, [_vp]),
    "mibayer_device_alloc": (_vp, [_vp, ctypes.c_size_t]),
    "mibayer_device_free": (None, [_vp, _vp]),
    "mibayer_copy_to_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "mibayer_copy_from_device": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_size_t]),
    "mibayer_dev_alloc": (_vp, [ctypes.c_int, ctypes.c_size_t]),
    "mibayer_dev_free": (None, [ctypes.c_int, _vp]),
    "mibayer_dev_upload": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_size_t]),
    "mibayer_dev_download": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_size_t]),
    "mibayer_dev_stream_create": (_vp, [ctypes.c_int]),
    "mibayer_dev_stream_destroy": (None, [ctypes.c_int, _vp]),
    "mibayer_dev_upload_async": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp]),
    "mibayer_dev_download_async": (ctypes.c_int, [ctypes.c_int, _vp, _vp, ctypes.c_size_t, _vp]),
    "mibayer_dev_event_query": (ctypes.c_int, [ctypes.c_int, _vp]),
    "mibayer_dev_event_create": (_vp, [ctypes.c_int]),
    "mibayer_dev_event_destroy": (None, [ctypes.c_int, _vp]),
    "mibayer_dev_event_record": (ctypes.c_int, [ctypes.c_int, _vp, _vp]),
    "mibayer_dev_event_wait": (ctypes.c_int, [ctypes.c_int, _vp]),
    "mibayer_dev_stream_wait_event": (ctypes.c_int, [ctypes.c_int, _vp, _vp]),
    "mibayer_fill_synthetic": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_uint32,
                                              ctypes.c_int, ctypes.c_uint32, _vp]),
    "mibayer_variant_count": (ctypes.c_int, []),
    "mibayer_variant_name": (ctypes.c_char_p, [ctypes.c_int]),
    "mibayer_auto_variant": (ctypes.c_int, [ctypes.c_int]),
    "mibayer_frame_class_variant": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mibayer_known_width_plan": (ctypes.c_int, [ctypes.c_int, ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mibayer_ctx_variant_name": (ctypes.c_char_p, [_vp]),
    "mibayer_plan_selectors": (ctypes.c_int, [ctypes.POINTER(Cfg), ctypes.POINTER(ctypes.c_uint32 * 4),
                                              ctypes.POINTER(ctypes.c_int)]),
    "mibayer_launch_geometry": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_int64), ctypes.POINTER(ctypes.c_int),
                                               ctypes.POINTER(ctypes.c_int64)]),
    "mibayer_block_to_tile": (ctypes.c_int64, [ctypes.c_int64, ctypes.c_int, ctypes.c_int64, ctypes.c_int]),
    "mibayer_colour_init": (None, [ctypes.POINTER(Colour)]),
    "mibayer_set_colour": (ctypes.c_int, [_vp, ctypes.POINTER(Colour)]),
    "mibayer_get_colour": (ctypes.c_int, [_vp, ctypes.POINTER(Colour)]),
    "mibayer_pool_set_colour": (ctypes.c_int, [_vp, ctypes.POINTER(Colour)]),
    "mibayer_colour_matrix": (ctypes.c_int, [ctypes.POINTER(ctypes.c_double), ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_int32)]),
    "mibayer_colour_tone": (ctypes.c_int, [ctypes.c_int, ctypes.c_double, ctypes.POINTER(ctypes.c_uint32)]),
    "mibayer_stats_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]),
    "mibayer_set_stats": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]),
    "mibayer_frame_stats": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "mibayer_pool_set_stats": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32]),
    "mibayer_pool_frame_stats": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "mibayer_stats_grey_world": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                                ctypes.POINTER(ctypes.c_double)]),
    "mibayer_focus_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                            ctypes.c_uint32, _vp, _vp]),
    "mibayer_set_focus": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]),
    "mibayer_frame_focus": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "mibayer_pool_set_focus": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_uint32]),
    "mibayer_pool_frame_focus": (ctypes.c_int, [_vp, _vp, ctypes.c_int]),
    "mibayer_focus_score": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, _vp,
                                           ctypes.POINTER(ctypes.c_double)]),
    "mibayer_hist_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                           ctypes.c_int, ctypes.c_int, _vp, _vp]),
    "mibayer_set_hist": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int]),
    "mibayer_frame_hist": (ctypes.c_int, [_vp, _vp]),
    "mibayer_pool_set_hist": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.c_int]),
    "mibayer_pool_frame_hist": (ctypes.c_int, [_vp, _vp]),
    "mibayer_hist_percentile": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_double,
                                               ctypes.POINTER(ctypes.c_int)]),
    "mibayer_hist_exposure": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.POINTER(ctypes.c_double),
                                             ctypes.POINTER(ctypes.c_double), ctypes.c_double, ctypes.c_double,
                                             ctypes.c_double, ctypes.POINTER(ctypes.c_double)]),
    "mibayer_shading_nodes": (ctypes.c_int, [ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_int), ctypes.POINTER(ctypes.c_int)]),
    "mibayer_set_shading": (ctypes.c_int, [_vp, ctypes.POINTER(Shading)]),
    "mibayer_get_shading": (ctypes.c_int, [_vp, ctypes.POINTER(Shading)]),
    "mibayer_shade_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "mibayer_pool_set_shading": (ctypes.c_int, [_vp, ctypes.POINTER(Shading)]),
    "mibayer_set_dpc": (ctypes.c_int, [_vp, ctypes.POINTER(Dpc)]),
    "mibayer_get_dpc": (ctypes.c_int, [_vp, ctypes.POINTER(Dpc)]),
    "mibayer_dpc_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "mibayer_pool_set_dpc": (ctypes.c_int, [_vp, ctypes.POINTER(Dpc)]),
    "mibayer_set_nr": (ctypes.c_int, [_vp, ctypes.POINTER(Nr)]),
    "mibayer_get_nr": (ctypes.c_int, [_vp, ctypes.POINTER(Nr)]),
    "mibayer_nr_device": (ctypes.c_int, [_vp, _vp, ctypes.c_size_t, _vp, ctypes.c_size_t, ctypes.c_int, _vp]),
    "mibayer_pool_set_nr": (ctypes.c_int, [_vp, ctypes.POINTER(Nr)]),
    "mibayer_nr_curve": (ctypes.c_int, [ctypes.c_int, ctypes.c_double, ctypes.c_double, ctypes.c_double,
                                        ctypes.c_double, ctypes.POINTER(Nr)]),
    "mibayer_stats_shading": (ctypes.c_int, [_vp, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                                             ctypes.POINTER(ctypes.c_uint32), ctypes.c_int, ctypes.c_int,
                                             ctypes.c_double, _vp]),
}


def device_pci_bus_id(device):
    """'0000:c1:00.0' of a HIP ordinal (None if the runtime does not say)."""
    buf = ctypes.create_string_buffer(32)
    if lib().mibayer_device_pci_bus_id(device, buf, len(buf)) != OK:
        return None
    return buf.value.decode()


def build(quiet=True):
    """Compile libmibayer.so (hipcc, gfx950), the lab build beside it and, when GStreamer headers exist, libgstbayer.so."""
    subprocess.run(["make", "-C", HERE, "all", "lab"], check=True,
                   stdout=subprocess.DEVNULL if quiet else None)


def lib():
    """The C ABI.  Fails loudly when the HIP library has not been built."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MibayerErrorNoLib(
                "%s is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(there is no CPU fallback)" % LIB_PATH)
        L = ctypes.CDLL(LIB_PATH)
        for name, (res, args) in ABI.items():
            fn = getattr(L, name)
            fn.restype = res
            fn.argtypes = args
        if L.mibayer_abi_version() != 5:
            raise MibayerErrorNoLib("libmibayer.so ABI version mismatch")
        _lib = L
    return _lib


class MibayerErrorNoLib(RuntimeError):
    pass


class FrameLost(MibayerError):
    """mibayer_pool_wait handed a frame back as lost (MIBAYER_ERR_TIMEOUT with its tag): the frame was in flight on a
    device that ran into the wait deadline; its buffers stay the device's until Pool.reclaim().  The stream carries on
    as long as Pool.alive() > 0."""

    def __init__(self, tag):
        super().__init__(ERR_TIMEOUT, "mibayer_pool_wait (frame lost)")
        self.tag = tag


def device_count():
    return lib().mibayer_device_count()


def variant_names():
    L = lib()
    return [L.mibayer_variant_name(i).decode() for i in range(L.mibayer_variant_count())]


def _check(rc, where):
    if rc != OK:
        raise MibayerError(rc, where)


def _ptr(a):
    return ctypes.c_void_p(a.ctypes.data)


def make_cfg(width, height, pattern="bggr", fmt="RGBx", src_stride=0, dst_stride=0, device=-1,
             inflight=0, variant=0, flags=0, bits=0, src_big_endian=False, out16=False, dst_big_endian=False,
             method="bilinear", colour=None):
    """bits / src_big_endian / out16 / dst_big_endian: the deep-sample flags (or pass them in `flags`); a FORMATS16
    name implies out16, a FORMATS24 name ("RGB", "BGR") FLAG_DST_24BIT, a FORMATS_PLANAR name FLAG_DST_PLANAR.
    method: "bilinear" (the reference's, bit-exact), "mhc" (Malvar-He-Cutler, FLAG_MHC) or "half" (FLAG_HALF: one pixel
    per CFA quad; width / height stay the mosaic's).
    colour: None / False = no colour stage; True or a Colour = FLAG_COLOUR (Context / Pool apply the Colour)"""
    if colour is not None and colour is not False:
        flags |= FLAG_COLOUR
    if method not in METHODS:
        raise ValueError("method must be one of %s, not %r" % (sorted(METHODS), method))
    flags |= METHODS[method]
    if isinstance(fmt, str) and fmt in FORMATS16:
        out16 = True
        r, g, b = FORMATS16[fmt]
    elif isinstance(fmt, str) and fmt in FORMATS24:
        flags |= FLAG_DST_24BIT
        r, g, b = FORMATS24[fmt]
    elif isinstance(fmt, str) and fmt in FORMATS_PLANAR:
        flags |= FLAG_DST_PLANAR
        r, g, b = FORMATS_PLANAR[fmt]
    else:
        r, g, b = FORMATS[fmt] if isinstance(fmt, str) else fmt
    flags |= deep_flags(bits, src_big_endian, out16, dst_big_endian)
    pat = PATTERNS[pattern] if isinstance(pattern, str) else int(pattern)
    return Cfg(ctypes.sizeof(Cfg), width, height, src_stride, dst_stride, pat, r, g, b,
               device, inflight, variant, flags)


def planes(frame, width, height, dst_stride=0):
    """A converted planar frame (MIBAYER_FLAG_DST_PLANAR, 3 * dst_stride * height bytes) viewed as (3, height, width):
    plane k, row y, the first `width` bytes of the stride; width / height are the OUTPUT's (a half-size context's
    out_width / out_height).  frame: a numpy uint8 array (the host path's), or a torch
    uint8 tensor -- over device memory the context converted into through its data_ptr(), as bench.py passes tensors --
    and the result is of the same kind.  A view of the same memory: nothing is copied or computed."""
    stride = dst_stride or (width + 3) & ~3
    return frame.reshape(3, height, stride)[:, :, :width]


class Pool:
    """Round-robin frame sharding over HIP devices (mibayer_pool): frame g -> devices[g % N]."""

    def __init__(self, devices, width, height, pattern="bggr", fmt="RGBx", inflight=2, flags=0, **deep):
        """deep: bits= / src_big_endian= / out16= / dst_big_endian= / method= / colour= (make_cfg)"""
        pc = PoolCfg()
        pc.struct_size = ctypes.sizeof(PoolCfg)
        pc.stream = make_cfg(width, height, pattern, fmt, inflight=inflight, flags=flags, **deep)
        pc.ndevices = len(devices)
        for i, d in enumerate(devices):
            pc.devices[i] = d
        self._h = _vp()
        _check(lib().mibayer_pool_create(ctypes.byref(pc), ctypes.byref(self._h)), "mibayer_pool_create")
        self.capacity = lib().mibayer_pool_capacity(self._h)
        self._zones = (1, 1)            # the grid frame_stats() asks for: the last one set_stats() switched on
        self._fzones = (1, 1)           # ... and frame_focus(): the last one set_focus() switched on
        if isinstance(deep.get("colour"), Colour):
            self.set_colour(deep["colour"])

    def set_colour(self, colour):
        """mibayer_pool_set_colour: the colour stage of every shard, for the frames submitted from now on"""
        _check(lib().mibayer_pool_set_colour(self._h, ctypes.byref(colour)), "mibayer_pool_set_colour")

    def set_stats(self, zones_x, zones_y, lo=0, hi=0):
        """mibayer_pool_set_stats: zone statistics for the frames submitted from now on; (0, 0) = off"""
        _check(lib().mibayer_pool_set_stats(self._h, zones_x, zones_y, lo, hi), "mibayer_pool_set_stats")
        if zones_x and zones_y:
            self._zones = (zones_y, zones_x)

    def frame_stats(self):
        """mibayer_pool_frame_stats: (zones_y, zones_x) STATS_DTYPE array of the frame wait() handed back last"""
        out = np.zeros(self._zones, STATS_DTYPE)
        _check(lib().mibayer_pool_frame_stats(self._h, _ptr(out), out.size), "mibayer_pool_frame_stats")
        return out

    def set_hist(self, on, window=(0, 0, 0, 0)):
        """mibayer_pool_set_hist: a histogram of `window` (x0, y0, w, h) for the frames submitted from now on"""
        _check(lib().mibayer_pool_set_hist(self._h, int(bool(on)), *window), "mibayer_pool_set_hist")

    def frame_hist(self):
        """mibayer_pool_frame_hist: (4, 256) HIST_DTYPE array of the frame wait() handed back last"""
        out = np.zeros(HIST_SHAPE, HIST_DTYPE)
        _check(lib().mibayer_pool_frame_hist(self._h, _ptr(out)), "mibayer_pool_frame_hist")
        return out

    def set_focus(self, zones_x, zones_y, thr=0):
        """mibayer_pool_set_focus: focus statistics for the frames submitted from now on; (0, 0) = off"""
        _check(lib().mibayer_pool_set_focus(self._h, zones_x, zones_y, thr), "mibayer_pool_set_focus")
        if zones_x and zones_y:
            self._fzones = (zones_y, zones_x)

    def frame_focus(self):
        """mibayer_pool_frame_focus: (zones_y, zones_x) FOCUS_DTYPE array of the frame wait() handed back last"""
        out = np.zeros(self._fzones, FOCUS_DTYPE)
        _check(lib().mibayer_pool_frame_focus(self._h, _ptr(out), out.size), "mibayer_pool_frame_focus")
        return out

    def set_shading(self, shading):
        """mibayer_pool_set_shading: the lens shading table (a Shading, or None = off) of the frames submitted from
        now on"""
        _check(lib().mibayer_pool_set_shading(self._h, None if shading is None else ctypes.byref(shading)),
               "mibayer_pool_set_shading")

    def set_dpc(self, dpc):
        """mibayer_pool_set_dpc: the defective pixel correction (a Dpc, or None = off) of the frames submitted from
        now on"""
        _check(lib().mibayer_pool_set_dpc(self._h, None if dpc is None else ctypes.byref(dpc)), "mibayer_pool_set_dpc")

    def set_nr(self, nr):
        """mibayer_pool_set_nr: the noise reduction curve (an Nr, or None = off) of the frames submitted from now on"""
        _check(lib().mibayer_pool_set_nr(self._h, None if nr is None else ctypes.byref(nr)), "mibayer_pool_set_nr")

    def submit(self, src, dst, tag=0):
        _check(lib().mibayer_pool_submit(self._h, _ptr(src), _ptr(dst), _vp(tag)), "mibayer_pool_submit")

    def wait(self):
        tag = _vp()
        rc = lib().mibayer_pool_wait(self._h, ctypes.byref(tag))
        if rc == ERR_TIMEOUT and tag.value:
            raise FrameLost(tag.value)          # (whether the stream carries on is alive() > 0)
        _check(rc, "mibayer_pool_wait")
        return tag.value or 0

    def reclaim(self):
        """Tags of lost frames whose device has let go of their buffers since (non-blocking)."""
        out = []
        while True:
            tag = _vp()
            if lib().mibayer_pool_reclaim(self._h, ctypes.byref(tag)) != OK:
                return out
            out.append(tag.value or 0)

    def lost(self):
        return lib().mibayer_pool_lost(self._h)

    def set_wait_spin(self, us):
        _check(lib().mibayer_pool_set_wait_spin(self._h, us), "mibayer_pool_set_wait_spin")

    def host_stats(self):
        st = HostStats()
        _check(lib().mibayer_pool_get_host_stats(self._h, ctypes.byref(st)), "mibayer_pool_get_host_stats")
        return st.as_dict()

    def pending(self):
        return lib().mibayer_pool_pending(self._h)

    def alive(self):
        return lib().mibayer_pool_alive(self._h)

    def set_wait_timeout(self, ms):
        _check(lib().mibayer_pool_set_wait_timeout(self._h, ms), "mibayer_pool_set_wait_timeout")

    def inject_stall(self, shard, ms):
        _check(lib().mibayer_pool_inject_stall(self._h, shard, ms), "mibayer_pool_inject_stall")

    def inject_fault(self, shard, after_frames):
        _check(lib().mibayer_pool_inject_fault(self._h, shard, after_frames), "mibayer_pool_inject_fault")

    def take_failure(self):
        """(devices dropped since the last call, ordinal of the latest, devices left, message)"""
        dev, alive = ctypes.c_int(-1), ctypes.c_int(0)
        buf = ctypes.create_string_buffer(300)
        n = lib().mibayer_pool_take_failure(self._h, ctypes.byref(dev), ctypes.byref(alive), buf, len(buf))
        return n, dev.value, alive.value, buf.value.decode()

    def close(self):
        if getattr(self, "_h", None):
            lib().mibayer_pool_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """One negotiated stream == one mibayer_ctx (what the element creates in set_caps).

    `fmt` is a GStreamer video format name of the src template (RGBx, BGRx, ...) or an explicit
    (r_off, g_off, b_off) triple.
    """

    def __init__(self, width, height, pattern="bggr", fmt="RGBx", src_stride=0, dst_stride=0,
                 device=-1, inflight=0, variant=0, flags=0, **deep):
        """deep: bits= / src_big_endian= / out16= / dst_big_endian= / method= / colour= (make_cfg); a deep context takes
        its source as bytes or as any integer array whose bytes are the frame (uint16 words)"""
        cfg = make_cfg(width, height, pattern, fmt, src_stride, dst_stride, device, inflight, variant, flags, **deep)
        self._h = _vp()
        _check(lib().mibayer_create(ctypes.byref(cfg), ctypes.byref(self._h)), "mibayer_create")
        out = Cfg()
        _check(lib().mibayer_get_cfg(self._h, ctypes.byref(out)), "mibayer_get_cfg")
        self.cfg = out
        self.width, self.height = out.width, out.height
        self.src_stride, self.dst_stride = out.src_stride, out.dst_stride
        self.src_bytes = out.src_stride * out.height
        self.planar = bool(out.flags & FLAG_DST_PLANAR)
        self.half = bool(out.flags & FLAG_HALF)
        # the output frame's pixels: the mosaic's, or one per CFA quad (FLAG_HALF; the last row of an odd height is dropped)
        self.out_width, self.out_height = (out.width // 2, out.height >> 1) if self.half else (out.width, out.height)
        self.dst_rows = (3 if self.planar else 1) * self.out_height     # rows of dst_stride bytes in a frame (stacked planes)
        self.dst_bytes = out.dst_stride * self.dst_rows
        self.variant_name = lib().mibayer_ctx_variant_name(self._h).decode()
        self.deep = bool(out.flags & (FLAG_SRC_BITS_MASK | FLAG_DST_16BIT | FLAG_DST_24BIT | FLAG_DST_PLANAR))
        self.method = "mhc" if out.flags & FLAG_MHC else "half" if self.half else "bilinear"
        self.colour = bool(out.flags & FLAG_COLOUR)
        self._zones = (1, 1)            # the grid frame_stats() asks for: the last one set_stats() switched on
        self._fzones = (1, 1)           # ... and frame_focus(): the last one set_focus() switched on
        if isinstance(deep.get("colour"), Colour):
            self.set_colour(deep["colour"])

    def set_colour(self, colour):
        """mibayer_set_colour: applies to the launches enqueued from now on"""
        _check(lib().mibayer_set_colour(self._h, ctypes.byref(colour)), "mibayer_set_colour")

    def get_colour(self):
        out = Colour()
        _check(lib().mibayer_get_colour(self._h, ctypes.byref(out)), "mibayer_get_colour")
        return out

    # -- lens shading correction ------------------------------------------------------------
    def set_shading(self, shading):
        """mibayer_set_shading: the table (a Shading, or None = off) of the host-path frames accepted and the
        shade_device calls made from now on"""
        _check(lib().mibayer_set_shading(self._h, None if shading is None else ctypes.byref(shading)),
               "mibayer_set_shading")

    def get_shading(self):
        """mibayer_get_shading: None when no table is set, else (kx, ky, black, (4, ny, nx) table)"""
        out = Shading()
        rc = lib().mibayer_get_shading(self._h, ctypes.byref(out))
        if rc == ERR_EMPTY:
            return None
        _check(rc, "mibayer_get_shading")
        nx, ny = shading_nodes(self.width, self.height, out.cell_log2_x, out.cell_log2_y)
        table = np.ctypeslib.as_array(ctypes.cast(out.table, ctypes.POINTER(ctypes.c_uint16)), (4, ny, nx)).copy()
        return out.cell_log2_x, out.cell_log2_y, tuple(out.black), table

    def shade_device(self, d_src, d_dst=None, nframes=1, src_frame_bytes=None, dst_frame_bytes=None, stream="ctx"):
        """mibayer_shade_device: nframes mosaics at d_src shaded into d_dst (None: in place) with the table set"""
        s = self.stream if stream == "ctx" else (stream or 0)
        pitch = src_frame_bytes or self.src_bytes
        _check(lib().mibayer_shade_device(self._h, _vp(d_src), pitch, _vp(d_src if d_dst is None else d_dst),
                                          (dst_frame_bytes or pitch), nframes, _vp(s)), "mibayer_shade_device")

    # -- defective pixel correction ---------------------------------------------------------
    def set_dpc(self, dpc):
        """mibayer_set_dpc: the correction (a Dpc, or None = off) of the host-path frames accepted and the dpc_device
        calls made from now on"""
        _check(lib().mibayer_set_dpc(self._h, None if dpc is None else ctypes.byref(dpc)), "mibayer_set_dpc")

    def get_dpc(self):
        """mibayer_get_dpc: None when off, else (hot, cold, (n, 2) uint32 list sorted by (y, x) without duplicates)"""
        out = Dpc()
        rc = lib().mibayer_get_dpc(self._h, ctypes.byref(out))
        if rc == ERR_EMPTY:
            return None
        _check(rc, "mibayer_get_dpc")
        if not out.ndefects:
            return out.hot, out.cold, np.zeros((0, 2), np.uint32)
        arr = np.ctypeslib.as_array(ctypes.cast(out.defects, ctypes.POINTER(ctypes.c_uint32)), (out.ndefects, 2)).copy()
        return out.hot, out.cold, arr

    def dpc_device(self, d_src, d_dst, nframes=1, src_frame_bytes=None, dst_frame_bytes=None, stream="ctx"):
        """mibayer_dpc_device: nframes mosaics at d_src corrected into d_dst (never d_src) with the parameters set"""
        s = self.stream if stream == "ctx" else (stream or 0)
        pitch = src_frame_bytes or self.src_bytes
        _check(lib().mibayer_dpc_device(self._h, _vp(d_src), pitch, _vp(d_dst), (dst_frame_bytes or pitch), nframes,
                                        _vp(s)), "mibayer_dpc_device")

    # -- noise reduction ----------------------------------------------------------------------
    def set_nr(self, nr):
        """mibayer_set_nr: the curve (an Nr, or None = off) of the host-path frames accepted and the nr_device calls
        made from now on"""
        _check(lib().mibayer_set_nr(self._h, None if nr is None else ctypes.byref(nr)), "mibayer_set_nr")

    def get_nr(self):
        """mibayer_get_nr: None when off, else the 17 nodes"""
        out = Nr()
        rc = lib().mibayer_get_nr(self._h, ctypes.byref(out))
        if rc == ERR_EMPTY:
            return None
        _check(rc, "mibayer_get_nr")
        return out.nodes()

    def nr_device(self, d_src, d_dst, nframes=1, src_frame_bytes=None, dst_frame_bytes=None, stream="ctx"):
        """mibayer_nr_device: nframes mosaics at d_src denoised into d_dst (never d_src) with the curve set"""
        s = self.stream if stream == "ctx" else (stream or 0)
        pitch = src_frame_bytes or self.src_bytes
        _check(lib().mibayer_nr_device(self._h, _vp(d_src), pitch, _vp(d_dst), (dst_frame_bytes or pitch), nframes,
                                       _vp(s)), "mibayer_nr_device")

    # -- mosaic zone statistics -------------------------------------------------------------
    def stats_device(self, d_src, d_stats, zones_x, zones_y, lo, hi, nframes=1, src_frame_bytes=None, stream="ctx"):
        """mibayer_stats_device: d_stats receives nframes * zones_y * zones_x StatsZone (64 bytes each)"""
        s = self.stream if stream == "ctx" else (stream or 0)
        _check(lib().mibayer_stats_device(self._h, _vp(d_src), src_frame_bytes or self.src_bytes, nframes, zones_x,
                                          zones_y, lo, hi, _vp(d_stats), _vp(s)), "mibayer_stats_device")

    def set_stats(self, zones_x, zones_y, lo=0, hi=0):
        """mibayer_set_stats: zone statistics for the host-path frames accepted from now on; (0, 0) = off"""
        _check(lib().mibayer_set_stats(self._h, zones_x, zones_y, lo, hi), "mibayer_set_stats")
        if zones_x and zones_y:
            self._zones = (zones_y, zones_x)

    def frame_stats(self):
        """mibayer_frame_stats: (zones_y, zones_x) STATS_DTYPE array of the frame handed back last"""
        out = np.zeros(self._zones, STATS_DTYPE)
        _check(lib().mibayer_frame_stats(self._h, _ptr(out), out.size), "mibayer_frame_stats")
        return out

    def stats_batch_via_device(self, frames, zones_x, zones_y, lo, hi, src_frame_bytes=None):
        """frames: (N, ...) on the host, each src_frame_bytes (default: one frame) long -> (N, zones_y, zones_x)
        STATS_DTYPE through ONE mibayer_stats_device launch; d_stats is pre-filled with junk"""
        frames = np.ascontiguousarray(frames)
        n = frames.shape[0]
        frames = frames.view(np.uint8).reshape(n, -1)
        pitch = src_frame_bytes or self.src_bytes
        assert frames.shape[1] == pitch
        nz = n * zones_x * zones_y
        d_src = self.device_alloc(n * pitch)
        d_stats = self.device_alloc(nz * 64)
        try:
            self.to_device(d_src, frames)
            self.to_device(d_stats, np.full(nz * 64, 0xA5, np.uint8))
            self.stats_device(d_src, d_stats, zones_x, zones_y, lo, hi, n, pitch)
            self.sync()
            out = self.from_device(d_stats, nz * 64)
        finally:
            self.device_free(d_src)
            self.device_free(d_stats)
        return out.view(STATS_DTYPE).reshape(n, zones_y, zones_x)

    # -- mosaic histogram -------------------------------------------------------------------
    def hist_device(self, d_src, d_hist, window=(0, 0, 0, 0), nframes=1, src_frame_bytes=None, stream="ctx"):
        """mibayer_hist_device: d_hist receives nframes Hist (4096 bytes each) of `window` (x0, y0, w, h)"""
        s = self.stream if stream == "ctx" else (stream or 0)
        _check(lib().mibayer_hist_device(self._h, _vp(d_src), src_frame_bytes or self.src_bytes, nframes, *window,
                                         _vp(d_hist), _vp(s)), "mibayer_hist_device")

    def set_hist(self, on, window=(0, 0, 0, 0)):
        """mibayer_set_hist: a histogram of `window` for the host-path frames accepted from now on"""
        _check(lib().mibayer_set_hist(self._h, int(bool(on)), *window), "mibayer_set_hist")

    def frame_hist(self):
        """mibayer_frame_hist: (4, 256) HIST_DTYPE array of the frame handed back last"""
        out = np.zeros(HIST_SHAPE, HIST_DTYPE)
        _check(lib().mibayer_frame_hist(self._h, _ptr(out)), "mibayer_frame_hist")
        return out

    def hist_batch_via_device(self, frames, window=(0, 0, 0, 0), src_frame_bytes=None, src_offset=0):
        """frames: (N, ...) on the host, each src_frame_bytes (default: one frame) long -> (N, 4, 256) HIST_DTYPE
        through ONE mibayer_hist_device launch.  d_hist is pre-filled with junk and followed by a guard that must
        survive; the mosaic starts src_offset bytes into its allocation"""
        frames = np.ascontiguousarray(frames)
        n = frames.shape[0]
        frames = frames.view(np.uint8).reshape(n, -1)
        pitch = src_frame_bytes or self.src_bytes
        assert frames.shape[1] == pitch
        nb = n * ctypes.sizeof(Hist)
        guard = 256
        d_src = self.device_alloc(n * pitch + src_offset)
        d_hist = self.device_alloc(nb + guard)
        try:
            self.to_device(d_src + src_offset, frames)
            self.to_device(d_hist, np.full(nb + guard, 0xA5, np.uint8))
            self.hist_device(d_src + src_offset, d_hist, window, n, pitch)
            self.sync()
            out = self.from_device(d_hist, nb + guard)
        finally:
            self.device_free(d_src)
            self.device_free(d_hist)
        if not (out[nb:] == 0xA5).all():
            raise AssertionError("mibayer_hist_device wrote past the last histogram")
        return out[:nb].view(HIST_DTYPE).reshape((n,) + HIST_SHAPE)

    # -- mosaic focus statistics ------------------------------------------------------------
    def focus_device(self, d_src, d_focus, zones_x, zones_y, thr, nframes=1, src_frame_bytes=None, stream="ctx"):
        """mibayer_focus_device: d_focus receives nframes * zones_y * zones_x FocusZone (96 bytes each)"""
        s = self.stream if stream == "ctx" else (stream or 0)
        _check(lib().mibayer_focus_device(self._h, _vp(d_src), src_frame_bytes or self.src_bytes, nframes, zones_x,
                                          zones_y, thr, _vp(d_focus), _vp(s)), "mibayer_focus_device")

    def set_focus(self, zones_x, zones_y, thr=0):
        """mibayer_set_focus: focus statistics for the host-path frames accepted from now on; (0, 0) = off"""
        _check(lib().mibayer_set_focus(self._h, zones_x, zones_y, thr), "mibayer_set_focus")
        if zones_x and zones_y:
            self._fzones = (zones_y, zones_x)

    def frame_focus(self):
        """mibayer_frame_focus: (zones_y, zones_x) FOCUS_DTYPE array of the frame handed back last"""
        out = np.zeros(self._fzones, FOCUS_DTYPE)
        _check(lib().mibayer_frame_focus(self._h, _ptr(out), out.size), "mibayer_frame_focus")
        return out

    def focus_batch_via_device(self, frames, zones_x, zones_y, thr, src_frame_bytes=None, src_offset=0):
        """frames: (N, ...) on the host, each src_frame_bytes (default: one frame) long -> (N, zones_y, zones_x)
        FOCUS_DTYPE through ONE mibayer_focus_device launch.  The mosaic starts src_offset bytes into its allocation
        and is followed by a guard; d_focus is pre-filled with junk and lies between two guards.  All guards, and the
        mosaic itself, must come back as they went (the kernel is read-only)"""
        frames = np.ascontiguousarray(frames)
        n = frames.shape[0]
        frames = frames.view(np.uint8).reshape(n, -1)
        pitch = src_frame_bytes or self.src_bytes
        assert frames.shape[1] == pitch
        nb = n * zones_x * zones_y * ctypes.sizeof(FocusZone)
        guard = 256
        d_src = self.device_alloc(src_offset + n * pitch + guard)
        d_focus = self.device_alloc(guard + nb + guard)
        try:
            self.to_device(d_src + src_offset, frames)
            self.to_device(d_src + src_offset + n * pitch, np.full(guard, 0x5A, np.uint8))
            self.to_device(d_focus, np.full(guard + nb + guard, 0xA5, np.uint8))
            self.focus_device(d_src + src_offset, d_focus + guard, zones_x, zones_y, thr, n, pitch)
            self.sync()
            back = self.from_device(d_src + src_offset, n * pitch + guard)
            out = self.from_device(d_focus, guard + nb + guard)
        finally:
            self.device_free(d_src)
            self.device_free(d_focus)
        if not (out[:guard] == 0xA5).all() or not (out[guard + nb:] == 0xA5).all():
            raise AssertionError("mibayer_focus_device wrote outside the focus zones")
        if not (back[:n * pitch] == frames.reshape(-1)).all() or not (back[n * pitch:] == 0x5A).all():
            raise AssertionError("mibayer_focus_device changed the mosaic or the bytes behind it")
        return out[guard:guard + nb].copy().view(FOCUS_DTYPE).reshape(n, zones_y, zones_x)

    # -- lifetime ---------------------------------------------------------------------------
    def close(self):
        if getattr(self, "_h", None):
            lib().mibayer_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    # -- host path --------------------------------------------------------------------------
    def process_host(self, src, dst=None):
        """src: uint8 array of src_stride*height bytes -> (height, dst_stride) uint8; planar: (3*height, dst_stride)."""
        src = self._src_bytes(src)
        assert src.size == self.src_bytes, (src.size, self.src_bytes)
        if dst is None:
            dst = np.full((self.dst_rows, self.dst_stride), 0xA5, np.uint8)
        assert dst.size == self.dst_bytes and dst.flags.c_contiguous
        _check(lib().mibayer_process_host(self._h, _ptr(src), _ptr(dst)), "mibayer_process_host")
        return dst

    def _src_bytes(self, src):
        if self.deep and isinstance(src, np.ndarray) and src.dtype != np.uint8:
            return np.ascontiguousarray(src).view(np.uint8).reshape(-1)
        return np.ascontiguousarray(src, dtype=np.uint8)

    def submit(self, src, dst, tag=0):
        _check(lib().mibayer_submit(self._h, _ptr(src), _ptr(dst), _vp(tag)), "mibayer_submit")

    def wait(self):
        tag = _vp()
        _check(lib().mibayer_wait(self._h, ctypes.byref(tag)), "mibayer_wait")
        return tag.value or 0

    def pending(self):
        return lib().mibayer_pending(self._h)

    def set_wait_timeout(self, ms):
        _check(lib().mibayer_set_wait_timeout(self._h, ms), "mibayer_set_wait_timeout")

    def set_wait_spin(self, us):
        _check(lib().mibayer_set_wait_spin(self._h, us), "mibayer_set_wait_spin")

    def host_stats(self):
        st = HostStats()
        _check(lib().mibayer_get_host_stats(self._h, ctypes.byref(st)), "mibayer_get_host_stats")
        return st.as_dict()

    def stall(self, ms):
        """Drill (csrc/mibayer_hooks.h): occupy the context's compute queue for `ms` milliseconds."""
        if not hasattr(lib(), "mibayer_internal_stall"):
            raise MibayerErrorNoLib("the stall drill is exported by the lab build only (make lab; MIBAYER_LIB_PATH)")
        fn = lib().mibayer_internal_stall
        fn.restype, fn.argtypes = ctypes.c_int, [_vp, ctypes.c_int]
        _check(fn(self._h, ms), "mibayer_internal_stall")

    @property
    def host_bands(self):
        """Seam (csrc/mibayer_hooks.h): the bands the next host-path frame submitted alone would be cut into."""
        if not hasattr(lib(), "mibayer_internal_host_bands"):
            raise MibayerErrorNoLib("the band count is exported by the lab build only (make lab; MIBAYER_LIB_PATH)")
        fn = lib().mibayer_internal_host_bands
        fn.restype, fn.argtypes = ctypes.c_int, [_vp]
        nb = fn(self._h)
        _check(min(nb, OK), "mibayer_internal_host_bands")
        return nb

    # -- device path ------------------------------------------------------------------------
    def device_alloc(self, nbytes):
        p = lib().mibayer_device_alloc(self._h, nbytes)
        if not p:
            raise MibayerError(ERR_NOMEM, "mibayer_device_alloc(%d)" % nbytes)
        return p

    def device_free(self, p):
        lib().mibayer_device_free(self._h, _vp(p))

    def to_device(self, d_dst, arr):
        arr = np.ascontiguousarray(arr)
        _check(lib().mibayer_copy_to_device(self._h, _vp(d_dst), _ptr(arr), arr.nbytes),
               "mibayer_copy_to_device")

    def from_device(self, d_src, nbytes):
        out = np.empty(nbytes, np.uint8)
        _check(lib().mibayer_copy_from_device(self._h, _ptr(out), _vp(d_src), nbytes),
               "mibayer_copy_from_device")
        return out

    @property
    def stream(self):
        """The context's own compute stream (hipStream_t as an int)."""
        return lib().mibayer_ctx_stream(self._h)

    def process_device(self, d_src, d_dst, nframes=1, src_frame_bytes=None, dst_frame_bytes=None,
                       stream="ctx"):
        """stream: "ctx" = the context's compute stream, else a hipStream_t value (0/None = null stream)."""
        s = self.stream if stream == "ctx" else (stream or 0)
        _check(lib().mibayer_process_device(
            self._h, _vp(d_src), src_frame_bytes or self.src_bytes, _vp(d_dst),
            dst_frame_bytes or self.dst_bytes, nframes, _vp(s)), "mibayer_process_device")

    def process_device_list(self, d_srcs, d_dsts, stream="ctx"):
        """One launch (per 16 frames) over frames that are separate device allocations."""
        s = self.stream if stream == "ctx" else (stream or 0)
        n = len(d_srcs)
        a, b = (_vp * n)(*d_srcs), (_vp * n)(*d_dsts)
        _check(lib().mibayer_process_device_list(self._h, a, b, n, _vp(s)), "mibayer_process_device_list")

    def sync(self):
        _check(lib().mibayer_sync(self._h), "mibayer_sync")

    def time_device(self, d_src, d_dst, nframes, warmup=2, reps=10, src_frame_bytes=None,
                    dst_frame_bytes=None):
        ms = ctypes.c_float()
        _check(lib().mibayer_time_device(
            self._h, _vp(d_src), src_frame_bytes or self.src_bytes, _vp(d_dst),
            dst_frame_bytes or self.dst_bytes, nframes, warmup, reps, ctypes.byref(ms)),
            "mibayer_time_device")
        return ms.value

    def autotune(self, d_src, d_dst, nframes, src_frame_bytes=None, dst_frame_bytes=None):
        """Measured plan selection (mibayer_autotune); returns the one-line report."""
        buf = ctypes.create_string_buffer(1024)
        _check(lib().mibayer_autotune(
            self._h, _vp(d_src), src_frame_bytes or self.src_bytes, _vp(d_dst),
            dst_frame_bytes or self.dst_bytes, nframes, buf, len(buf)), "mibayer_autotune")
        self.variant_name = lib().mibayer_ctx_variant_name(self._h).decode()
        return buf.value.decode()

    def autotune_list(self, d_srcs, d_dsts):
        """mibayer_autotune_list over separately allocated frames; returns the one-line report."""
        n = len(d_srcs)
        a, b = (_vp * n)(*d_srcs), (_vp * n)(*d_dsts)
        buf = ctypes.create_string_buffer(1024)
        _check(lib().mibayer_autotune_list(self._h, a, b, n, buf, len(buf)), "mibayer_autotune_list")
        self.variant_name = lib().mibayer_ctx_variant_name(self._h).decode()
        return buf.value.decode()

    def get_plan(self):
        """(variant id, band override, store alignment)"""
        v, b, a = ctypes.c_int(), ctypes.c_int(), ctypes.c_int()
        _check(lib().mibayer_get_plan(self._h, ctypes.byref(v), ctypes.byref(b), ctypes.byref(a)), "mibayer_get_plan")
        return v.value, b.value, a.value

    def variant_name_for(self, nframes):
        """The kernel variant launches of `nframes` frames run (`variant_name` describes the batch-class plan
        only; a context that launches frame by frame -- the host path, stream mode -- runs the frame-class plan)."""
        return variant_names()[self.get_plan_for(nframes)[0]]

    def get_plan_for(self, nframes):
        """(variant id, band override, store alignment, source) of the launch class an nframes-frame launch falls into"""
        v, b, a, s = (ctypes.c_int() for _ in range(4))
        _check(lib().mibayer_get_plan_for(self._h, nframes, ctypes.byref(v), ctypes.byref(b), ctypes.byref(a),
                                          ctypes.byref(s)), "mibayer_get_plan_for")
        return v.value, b.value, a.value, s.value

    def set_plan_for(self, nframes, variant, band, align=0):
        _check(lib().mibayer_set_plan_for(self._h, nframes, variant, band, align), "mibayer_set_plan_for")

    def frame_queue(self, k):
        """Frame queue k of the context's device (hipStream_t as an int): FRAME_QUEUES compute streams on hardware
        queues of their own, for independent one-frame launches; created on first use."""
        s = lib().mibayer_ctx_frame_queue(self._h, k)
        if not s:
            raise MibayerError(ERR_HIP, "mibayer_ctx_frame_queue(%d)" % k)
        return s

    @property
    def frame_queues(self):
        return [self.frame_queue(k) for k in range(FRAME_QUEUES)]

    def set_plan(self, variant, band, align=0):
        _check(lib().mibayer_set_plan(self._h, variant, band, align), "mibayer_set_plan")
        self.variant_name = lib().mibayer_ctx_variant_name(self._h).decode()

    def plan_from_cache(self):
        hit = lib().mibayer_plan_from_cache(self._h) == 1
        self.variant_name = lib().mibayer_ctx_variant_name(self._h).decode()
        return hit

    @property
    def plan_source(self):
        return lib().mibayer_plan_source(self._h)

    def copy_plan_from(self, other):
        _check(lib().mibayer_copy_plan(self._h, other._h), "mibayer_copy_plan")
        self.variant_name = lib().mibayer_ctx_variant_name(self._h).decode()

    def fill_synthetic(self, d_src, nframes, seed, first_frame=0, src_frame_bytes=None, stream="ctx"):
        s = self.stream if stream == "ctx" else (stream or 0)
        _check(lib().mibayer_fill_synthetic(
            self._h, _vp(d_src), src_frame_bytes or self.src_bytes, first_frame, nframes, seed,
            _vp(s)), "mibayer_fill_synthetic")

    def launch_geometry(self, nframes=1):
        tw, th, tx, band = (ctypes.c_int() for _ in range(4))
        rows, grid = ctypes.c_int64(), ctypes.c_int64()
        _check(lib().mibayer_launch_geometry(self._h, nframes, ctypes.byref(tw), ctypes.byref(th),
                                             ctypes.byref(tx), ctypes.byref(rows), ctypes.byref(band),
                                             ctypes.byref(grid)), "mibayer_launch_geometry")
        return {"tile_w": tw.value, "tile_h": th.value, "tiles_x": tx.value, "tile_rows": rows.value,
                "band": band.value, "grid_blocks": grid.value}

    # -- convenience for tests ---------------------------------------------------------------
    def process_batch_via_device(self, frames):
        """frames: (N, height, src_stride) uint8 on the host -> (N, height, dst_stride) uint8 (planar: N, 3*height, .),
        through ONE device-resident batch launch (mibayer_process_device)."""
        if self.deep and frames.dtype != np.uint8:
            frames = np.ascontiguousarray(frames).view(np.uint8).reshape(frames.shape[0], -1)
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.shape[0]
        assert frames[0].size == self.src_bytes
        d_src = self.device_alloc(n * self.src_bytes)
        d_dst = self.device_alloc(n * self.dst_bytes)
        try:
            self.to_device(d_src, frames)
            self.process_device(d_src, d_dst, n)
            self.sync()
            out = self.from_device(d_dst, n * self.dst_bytes)
        finally:
            self.device_free(d_src)
            self.device_free(d_dst)
        return out.reshape(n, self.dst_rows, self.dst_stride)

    def planes(self, frame):
        """planes() of a frame this context converted"""
        assert self.planar
        return planes(frame, self.out_width, self.out_height, self.dst_stride)
