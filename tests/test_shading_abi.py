"""CPU tests of the lens shading entry points at the boundaries: struct mibayer_shading and group `shading` in
include/mibayer.h and the harness, the two pure host helpers against the NumPy model (tests/shading_model.py) bit for
bit, the argument rules, and the bayer2rgb property over the test double."""
import ctypes
import os
import re

import numpy as np
import pytest

import shading_model as shm
import stats_model as sm
from test_colour_abi import prop_block
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: F401  (fixture)
from test_highbit_abi import inspect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHADING = ["mibayer_shading_nodes", "mibayer_set_shading", "mibayer_get_shading", "mibayer_shade_device",
           "mibayer_pool_set_shading", "mibayer_stats_shading"]


def test_header_struct_and_group(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    assert re.search(r"#define MIBAYER_SHADING_MAX_NODES 129\b", text) and pkg.SHADING_MAX_NODES == 129 == shm.MAX_NODES
    m = re.search(r"typedef struct mibayer_shading \{(.*?)\} mibayer_shading;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == [
        "uint32_t struct_size", "int32_t cell_log2_x", "int32_t cell_log2_y", "uint32_t black[4]", "const uint16_t *table"]
    assert [name for name, _ in pkg.Shading._fields_] == ["struct_size", "cell_log2_x", "cell_log2_y", "black", "table"]
    assert ctypes.sizeof(pkg.Shading) == 40 and pkg.Shading.table.offset == 32
    block = text[text.index("* group shading:"):text.index("* group hist:")]
    assert sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block))) == sorted(SHADING)
    assert "5, later additive: lens shading correction" in text


def test_symbols_in_both_libraries_and_the_harness(pkg, lab_pkg):
    for p in (pkg, lab_pkg):
        assert all(name in p.ABI and hasattr(p.lib(), name) for name in SHADING)
    for name in ("Shading", "shading_nodes", "stats_shading"):
        assert hasattr(pkg, name)
    for name in ("set_shading", "get_shading", "shade_device"):
        assert hasattr(pkg.Context, name)
    assert hasattr(pkg.Pool, "set_shading")


# (W, H, kx, ky): W - 1 and H - 1 exactly on a cell boundary, kx != ky, the smallest and the largest cells and frames
NODE_SIZES = [(4, 3, 2, 2), (5, 5, 2, 2), (8, 8, 2, 2), (9, 9, 3, 3), (257, 129, 8, 7), (256, 128, 8, 7), (258, 37, 5, 3),
              (512, 508, 2, 2), (509, 512, 2, 2), (3840, 2160, 5, 5), (32768, 32768, 8, 8), (32769, 4, 8, 2)]


def test_shading_nodes_matches_the_model(pkg):
    L = pkg.lib()
    nx, ny = ctypes.c_int(-7), ctypes.c_int(-7)
    for (w, h, kx, ky) in NODE_SIZES:
        try:
            want = shm.nodes(w, h, kx, ky)
        except ValueError:
            assert L.mibayer_shading_nodes(w, h, kx, ky, ctypes.byref(nx), ctypes.byref(ny)) == pkg.ERR_ARG, (w, h, kx, ky)
            continue
        assert pkg.shading_nodes(w, h, kx, ky) == want, (w, h, kx, ky)
    assert pkg.shading_nodes(512, 508, 2, 2) == (129, 128) and pkg.shading_nodes(5, 5, 2, 2) == (3, 3)
    for bad in ((513, 4, 2, 2), (4, 513, 2, 2), (4, 4, 1, 2), (4, 4, 2, 1), (4, 4, 9, 2), (4, 4, 2, 9), (0, 4, 2, 2),
                (4, 0, 2, 2), (-4, 4, 2, 2)):
        assert L.mibayer_shading_nodes(*bad, ctypes.byref(nx), ctypes.byref(ny)) == pkg.ERR_ARG, bad
    assert (nx.value, ny.value) == (-7, -7)             # a refused call writes nothing
    assert L.mibayer_shading_nodes(64, 48, 4, 4, None, ctypes.byref(ny)) == pkg.ERR_ARG
    assert L.mibayer_shading_nodes(64, 48, 4, 4, ctypes.byref(nx), None) == pkg.ERR_ARG


def vignetted(w, h, depth, rng):
    """a noisy flat field with fall-off towards a corner-ish point, per-site levels"""
    vmax = (1 << depth) - 1
    y, x = np.mgrid[0:h, 0:w]
    r2 = ((x - 0.4 * w) ** 2 + (y - 0.55 * h) ** 2) / float(w * w + h * h)
    lv = np.array([0.8, 0.7, 0.65, 0.5])[2 * (y & 1) + (x & 1)] * vmax
    return np.clip(np.rint(vmax // 32 + lv / (1.0 + 3.0 * r2) ** 2 + rng.normal(0, vmax / 200.0, (h, w))), 0, vmax).astype(np.int64)


# (W, H, zones_x, zones_y, kx, ky, depth): 1 x 1 and 64 x 64 zones, empty trailing zones (66 / 64 -> cells of 4: 17 used),
# W - 1 on a cell boundary, kx != ky, an odd height
STATS_CASES = [(64, 48, 1, 1, 4, 4, 8), (256, 128, 64, 64, 4, 3, 12), (66, 70, 32, 35, 2, 3, 10), (258, 37, 12, 7, 5, 3, 8),
               (130, 66, 64, 33, 3, 2, 16), (257 - 1, 129, 9, 5, 8, 7, 14), (20, 12, 10, 6, 2, 2, 8), (640, 480, 40, 30, 5, 5, 12)]


@pytest.mark.parametrize("case", STATS_CASES, ids=lambda c: "%dx%d_z%dx%d_k%d%d_%d" % c)
def test_stats_shading_matches_the_model_bit_for_bit(pkg, case):
    w, h, zx, zy, kx, ky, depth = case
    rng = np.random.default_rng(list(case))
    S = vignetted(w, h, depth, rng)
    vmax = (1 << depth) - 1
    zones = sm.zone_stats(S, zx, zy, vmax // 64, vmax)          # lo above zero: some zones lose samples
    for black, max_gain in (((vmax // 32,) * 4, 7.99), (None, 1.5), ((0, 3, 1, 2), 4.0)):
        ok, table = pkg.stats_shading(zones, w, h, black, kx, ky, max_gain)
        want_ok, want = shm.stats_shading(zones, w, h, black, kx, ky, max_gain)
        assert ok == want_ok == 1 and table.dtype == want.dtype and table.shape == want.shape
        assert np.array_equal(table, want), (black, max_gain, np.argwhere(table != want)[:5])
        assert table.min() >= 4096 and table.max() <= int(max_gain * 4096 + 0.5)
    assert len(np.unique(table)) > 1 or zx * zy == 1       # one zone: one mean, unity


def test_stats_shading_empty_zones_and_refusals(pkg):
    w, h, zx, zy = 66, 70, 32, 35
    rng = np.random.default_rng(66)
    S = vignetted(w, h, 8, rng)
    zones = sm.zone_stats(S, zx, zy, 0, 255)
    assert (zones["count"][:, 17:] == 0).all() and zones["count"][:, :17].all()         # cells of 4 pixels: 17 columns
    # holes: zones emptied by hand take their nearest neighbour, the first in row-major order among equals
    z = zones.copy()
    z["count"][3:6, 4:9] = 0
    z["count"][0, 0] = 0
    z["count"][17, 16, 2] = 0
    ok, table = pkg.stats_shading(z, w, h, (2, 2, 2, 2), 2, 3, 6.0)
    want_ok, want = shm.stats_shading(z, w, h, (2, 2, 2, 2), 2, 3, 6.0)
    assert ok == want_ok == 1 and np.array_equal(table, want)
    # a site without samples, a site at or under its black level: 0 and unity
    z = zones.copy()
    z["count"][..., 1] = 0
    assert pkg.stats_shading(z, w, h, None, 2, 3, 6.0)[0] == 0 == shm.stats_shading(z, w, h, None, 2, 3, 6.0)[0]
    ok, table = pkg.stats_shading(zones, w, h, (0, 0, 255, 0), 2, 3, 6.0)
    assert ok == 0 and (table == 4096).all() and shm.stats_shading(zones, w, h, (0, 0, 255, 0), 2, 3, 6.0)[0] == 0


def test_stats_shading_argument_rules(pkg):
    L = pkg.lib()
    zones = np.zeros((2, 2), sm.STATS_DTYPE)
    zones["count"], zones["sum"] = 10, 1000
    out = np.zeros((4, 4, 5), np.uint16)                # 64 x 48 under cells of 16
    call = lambda z, zx, zy, w, h, kx, ky, mg, o: L.mibayer_stats_shading(z, zx, zy, w, h, None, kx, ky, mg, o)  # noqa: E731
    zp, op = zones.ctypes.data, out.ctypes.data
    assert call(zp, 2, 2, 64, 48, 4, 4, 4.0, op) == 1 and (out == 4096).all()
    for bad in ((None, 2, 2, 64, 48, 4, 4, 4.0, op), (zp, 2, 2, 64, 48, 4, 4, 4.0, None), (zp, 0, 2, 64, 48, 4, 4, 4.0, op),
                (zp, 2, 65, 64, 48, 4, 4, 4.0, op), (zp, 33, 2, 64, 48, 4, 4, 4.0, op), (zp, 2, 25, 64, 48, 4, 4, 4.0, op),
                (zp, 2, 2, 63, 48, 4, 4, 4.0, op), (zp, 2, 2, 0, 48, 4, 4, 4.0, op), (zp, 2, 2, 64, 48, 1, 4, 4.0, op),
                (zp, 2, 2, 64, 48, 4, 9, 4.0, op), (zp, 2, 2, 1024, 48, 2, 4, 4.0, op), (zp, 2, 2, 64, 48, 4, 4, 0.99, op),
                (zp, 2, 2, 64, 48, 4, 4, 8.0, op), (zp, 2, 2, 64, 48, 4, 4, float("nan"), op)):
        assert call(*bad) == pkg.ERR_ARG, bad
    assert call(zp, 2, 2, 64, 48, 4, 4, 1.0, op) == 1 and call(zp, 2, 2, 64, 48, 4, 4, 7.99, op) == 1


def test_null_handles_and_contexts_without_a_device(pkg):
    L = pkg.lib()
    nx, ny = pkg.shading_nodes(64, 48, 4, 4)
    table = np.full((4, ny, nx), 4096, np.uint16)
    sh = pkg.Shading(4, 4, table)
    assert L.mibayer_set_shading(None, sh) == pkg.ERR_ARG and L.mibayer_set_shading(None, None) == pkg.ERR_ARG
    assert L.mibayer_get_shading(None, sh) == pkg.ERR_ARG
    assert L.mibayer_pool_set_shading(None, sh) == pkg.ERR_ARG
    assert L.mibayer_shade_device(None, 16, 0, 16, 0, 1, None) == pkg.ERR_ARG
    # the rules of a context: what the header says, or no device
    try:
        ctx = pkg.Context(64, 48)
    except pkg.MibayerError as e:
        assert e.status == pkg.ERR_NO_DEVICE
        return
    with ctx:
        bad = table.copy()
        bad[0, 0, 0] = 32768
        for s in (pkg.Shading(4, 4, bad), pkg.Shading(4, 4, table, (256, 0, 0, 0)), pkg.Shading(1, 4, table),
                  pkg.Shading(4, 4, None)):
            assert L.mibayer_set_shading(ctx._h, s) == pkg.ERR_ARG
        assert L.mibayer_get_shading(ctx._h, None) == pkg.ERR_ARG
        ctx.set_shading(sh)
        ctx.set_shading(None)


def test_the_calibration_tool_and_the_model_write_the_same_file(tmp_path):
    """the MISH layout has two writers (tools/shading_calibrate.py, tests/shading_model.py) and one reader (the element)"""
    import importlib.util
    spec = importlib.util.spec_from_file_location("shading_calibrate", os.path.join(ROOT, "tools", "shading_calibrate.py"))
    tool = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(tool)
    table = np.random.default_rng(3).integers(0, 32768, (4, 7, 10)).astype(np.uint16)
    a, b = str(tmp_path / "tool.mish"), str(tmp_path / "model.mish")
    tool.write_mish(a, 5, 3, table, (1, 2, 3, 4))
    shm.write_file(b, 5, 3, table, (1, 2, 3, 4))
    data = open(a, "rb").read()
    assert data == open(b, "rb").read() and len(data) == 40 + 2 * table.size
    assert data[:4] == b"MISH" and np.frombuffer(data[4:40], "<u4").tolist() == [1, 5, 3, 10, 7, 1, 2, 3, 4]
    assert np.array_equal(np.frombuffer(data[40:], "<u2").reshape(4, 7, 10), table)


@needs_gst
def test_inspect_lists_shading_file_on_bayer2rgb_only(plugin, tmp_path):  # noqa: F811
    block = prop_block(inspect(tmp_path, "bayer2rgb"), "shading-file")
    assert block is not None and "String. Default: \"\"" in " ".join(block.split()), block
    assert "changeable only in NULL or READY state" in block
    for element in ("rgb2bayer", "hipbayer2rgb"):
        assert prop_block(inspect(tmp_path, element), "shading-file") is None, element


@needs_gst
def test_mock_rig_converts_with_the_default_and_fails_cleanly_with_a_file(rig, tmp_path):  # noqa: F811
    """The mock library has no shading entry points.  With the default -- spelled out or not -- the element calls none
    of them and converts as before; a file ends in an element error, not in a crash."""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=7).tofile(inp)
    for launch in ("bayer2rgb", 'bayer2rgb shading-file=""', 'bayer2rgb inflight=3 devices=0,0 shading-file=""'):
        kv = run(rig, "convert", launch, B2R % ("gbrg", w, h), inp, 260 * h, outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n) and kv["errors"] == "0", (launch, kv)
        seq, fill = stamps(outp, n, 4 * w * h)
        assert fill == list(range(7, 7 + n)) and seq == list(range(n)), launch
    path = tmp_path / "lens.mish"
    nx, ny = shm.nodes(w, h, 5, 3)
    shm.write_file(str(path), 5, 3, np.full((4, ny, nx), 4096, np.uint16), (0, 0, 0, 0))
    for launch in ("bayer2rgb shading-file=%s" % path, "bayer2rgb inflight=3 devices=0,0 shading-file=%s" % path):
        kv = run(rig, "caps", launch, B2R % ("gbrg", w, h), 260 * h)
        assert int(kv["errors"]) >= 1 and kv["caps_accepted"] == "0", (launch, kv)
