"""CPU tests of the defective pixel correction entry points at the boundaries: struct mibayer_dpc and group `dpc` in
include/mibayer.h and the harness, the symbols in both libraries, the argument rules that need no device, the three
bayer2rgb properties, and the refusals over the test double (which has no correction)."""
import ctypes
import os
import re
import subprocess

import numpy as np

import dpc_model as dm
from test_colour_abi import prop_block
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: F401  (fixture)
from test_highbit_abi import inspect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DPC = ["mibayer_set_dpc", "mibayer_get_dpc", "mibayer_dpc_device", "mibayer_pool_set_dpc"]
PROPS = ("dpc-hot-threshold", "dpc-cold-threshold", "defect-file")


def test_symbols_in_both_libraries_and_the_harness(pkg, lab_pkg):
    for p in (pkg, lab_pkg):
        assert all(name in p.ABI and hasattr(p.lib(), name) for name in DPC)
    assert hasattr(pkg, "Dpc") and hasattr(pkg.Pool, "set_dpc")
    for name in ("set_dpc", "get_dpc", "dpc_device"):
        assert hasattr(pkg.Context, name)


def test_header_struct_and_group(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    assert re.search(r"#define MIBAYER_DPC_MAX_DEFECTS 65536\b", text) and pkg.DPC_MAX_DEFECTS == 65536 == dm.MAX_DEFECTS
    m = re.search(r"typedef struct mibayer_dpc \{(.*?)\} mibayer_dpc;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == [
        "uint32_t struct_size", "int32_t hot", "int32_t cold", "uint32_t ndefects", "const uint32_t *defects"]
    assert [name for name, _ in pkg.Dpc._fields_] == ["struct_size", "hot", "cold", "ndefects", "defects"]
    assert ctypes.sizeof(pkg.Dpc) == 24 and pkg.Dpc.defects.offset == 16
    block = text[text.index("* group dpc:"):text.index("* group shading:")]
    assert sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block))) == sorted(DPC)
    assert "5, later additive: defective pixel correction" in text
    # the open item the definition leaves: listed neighbours see each other
    assert "see each other" in text
    d = pkg.Dpc(3, -1, [(5, 7), (1, 2)])
    assert (d.struct_size, d.hot, d.cold, d.ndefects) == (24, 3, -1, 2) and d.defects
    assert pkg.Dpc().ndefects == 0 and not pkg.Dpc().defects and (pkg.Dpc().hot, pkg.Dpc().cold) == (-1, -1)


def test_the_readme_counts_the_exports(pkg):
    text = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"\b%d (exported )?(functions|entry points|symbols)" % len(pkg.ABI), text), len(pkg.ABI)


def test_null_handles_and_contexts_without_a_device(pkg):
    L = pkg.lib()
    d = pkg.Dpc(4, 4, [(1, 1)])
    assert L.mibayer_set_dpc(None, d) == pkg.ERR_ARG and L.mibayer_set_dpc(None, None) == pkg.ERR_ARG
    assert L.mibayer_get_dpc(None, d) == pkg.ERR_ARG
    assert L.mibayer_pool_set_dpc(None, d) == pkg.ERR_ARG and L.mibayer_pool_set_dpc(None, None) == pkg.ERR_ARG
    assert L.mibayer_dpc_device(None, 16, 0, 32, 0, 1, None) == pkg.ERR_ARG
    # the rules of a context: what the header says, or no device
    try:
        ctx = pkg.Context(64, 48)
    except pkg.MibayerError as e:
        assert e.status == pkg.ERR_NO_DEVICE
        return
    with ctx:
        short = pkg.Dpc(4, 4)
        short.struct_size -= 4
        for bad in (pkg.Dpc(256, 4), pkg.Dpc(4, -2), pkg.Dpc(4, 4, [(64, 0)]), pkg.Dpc(4, 4, [(0, 48)]), short):
            assert L.mibayer_set_dpc(ctx._h, bad) == pkg.ERR_ARG
        assert L.mibayer_get_dpc(ctx._h, None) == pkg.ERR_ARG and ctx.get_dpc() is None
        ctx.set_dpc(d)
        assert ctx.get_dpc()[2].tolist() == [[1, 1]]
        ctx.set_dpc(None)


@needs_gst
def test_inspect_lists_the_properties_on_bayer2rgb_only(plugin, tmp_path):  # noqa: F811
    out = inspect(tmp_path, "bayer2rgb")
    for name in PROPS[:2]:
        block = prop_block(out, name)
        assert block is not None and "Integer. Range: -1 - 65535 Default: -1" in " ".join(block.split()), block
        assert "changeable only in NULL or READY state" in block
    block = prop_block(out, PROPS[2])
    assert block is not None and "String. Default: \"\"" in " ".join(block.split()), block
    for element in ("rgb2bayer", "hipbayer2rgb"):
        for name in PROPS:
            assert prop_block(inspect(tmp_path, element), name) is None, (element, name)


@needs_gst
def test_mock_rig_converts_with_the_defaults_and_fails_cleanly_otherwise(rig, tmp_path):  # noqa: F811
    """The mock library has no defective pixel correction.  With the defaults -- spelled out or not -- the element calls
    none of its entry points and converts as before; a threshold, a list, a list that cannot be read, is not `x y` or
    names a pixel outside the frame each end in an element error, not in a crash."""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=7).tofile(inp)
    off = 'dpc-hot-threshold=-1 dpc-cold-threshold=-1 defect-file=""'
    for launch in ("bayer2rgb", "bayer2rgb " + off, "bayer2rgb inflight=3 devices=0,0 " + off):
        kv = run(rig, "convert", launch, B2R % ("gbrg", w, h), inp, 260 * h, outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n) and kv["errors"] == "0", (launch, kv)
        seq, fill = stamps(outp, n, 4 * w * h)
        assert fill == list(range(7, 7 + n)) and seq == list(range(n)), launch
    good, outside, junk = tmp_path / "good.txt", tmp_path / "outside.txt", tmp_path / "junk.txt"
    good.write_text("# two defects\n\n3 4\n257 36 # the last pixel\n")
    outside.write_text("3 4\n258 0\n")
    junk.write_text("3 4\nx y\n")
    for launch in ("bayer2rgb dpc-hot-threshold=40", "bayer2rgb dpc-cold-threshold=0", "bayer2rgb defect-file=%s" % good,
                   "bayer2rgb inflight=3 devices=0,0 dpc-hot-threshold=40 defect-file=%s" % good,
                   "bayer2rgb defect-file=%s" % outside, "bayer2rgb defect-file=%s" % junk,
                   "bayer2rgb defect-file=%s" % (tmp_path / "missing.txt")):
        kv = run(rig, "caps", launch, B2R % ("gbrg", w, h), 260 * h)
        assert int(kv["errors"]) >= 1 and kv["caps_accepted"] == "0", (launch, kv)


def test_the_pool_refuses_over_the_test_double(tmp_path):
    """the pool binds mibayer_set_dpc weakly: over contexts without it mibayer_pool_set_dpc is refused, NULL included,
    and the pool converts as before"""
    csrc = os.path.join(ROOT, "gst-plugins-bad_amd", "csrc")
    check = os.path.join(ROOT, "tests", "check")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    obj, exe = str(tmp_path / "mock.o"), str(tmp_path / "pool_dpc")
    res = subprocess.run(["gcc", "-O1", "-Wall"] + inc + ["-c", os.path.join(check, "mock_mibayer.c"), "-o", obj],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall"] + inc
                         + [os.path.join(check, "pool_dpc.cpp"), os.path.join(csrc, "mibayer_pool.cpp"), obj, "-o", exe,
                            "-lpthread"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.split() == ["set=-1", "off=-1", "delivered=5"], (res.returncode, res.stdout, res.stderr[-500:])
