"""CPU tests of the noise reduction entry points at the boundaries: struct mibayer_nr and group `nr` in
include/mibayer.h and the harness, the symbols in both libraries, the argument rules that need no device,
mibayer_nr_curve against the model, the three bayer2rgb properties, and the refusal over the test double (which has no
noise reduction)."""
import ctypes
import os
import re
import subprocess

import numpy as np

import nr_model as nm
from test_colour_abi import prop_block
from test_gst_element import needs_gst, plugin  # noqa: F401  (fixture)
from test_gst_element_logic import B2R, frames, rig, run, stamps  # noqa: F401  (fixture)
from test_highbit_abi import inspect

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NR = ["mibayer_set_nr", "mibayer_get_nr", "mibayer_nr_device", "mibayer_pool_set_nr", "mibayer_nr_curve"]
PROPS = {"denoise": "Double. Range: 0 - 1000 Default: 0", "noise-read": "Double. Range: 0 - 65535 Default: 2",
         "noise-shot": "Double. Range: 0 - 65535 Default: 0"}


def test_symbols_in_both_libraries_and_the_harness(pkg, lab_pkg):
    for p in (pkg, lab_pkg):
        assert all(name in p.ABI and hasattr(p.lib(), name) for name in NR)
    assert hasattr(pkg, "Nr") and hasattr(pkg, "nr_curve") and hasattr(pkg.Pool, "set_nr")
    for name in ("set_nr", "get_nr", "nr_device"):
        assert hasattr(pkg.Context, name)


def test_header_struct_and_group(pkg):
    text = open(os.path.join(ROOT, "include", "mibayer.h")).read()
    assert re.search(r"#define MIBAYER_ABI_VERSION 5\b", text)
    assert re.search(r"#define MIBAYER_NR_NODES 17\b", text) and pkg.NR_NODES == 17 == nm.NODES
    m = re.search(r"typedef struct mibayer_nr \{(.*?)\} mibayer_nr;", text, re.S)
    body = re.sub(r"/\*.*?\*/", "", m.group(1), flags=re.S)
    assert [" ".join(f.split()) for f in body.split(";") if f.strip()] == [
        "uint32_t struct_size", "uint16_t curve[17]", "uint16_t reserved"]
    assert [name for name, _ in pkg.Nr._fields_] == ["struct_size", "curve", "reserved"]
    assert ctypes.sizeof(pkg.Nr) == 40 and pkg.Nr.curve.offset == 4 and pkg.Nr.reserved.offset == 38
    # the group sits in front of `dpc`, whose own test slices the header from there
    block = text[text.index("* group nr:"):text.index("* group dpc:")]
    assert sorted(set(re.findall(r"\b(mibayer_[a-z0-9_]+)\b", block))) == sorted(NR)
    assert "5, later additive: noise reduction" in text
    n = pkg.Nr(range(17))
    assert n.struct_size == 40 and n.nodes() == list(range(17)) and pkg.Nr(9).nodes() == [9] * 17 and pkg.Nr().nodes() == [0] * 17


def test_the_readme_counts_the_exports(pkg):
    text = open(os.path.join(ROOT, "README.md")).read()
    assert re.search(r"\b%d (exported )?(functions|entry points|symbols)" % len(pkg.ABI), text), len(pkg.ABI)


def test_null_handles_and_contexts_without_a_device(pkg):
    L = pkg.lib()
    n = pkg.Nr(8)
    assert L.mibayer_set_nr(None, n) == pkg.ERR_ARG and L.mibayer_set_nr(None, None) == pkg.ERR_ARG
    assert L.mibayer_get_nr(None, n) == pkg.ERR_ARG
    assert L.mibayer_pool_set_nr(None, n) == pkg.ERR_ARG and L.mibayer_pool_set_nr(None, None) == pkg.ERR_ARG
    assert L.mibayer_nr_device(None, 16, 0, 32, 0, 1, None) == pkg.ERR_ARG
    # the rules of a context: what the header says, or no device
    try:
        ctx = pkg.Context(64, 48)
    except pkg.MibayerError as e:
        assert e.status == pkg.ERR_NO_DEVICE
        return
    with ctx:
        short, high = pkg.Nr(8), pkg.Nr(8)
        short.struct_size -= 4
        high.curve[0] = 256
        for bad in (short, high):
            assert L.mibayer_set_nr(ctx._h, bad) == pkg.ERR_ARG
        assert L.mibayer_get_nr(ctx._h, None) == pkg.ERR_ARG and ctx.get_nr() is None
        ctx.set_nr(n)
        assert ctx.get_nr() == [8] * 17
        ctx.set_nr(None)


def test_nr_curve_is_the_models(pkg):
    rng = np.random.default_rng(17)
    L = pkg.lib()
    for bits in (8, 10, 12, 14, 16):
        vmax = (1 << bits) - 1
        args = [(0, 2, 0, 1), (0, 0, 0, 0), (vmax / 16, 2.5, 0.37, 1.5), (0, 1e6, 0, 1), (0, 0, 1e9, 1e9), (vmax, 1, 1, 3)]
        args += [(rng.uniform(0, vmax / 4), rng.uniform(0, vmax / 64), rng.uniform(0, 4), rng.uniform(0, 4)) for _ in range(200)]
        for a in args:
            assert pkg.nr_curve(bits, *a).nodes() == nm.noise_curve(bits, *a), (bits, a)
        assert max(pkg.nr_curve(bits, 0, 1e6, 0, 1).nodes()) == nm.t_max(bits)
    out = pkg.Nr(7)
    for bad in ((-1.0, 2, 0, 1), (0, -2.0, 0, 1), (0, 2, -0.1, 1), (0, 2, 0, -1.0), (float("nan"), 2, 0, 1),
                (0, float("inf"), 0, 1), (0, 2, float("nan"), 1), (0, 2, 0, float("inf"))):
        assert L.mibayer_nr_curve(8, *[float(v) for v in bad], ctypes.byref(out)) == pkg.ERR_ARG, bad
    for bits in (0, 7, 9, 11, 17, -8):
        assert L.mibayer_nr_curve(bits, 0.0, 2.0, 0.0, 1.0, ctypes.byref(out)) == pkg.ERR_ARG
    assert L.mibayer_nr_curve(8, 0.0, 2.0, 0.0, 1.0, None) == pkg.ERR_ARG
    assert out.nodes() == [7] * 17      # a refused call writes nothing


@needs_gst
def test_inspect_lists_the_properties_on_bayer2rgb_only(plugin, tmp_path):  # noqa: F811
    out = inspect(tmp_path, "bayer2rgb")
    for name, line in PROPS.items():
        block = prop_block(out, name)
        assert block is not None and line in " ".join(block.split()), block
        assert "changeable only in NULL or READY state" in block
    for element in ("rgb2bayer", "hipbayer2rgb"):
        for name in PROPS:
            assert prop_block(inspect(tmp_path, element), name) is None, (element, name)


@needs_gst
def test_mock_rig_converts_with_the_defaults_and_fails_cleanly_otherwise(rig, tmp_path):  # noqa: F811
    """The mock library has no noise reduction.  With the default -- spelled out or not -- the element calls none of
    its entry points and converts as before; a strength above 0 ends in an element error, not in a crash."""
    w, h, n = 258, 37, 5
    inp, outp = tmp_path / "in.raw", tmp_path / "out.raw"
    frames(n, 260 * h, first=7).tofile(inp)
    off = "denoise=0 noise-read=5 noise-shot=0.5"
    for launch in ("bayer2rgb", "bayer2rgb " + off, "bayer2rgb inflight=3 devices=0,0 " + off):
        kv = run(rig, "convert", launch, B2R % ("gbrg", w, h), inp, 260 * h, outp)
        assert kv["pushed"] == str(n) and kv["pulled"] == str(n) and kv["errors"] == "0", (launch, kv)
        seq, fill = stamps(outp, n, 4 * w * h)
        assert fill == list(range(7, 7 + n)) and seq == list(range(n)), launch
    for launch in ("bayer2rgb denoise=1.5", "bayer2rgb inflight=3 devices=0,0 denoise=0.5 noise-read=3"):
        kv = run(rig, "caps", launch, B2R % ("gbrg", w, h), 260 * h)
        assert int(kv["errors"]) >= 1 and kv["caps_accepted"] == "0", (launch, kv)


def test_the_pool_refuses_over_the_test_double(tmp_path):
    """the pool binds mibayer_set_nr weakly: over contexts without it mibayer_pool_set_nr is refused, NULL included,
    and the pool converts as before"""
    csrc = os.path.join(ROOT, "gst-plugins-bad_amd", "csrc")
    check = os.path.join(ROOT, "tests", "check")
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + csrc]
    obj, exe = str(tmp_path / "mock.o"), str(tmp_path / "pool_nr")
    res = subprocess.run(["gcc", "-O1", "-Wall"] + inc + ["-c", os.path.join(check, "mock_mibayer.c"), "-o", obj],
                         capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run(["g++", "-std=c++17", "-O1", "-Wall"] + inc
                         + [os.path.join(check, "pool_nr.cpp"), os.path.join(csrc, "mibayer_pool.cpp"), obj, "-o", exe,
                            "-lpthread"], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr[-2000:]
    res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
    assert res.returncode == 0 and res.stdout.split() == ["set=-1", "off=-1", "delivered=5"], (res.returncode, res.stdout, res.stderr[-500:])
