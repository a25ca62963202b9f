#!/usr/bin/env python3
"""Generates tests/golden/reference_pins.json: the md5 of what the reference's own compiled functions return for every
input of the tests that pin the oracle and the HIP path against them, so that those tests also run where oracle/_ref
was not built.

Run where oracle/_ref was built (`make -C oracle`, which needs the reference tree):
    python tests/golden/make_reference_pins.py

The inputs are drawn by the tests' own case generators (tests/test_oracle.py, tests/test_gpu_parity.py,
tests/test_gpu_rgb2bayer.py); per case the file holds md5(input) and md5(output of the reference):
  frame_driver             gst_bayer2rgb_process (oracle/_ref/libbayer_frame_ref.so), whole destination rows
  known_md5                the same, on the known-answer frames of known_md5.json up to 4K
  rgb2bayer_transform      gst_rgb2bayer_transform, whole destination rows
  ref_rows                 the restated frame driver over the reference's row kernels (oracle/_ref/libbayerorc_ref.so)
  hip_frame_driver         gst_bayer2rgb_process on the GPU test's frames
  hip_rgb2bayer_transform  gst_rgb2bayer_transform on the GPU test's frames, the W valid columns of each row
"""
import hashlib
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
sys.path.insert(0, ROOT)
sys.path.insert(0, TESTS)
import __graft_entry__ as entry  # noqa: E402
import test_gpu_parity  # noqa: E402
import test_gpu_rgb2bayer  # noqa: E402
import test_oracle  # noqa: E402


def md5(a):
    return hashlib.md5(np.ascontiguousarray(a).tobytes()).hexdigest()


def main():
    oracle = entry.load_oracle()
    oracle.lib()
    if not oracle.have_ref_rows() or not oracle.have_ref_frame():
        sys.exit("oracle/_ref/*.so missing: run `make -C oracle` where the reference tree exists")
    formats = entry.load_package().FORMATS
    cases = {}

    pins = cases["frame_driver"] = {}
    for c in test_oracle.frame_driver_cases(oracle):
        r, g, b = c["rgb"]
        out = oracle.ref_frame_bayer2rgb(c["src"], c["w"], c["pat"], r, g, b, dst_stride=c["dst_stride"])
        pins[c["key"]] = {"in": md5(c["src"]), "out": md5(out)}

    pins = cases["known_md5"] = {}
    with open(os.path.join(HERE, "known_md5.json")) as f:
        for e in json.load(f)["entries"]:
            if e["width"] > 3840:
                continue
            src = oracle.fill_synthetic(e["width"], e["height"], 1, e["seed"])[0]
            r, g, b = oracle.LAYOUTS[e["format"]]
            out = oracle.ref_frame_bayer2rgb(src, e["width"], e["pattern"], r, g, b)
            key = "%dx%d/%d/%s/%s" % (e["width"], e["height"], e["seed"], e["pattern"], e["format"])
            pins[key] = {"in": md5(src), "out": md5(out)}
            if pins[key] != {"in": e["md5_input"], "out": e["md5_output"]}:
                sys.exit("known answer %s does not reproduce through the reference's frame driver" % key)

    pins = cases["rgb2bayer_transform"] = {}
    for c in test_oracle.rgb2bayer_transform_cases():
        pins[c["key"]] = {"in": md5(c["src"]), "out": md5(oracle.ref_frame_rgb2bayer(c["src"], c["w"], c["pat"]))}

    pins = cases["ref_rows"] = {}
    for c in test_oracle.ref_rows_cases(oracle):
        r, g, b = c["rgb"]
        out = oracle.bayer2rgb(c["src"], c["w"], c["pat"], r, g, b, ref_rows=True)
        pins[c["key"]] = {"in": md5(c["src"]), "out": md5(out)}

    pins = cases["hip_frame_driver"] = {}
    for c in test_gpu_parity.hip_frame_driver_cases():
        r, g, b = formats[c["fmt"]]
        out = oracle.ref_frame_bayer2rgb(c["src"], c["w"], c["pat"], r, g, b)
        pins[c["key"]] = {"in": md5(c["src"]), "out": md5(out)}

    pins = cases["hip_rgb2bayer_transform"] = {}
    for c in test_gpu_rgb2bayer.hip_rgb2bayer_transform_cases():
        out = oracle.ref_frame_rgb2bayer(c["src"], c["w"], c["pat"])[:, :c["w"]]
        pins[c["key"]] = {"in": md5(c["src"]), "out": md5(out)}

    with open(os.path.join(HERE, "reference_pins.json"), "w") as f:
        json.dump({"source": "md5 of the outputs of the reference's own gst_bayer2rgb_process, gst_rgb2bayer_transform "
                             "and row kernels (oracle/_ref) on the inputs of the tests that pin against them; "
                             "tests/golden/make_reference_pins.py",
                   "cases": cases}, f, indent=0, sort_keys=True)
        f.write("\n")
    print("wrote %s" % ", ".join("%s: %d" % (k, len(v)) for k, v in cases.items()))


if __name__ == "__main__":
    main()
