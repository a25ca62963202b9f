#!/usr/bin/env python3
"""ISA / resource summary of the production kernels, so the claims of DESIGN.md (v_lerp_u8, v_perm_b32, DPP wave shifts,
16-byte global loads, nt stores, register and LDS budgets, no scratch, no MFMA) are checkable without a toolchain.
Runs `make -C gst-plugins-bad_amd asm` (hipcc -save-temps + -Rpass-analysis=kernel-resource-usage, cross-compiles
without a GPU) and writes profiles/<tag>_isa_summary.md.     Usage: python tools/isa_summary.py r02 [file name]"""
import collections
import os
import re
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "gst-plugins-bad_amd")
tag = sys.argv[1] if len(sys.argv) > 1 else "r02"

# the 24 tile kernels the product build launches: 3 shapes x stores {nt, plain} x {fast, generic, aligned128}, and the
# hybrid store policy x {fast, generic} (LDS_VARIANT_AL / LDS_VARIANT of ids 1-9 in csrc/mibayer_kernels.hip)
TILE_SHAPES = [(4, 2, 4), (2, 4, 4), (1, 8, 4)]         # WX, WY, RPW: 1024x8, 512x16, 256x32 px
TILE_STORES = [("nt", 1, True), ("plain", 0, True), ("hybrid", 5, False)]      # name, ST, has the 128-byte aligned arm


def tile_kernels():
    out = []
    for wx, wy, rpw in TILE_SHAPES:
        size = "%dx%d" % (256 * wx, wy * rpw)
        for store, st, has_arm in TILE_STORES:
            for arm, generic in (("fast path (W%16==0)", 0), ("generic path (any even W)", 1)):
                out.append(("bayer2rgb %s tile, %s stores, %s" % (size, store, arm),
                            "bayer2rgb_lds_kernelILi%dELi%dELi%dELi0ELi%dELb1ELb%dEE" % (wx, wy, rpw, st, generic)))
            if has_arm:
                out.append(("bayer2rgb %s tile, %s stores, 128-byte aligned arm (generic geometries)" % (size, store),
                            "bayer2rgb_lds_aligned_kernelILi%dELi%dELi%dELi%dELi128EE" % (wx, wy, rpw, st)))
    return out


# demangled-name fragments of the kernels that ship as defaults (everything else in the variant table is an A/B arm)
PRODUCTION = tile_kernels() + [
    ("rgb2bayer flat kernel, 2 groups/thread, 4 px/group, nt loads, 16-byte path -- default",
     "rgb2bayer_flat_kernelILi2ELi4ELi1ELi16EE"),
    ("rgb2bayer flat kernel, generic path (width % 4 != 0 or unaligned frames)", "rgb2bayer_flat_kernelILi2ELi4ELi1ELi4EE"),
    ("synthetic frame generator (bench input)", "fill_synthetic_kernel"),
    ("deep samples: 16-bit words -> 16-bit channels (ARGB64 & co.)", "bayer2rgb_deep_kernelILb0ELb1EE"),
    ("deep samples: 16-bit words -> 8-bit channels", "bayer2rgb_deep_kernelILb0ELb0EE"),
    ("deep samples: 8-bit mosaic -> 16-bit channels", "bayer2rgb_deep_kernelILb1ELb1EE"),
    ("deep samples: 8-bit mosaic -> 8-bit channels (3-byte pixels or planes: MIBAYER_FLAG_DST_24BIT / _DST_PLANAR)",
     "bayer2rgb_deep_kernelILb1ELb0EE"),
    ("Malvar-He-Cutler: 8-bit mosaic -> 8-bit channels", "bayer2rgb_mhc_kernelILb1ELb0EE"),
    ("Malvar-He-Cutler: 8-bit mosaic -> 16-bit channels", "bayer2rgb_mhc_kernelILb1ELb1EE"),
    ("Malvar-He-Cutler: 16-bit words -> 8-bit channels", "bayer2rgb_mhc_kernelILb0ELb0EE"),
    ("Malvar-He-Cutler: 16-bit words -> 16-bit channels", "bayer2rgb_mhc_kernelILb0ELb1EE"),
    ("fused colour stage: either demosaic, every sample / channel width (run-time branches)", "bayer2rgb_colour_kernel"),
    ("mosaic zone statistics: both sample widths and byte orders (run-time branches)", "mosaic_stats_kernel"),
    ("mosaic histogram: both sample widths and byte orders (run-time branches)", "mosaic_hist_kernel"),
    ("mosaic focus statistics: 8-bit mosaic (packed 16-bit halves)", "mosaic_focus_kernelILb1EE"),
    ("mosaic focus statistics: 16-bit words, both byte orders", "mosaic_focus_kernelILb0EE"),
]
INTERESTING = ["v_lerp_u8", "v_perm_b32", "v_alignbit_b32", "v_bfi_b32", "v_mov_b32_dpp", "ds_bpermute_b32",
               "global_load_dwordx4", "global_load_dwordx2", "global_load_dword", "global_store_dwordx4",
               "global_store_dwordx3", "global_store_dwordx2", "global_store_dword", "global_store_short",
               "ds_write_b128", "ds_write_b32", "ds_read_b32", "ds_add_u32", "ds_add_u64", "global_atomic_add",
               "global_atomic_add_x2",
               "ds_read_b128", "ds_read2_b32", "v_mad_i32_i24", "v_mad_u32_u24", "v_mul_i32_i24", "v_mul_u32_u24", "s_sleep", "s_barrier", "s_waitcnt", "v_mfma", "scratch_", "buffer_"]

subprocess.run(["make", "-C", PKG, "asm"], check=True, stdout=subprocess.DEVNULL)
asm = open(os.path.join(PKG, "build", "mibayer_kernels-hip-amdgcn-amd-amdhsa-gfx950.s")).read()
usage = open(os.path.join(PKG, "build", "resource_usage.txt")).read()

res = {}
cur = None
for line in usage.splitlines():
    m = re.search(r"Function Name: (\S+)", line)
    if m:
        cur = m.group(1)
        res[cur] = {}
        continue
    m = re.search(r"remark: [^ ]+\s+(.+?): (\S+) \[-Rpass", line)
    if m and cur:
        res[cur][m.group(1).strip()] = m.group(2)

bodies = {}
for m in re.finditer(r"^(_ZN7mibayer\w+):\s*; @\1\n(.*?)\n\.Lfunc_end", asm, re.S | re.M):
    bodies[m.group(1)] = m.group(2)

# a second argument names the file (a pair of summaries around a refactor: ..._isa_parent.md, ..._isa_after.md)
path = os.path.join(ROOT, "profiles", sys.argv[2] if len(sys.argv) > 2 else "%s_isa_summary.md" % tag)
out = ["# profiles/%s -- gfx950 ISA and resources of the production kernels" % os.path.basename(path), "",
       "Generated by `python tools/isa_summary.py %s` (hipcc -O3 --offload-arch=gfx950 -save-temps, "
       "`-Rpass-analysis=kernel-resource-usage`); %d kernels in the translation unit, the A/B arms are omitted." % (
           tag, len(res)), ""]
for title, frag in PRODUCTION:
    names = [n for n in res if frag in n]
    if not names:
        out += ["## %s" % title, "", "(not found: `%s`)" % frag, ""]
        continue
    name = names[0]
    r = res[name]
    body = bodies.get(name, "")
    insts = [ln.split()[0] for ln in body.splitlines()
             if ln.startswith("\t") and not ln.strip().startswith((";", ".")) and ln.split()]
    hist = collections.Counter(insts)
    nt_stores = len(re.findall(r"global_store_\w+ .* nt", body))
    nt_loads = len(re.findall(r"global_load_\w+ .* nt", body))
    dpp = collections.Counter(re.findall(r"(wave_sh[lr]:1|row_sh[lr]:\d+)", body))
    out += ["## %s" % title, "", "`%s`" % name, "",
            "| VGPRs | AGPRs | SGPRs | scratch B/lane | LDS B/block | occupancy waves/SIMD | spills | instructions |",
            "|---:|---:|---:|---:|---:|---:|---:|---:|",
            "| %s | %s | %s | %s | %s | %s | %s / %s | %d |" % (
                r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"),
                r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]"), r.get("SGPRs Spill"),
                r.get("VGPRs Spill"), len(insts)), ""]
    rows = []
    for key in INTERESTING:
        family = key.endswith("_") or key in ("v_mfma", "v_mov_b32_dpp", "s_sleep", "s_waitcnt")
        n = sum(v for k, v in hist.items() if (k.startswith(key) if family else k == key))
        if n or key in ("v_mfma", "scratch_"):
            rows.append("%s x%d" % (key + ("*" if key.endswith("_") or key == "v_mfma" else ""), n))
    out += ["Instruction mix: " + ", ".join(rows) + ".",
            "Cache hints: %d store(s) and %d load(s) carry `nt`.  DPP controls: %s." % (
                nt_stores, nt_loads, ", ".join("%s x%d" % kv for kv in sorted(dpp.items())) or "none"), ""]
    top = ", ".join("%s %d" % kv for kv in hist.most_common(12))
    out += ["Most frequent: " + top + ".", ""]
with open(path, "w") as f:
    f.write("\n".join(out) + "\n")
print("\n".join(out))
