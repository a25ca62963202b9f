#!/usr/bin/env python3
"""Which kernels of csrc/mibayer_kernels.hip changed between two builds: compares the gfx950 instruction streams of two
`make -C gst-plugins-bad_amd asm` listings function by function, label numbers aside, and prints a markdown report with
the resources and the instruction mix of the functions that are new.

  python tools/isa_compare.py PARENT.s THIS.s [THIS_resource_usage.txt] > profiles/<date>_<what>_isa_compare.md

PARENT.s / THIS.s: build/mibayer_kernels-hip-amdgcn-amd-amdhsa-gfx950.s of the two trees; the optional third file is
build/resource_usage.txt of the second (hipcc -Rpass-analysis=kernel-resource-usage)."""
import collections
import re
import sys


def bodies(path):
    asm = open(path).read()
    return {m.group(1): m.group(2)
            for m in re.finditer(r"^(_ZN7mibayer\w+):\s*; @\1\n(.*?)\n\.Lfunc_end", asm, re.S | re.M)}


def stream(body):
    """the instructions of a function, comments and directives dropped, local labels renumbered in order of appearance"""
    lines = [ln.split(";")[0].strip() for ln in body.splitlines()]
    lines = [ln for ln in lines if ln and not ln.startswith(".") or re.match(r"\.LBB\d+_\d+:", ln or "")]
    names = {}
    out = []
    for ln in lines:
        out.append(re.sub(r"\.LBB\d+_\d+", lambda m: names.setdefault(m.group(0), "L%d" % len(names)), ln))
    return out


def resources(path):
    res, cur = {}, None
    for line in open(path).read().splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = m.group(1)
            res[cur] = {}
            continue
        m = re.search(r"remark: [^ ]+\s+(.+?): (\S+) \[-Rpass", line)
        if m and cur:
            res[cur][m.group(1).strip()] = m.group(2)
    return res


def main():
    old, new = bodies(sys.argv[1]), bodies(sys.argv[2])
    res = resources(sys.argv[3]) if len(sys.argv) > 3 else {}
    same = [k for k in old if k in new and stream(old[k]) == stream(new[k])]
    changed = [k for k in old if k in new and stream(old[k]) != stream(new[k])]
    gone = [k for k in old if k not in new]
    added = [k for k in new if k not in old]
    print("# gfx950 instruction streams, function by function: parent against this commit\n")
    print("`tools/isa_compare.py` over the two `make asm` listings (hipcc -O3 --offload-arch=gfx950 -save-temps), label "
          "numbers aside.\n")
    print("* kernel functions in the parent: %d; in this commit: %d" % (len(old), len(new)))
    print("* the same instruction stream in both: %d" % len(same))
    print("* changed: %d%s" % (len(changed), "".join("\n  * `%s`" % k for k in changed)))
    print("* removed: %d%s" % (len(gone), "".join("\n  * `%s`" % k for k in gone)))
    print("* new: %d%s\n" % (len(added), "".join("\n  * `%s`" % k for k in added)))
    for k in added:
        insts = [ln.split()[0] for ln in stream(new[k]) if not ln.endswith(":")]
        hist = collections.Counter(insts)
        r = res.get(k, {})
        print("## `%s`\n" % k)
        print("| VGPRs | AGPRs | SGPRs | scratch B/lane | LDS B/block | occupancy waves/SIMD | spills (SGPR / VGPR) | instructions |")
        print("|---:|---:|---:|---:|---:|---:|---:|---:|")
        print("| %s | %s | %s | %s | %s | %s | %s / %s | %d |\n" % (
            r.get("VGPRs"), r.get("AGPRs"), r.get("TotalSGPRs"), r.get("ScratchSize [bytes/lane]"),
            r.get("LDS Size [bytes/block]"), r.get("Occupancy [waves/SIMD]"), r.get("SGPRs Spill"), r.get("VGPRs Spill"),
            len(insts)))
        families = collections.Counter()
        for name, n in hist.items():
            for fam in ("global_load", "global_atomic", "ds_add", "ds_", "v_pk_", "v_mov", "v_perm", "v_alignbyte", "s_waitcnt",
                        "s_barrier", "scratch_", "buffer_"):
                if name.startswith(fam):
                    families[fam + "*"] += n
                    break
        for fam in ("scratch_*", "buffer_*"):
            families.setdefault(fam, 0)
        print("Instruction families: " + ", ".join("%s x%d" % kv for kv in sorted(families.items())) + ".")
        print("Most frequent: " + ", ".join("%s %d" % kv for kv in hist.most_common(14)) + ".\n")


if __name__ == "__main__":
    main()
