#!/usr/bin/env python3
"""Per-kernel comparison of two trees' device assembly:  tools/isa_diff.py <dir_parent> <dir_new> [out.json]

Each directory holds <file>.s for the same .hip files, compiled device-only to assembly with the Makefile's FLAGS (tools/isa_count.sh
shows the command line).  Per kernel: whether the instruction lines are identical once the .LBB label numbers are renumbered in
order of appearance, the instruction counts, and vgpr_count / sgpr_count / private_segment_fixed_size / group_segment_fixed_size
from the code object metadata.  Exit status 1 if a kernel exists on one side only, gains scratch, or gains VGPRs."""
import json
import os
import re
import sys

META = ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "group_segment_fixed_size")


def kernels(path):
    lines = open(path).read().split("\n")
    meta, cur = {}, None
    for l in lines:  # the amdhsa.kernels list of the metadata note: one "  - " item per kernel
        if l.startswith("  - "):
            cur = {}
            l = "    " + l[4:]
        m = re.match(r"^    \.(\w+):\s+(\S+)$", l)
        if cur is not None and m:
            cur[m.group(1)] = m.group(2)
            if m.group(1) == "name":
                meta[m.group(2)] = cur
    out = {}
    for name, md in meta.items():
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        labels, ins = {}, []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].rstrip()
            if not re.match(r"^(\s+[a-z]|\.LBB)", l):
                continue
            l = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), ".L%d" % len(labels)), l)
            ins.append(" ".join(l.split()))
        out[name] = {"stream": ins, "instructions": sum(not i.startswith(".L") for i in ins), **{k: int(md[k]) for k in META}}
    return out


def main():
    dp, dn = sys.argv[1], sys.argv[2]
    res, bad = {}, []
    for f in sorted(os.listdir(dp)):
        if not f.endswith(".s"):
            continue
        kp, kn = kernels(os.path.join(dp, f)), kernels(os.path.join(dn, f))
        if set(kp) != set(kn):
            bad.append(f + ": kernel sets differ")
        per = {}
        for name in sorted(set(kp) & set(kn)):
            p, n = kp[name], kn[name]
            per[name] = {"identical": p["stream"] == n["stream"],
                         "parent": {k: v for k, v in p.items() if k != "stream"}, "new": {k: v for k, v in n.items() if k != "stream"}}
            if n["private_segment_fixed_size"] > p["private_segment_fixed_size"] or n["vgpr_count"] > p["vgpr_count"]:
                bad.append(name + ": more scratch or VGPRs than the parent")
        res[f[:-2] + ".hip"] = {"kernels": len(per), "identical": sum(k["identical"] for k in per.values()), "per_kernel": per}
        print(f"{f[:-2]}.hip: {len(per)} kernels, {res[f[:-2] + '.hip']['identical']} identical to the parent")
        for name, k in per.items():
            if not k["identical"]:
                print("   differs:", name, k["parent"], k["new"])
    if len(sys.argv) > 3:
        json.dump(res, open(sys.argv[3], "w"), indent=1)
    for b in bad:
        print("FAIL", b)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
