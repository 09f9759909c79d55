#!/usr/bin/env python3
"""Per-kernel comparison of two trees' device assembly:  tools/isa_diff.py <dir_parent> <dir_new> [out.json]

Each directory holds <file>.s for the same .hip files, compiled device-only to assembly with the Makefile's FLAGS (tools/isa_count.sh
shows the command line).  Per kernel: whether the instruction lines are identical once the .LBB label numbers are renumbered in
order of appearance, whether the instruction counts are equal, whether the opcode histograms are (the first token of every
instruction line, compared as a multiset: equal where only register numbers, offsets and the order of instructions moved), and
vgpr_count / sgpr_count / private_segment_fixed_size / group_segment_fixed_size from the code object metadata.  Exit status 1 if a
kernel exists on one side only, gains scratch, or gains VGPRs."""
import collections
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
        ops = collections.Counter(i.split()[0] for i in ins if not i.startswith(".L"))
        out[name] = {"stream": ins, "opcodes": ops, "instructions": sum(ops.values()), **{k: int(md[k]) for k in META}}
    return out


def shown(k):
    return {key: v for key, v in k.items() if key not in ("stream", "opcodes")}


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
            per[name] = {"identical": p["stream"] == n["stream"], "same_instruction_count": p["instructions"] == n["instructions"],
                         "same_opcode_histogram": p["opcodes"] == n["opcodes"], "parent": shown(p), "new": shown(n)}
            if n["private_segment_fixed_size"] > p["private_segment_fixed_size"] or n["vgpr_count"] > p["vgpr_count"]:
                bad.append(name + ": more scratch or VGPRs than the parent")
        res[f[:-2] + ".hip"] = {"kernels": len(per), "identical": sum(k["identical"] for k in per.values()), "per_kernel": per}
        print(f"{f[:-2]}.hip: {len(per)} kernels, {res[f[:-2] + '.hip']['identical']} identical to the parent")
        for name, k in per.items():
            if not k["identical"]:
                print("   differs:", name, "instruction count", "equal," if k["same_instruction_count"] else "DIFFERS,",
                      "opcode histogram", "equal" if k["same_opcode_histogram"] else "DIFFERS", k["parent"], k["new"])
    if len(sys.argv) > 3:
        json.dump(res, open(sys.argv[3], "w"), indent=1)
    for b in bad:
        print("FAIL", b)
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
