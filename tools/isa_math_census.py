"""Math / non-math census of a kernel's loops: how many VALU instructions of a loop body are the float routines of fgnn_math.h
(fg_exp / fg_log / fg_log1p, the sums, the sign handling) and how many are bookkeeping (addresses, counters, unpacking, bounds tests).
A sibling of tools/isa_cost_classes.py (which prices the same loops by issue class); reads the same device assembly:
    hipcc <the flags of csrc/Makefile> -S --cuda-device-only -o bp4.s feedback_gnn_amd/csrc/fgnn_bp4.hip
    python tools/isa_math_census.py bp4.s <kernel-name-substring> [min_loop_instructions]
    python tools/isa_math_census.py --checks bp4.s <kernel-name-substring>       one executed check of the kernels with compile-time trips
    python tools/isa_math_census.py --gnn-edge gnn.s <kernel-name-substring>     head and tail of the literal streaming GNN's edge loop
The classes are read off the mnemonic and its literal operands:
    float  every *_f32 arithmetic op, compare and select, v_cvt_f32_i32 (the exponent of a log), v_exp / v_log
    rint   the integer steps INSIDE the routines: ldexp (v_lshl_add_u32 .., 23, ..), the log's offset / exponent mask / table index
           (0xc0ca0000, 0xff800000, the WORD_1 select or a shift by 18), RC * 2^-e (v_sub_u32)
    sign   sign words: v_xor_b32, v_bfi_b32, |x| as an and with 0x7fffffff, syndrome bit << 31
    other  everything else — printed as a histogram so the split can be audited
`other` is the share a restructuring of the loops could remove; float + rint + sign is what the oracle's float operations cost."""
import collections
import re
import sys

FLOAT = re.compile(r"^v_(fma|fmac|fmaak|fmamk|mul|add|sub|subrev|med3|min|max|cmp_\w+|cmpx_\w+|exp|log|rcp|ldexp)_f32")


def classify(line):
    t = line.split(None, 1)
    op, args = t[0], (t[1].split(";")[0] if len(t) > 1 else "")
    if not op.startswith("v_"):
        return None
    if FLOAT.match(op) or op.startswith("v_cndmask") or op.startswith("v_cvt_f32_i32"):
        return "float"
    if op.startswith("v_lshl_add_u32") and re.search(r",\s*23\s*,", args):
        return "rint"
    if op.startswith(("v_add_u32", "v_add_co_u32")) and "0xc0ca0000" in args:
        return "rint"
    if op.startswith("v_and_b32") and ("0xff800000" in args or "WORD_1" in args):
        return "rint"
    if op.startswith(("v_bfe_u32", "v_lshrrev_b32")) and re.search(r",\s*18\b", args):
        return "rint"
    if op.startswith(("v_sub_u32", "v_subrev_u32")):
        return "rint"
    if op.startswith(("v_xor_b32", "v_bfi_b32", "v_and_or_b32")):
        return "sign"
    if op.startswith("v_and_b32") and "0x7fffffff" in args:
        return "sign"
    if op.startswith("v_lshlrev_b32") and re.match(r"\s*v\d+,\s*31\s*,", args):
        return "sign"
    return "other"


def main():
    txt = open(sys.argv[1]).read().split("\n")
    pat = sys.argv[2]
    minlen = int(sys.argv[3]) if len(sys.argv) > 3 else 150
    start = next(i for i, l in enumerate(txt) if l.startswith("_Z") and pat in l and ":" in l)
    end = next(i for i in range(start, len(txt)) if "s_endpgm" in txt[i])
    body = txt[start:end]
    labels = {}
    for i, l in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):", l)
        if m:
            labels[m.group(1)] = i
    loops = []
    for i, l in enumerate(body):
        m = re.match(r"^\s+s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            loops.append((labels[m.group(1)], i, m.group(1)))
    # innermost loops only: a loop that contains another is the sum of its children plus glue
    inner = [lp for lp in loops if not any(o is not lp and lp[0] <= o[0] and o[1] <= lp[1] for o in loops)]
    for a, b, name in inner:
        ins = [l.strip() for l in body[a:b + 1] if re.match(r"^\s+[a-z]", l)]
        if len(ins) < minlen:
            continue
        cls = collections.Counter()
        other = collections.Counter()
        non_valu = collections.Counter()
        for l in ins:
            c = classify(l)
            if c is None:
                non_valu[l.split()[0].split("_b")[0]] += 1
                continue
            cls[c] += 1
            if c == "other":
                other[l.split()[0]] += 1
        n = sum(cls.values())
        print(f"{name}: lines {a}..{b}: {n} VALU = {cls['float']} float + {cls['rint']} routine-integer + {cls['sign']} sign + "
              f"{cls['other']} other ({100.0 * cls['other'] / n:.1f} % non-math)")
        print("    other: " + ", ".join(f"{k} {v}" for k, v in other.most_common()))
        print("    non-VALU: " + ", ".join(f"{k} {v}" for k, v in non_valu.most_common()))


def kernel_body(path, pat):
    txt = open(path).read().split("\n")
    start = next(i for i, l in enumerate(txt) if l.startswith("_Z") and pat in l and ":" in l)
    end = next(i for i in range(start, len(txt)) if "s_endpgm" in txt[i])
    return [l.strip() for l in txt[start:end]]


def back_edges(body):
    """(first line, last line) of every loop: a conditional branch to a label above it."""
    labels = {m.group(1): i for i, l in enumerate(body) for m in [re.match(r"^(\.LBB\d+_\d+):", l)] if m}
    out = []
    for i, l in enumerate(body):
        m = re.match(r"^s_cbranch_\w+\s+(\.LBB\d+_\d+)", l)
        if m and labels.get(m.group(1), 1 << 30) < i:
            out.append((labels[m.group(1)], i))
    return out


def checks():
    """--checks bp4.s <kernel>: the kernels with compile-time trips have no check loop; one EXECUTED check is what lies between two
    consecutive row loads (global_load_dwordx4 at scalar base + 32-bit thread offset) of the unrolled check phase."""
    body = kernel_body(sys.argv[2], sys.argv[3])
    rows = [i for i, l in enumerate(body) if re.match(r"global_load_dwordx4 v\[\d+:\d+\], v\d+, s\[\d+:\d+\]$", l)]
    seen = collections.Counter()
    for a, b in zip(rows, rows[1:]):
        cls, other = collections.Counter(), collections.Counter()
        for l in body[a:b]:
            c = classify(l) if l and not l.startswith((";", ".")) else None
            if c:
                cls[c] += 1
            if c == "other":
                other[l.split()[0]] += 1
        n = sum(cls.values())
        if n > 700:  # the qubit phase of the next iteration lies between the last row of one copy and the first of the other
            continue
        seen[f"{n} VALU = {cls['float']} float + {cls['rint']} routine-integer + {cls['sign']} sign + {cls['other']} other"
             + (" (" + ", ".join(f"{k} {v}" for k, v in other.most_common()) + ")" if other else "")] += 1
    for k, v in seen.most_common():
        print(f"{v} x one executed check: {k}")


def gnn_edge():
    """--gnn-edge gnn.s <kernel>: the literal streaming GNN kernel's edge loops.  The unit loop is the innermost loop with ten
    v_pk_fma_f32; the edge loop is the smallest loop around it; `head` = the edge loop's VALU instructions before the unit loop (zeroing
    the message accumulators, picking gv[e]), `tail` = those after it (bias, accumulation into feat), per basic block so that the two
    sides of a scalar branch on e are told apart."""
    body = kernel_body(sys.argv[2], sys.argv[3])
    loops = back_edges(body)

    def valu(a, b):
        return collections.Counter(l.split()[0] for l in body[a:b] if l.startswith("v_"))

    def blocks(a, b):
        out, cur, name = [], collections.Counter(), "(fall-through)"
        for l in body[a:b]:
            m = re.match(r"^(\.LBB\d+_\d+):", l)
            if m or l.startswith(("s_cbranch", "s_branch")):
                if cur:
                    out.append((name, cur))
                cur = collections.Counter()
                if m:
                    name = m.group(1)
                continue
            if l.startswith("v_"):
                cur[l.split()[0]] += 1
        if cur:
            out.append((name, cur))
        return out

    fmt = lambda c: f"{sum(c.values())} VALU (" + ", ".join(f"{k} {v}" for k, v in c.most_common()) + ")"
    for a, b in loops:
        if sum("v_pk_fma_f32" in l for l in body[a:b]) != 10 or any(a < x and y < b for x, y in loops):
            continue
        outer = [(x, y) for x, y in loops if x < a and y > b]
        x, y = min(outer, key=lambda t: t[1] - t[0])
        # the edge loop may close through a later unconditional branch: extend to the last branch back to its header
        hdr = re.match(r"^(\.LBB\d+_\d+):", body[x]).group(1)
        for i in range(y, len(body)):
            if re.match(r"^s_(c)?branch\w*\s+" + re.escape(hdr) + r"$", body[i]):
                y = i
            if i > y + 120:
                break
        print(f"unit loop lines {a}..{b}: {fmt(valu(a, b))}, s_load {sum('s_load' in l for l in body[a:b])}")
        print(f"  edge loop lines {x}..{y}: head {fmt(valu(x, a))}")
        for name, c in blocks(b + 1, y + 1):
            print(f"    tail block {name}: {fmt(c)}")


if __name__ == "__main__":
    if len(sys.argv) > 1 and sys.argv[1] == "--checks":
        checks()
    elif len(sys.argv) > 1 and sys.argv[1] == "--gnn-edge":
        gnn_edge()
    else:
        main()
