"""Static instruction budget of the pair rounds (no GPU needed):  python tools/round_isa_budget.py [--asm FILE] [extra hipcc flags]

Compiles msm.hip for gfx950 to assembly with line tables (the build's own flags plus -S -gline-tables-only), takes
k_affine_round<true,false,false> and <false,false,false> apart into the pass-1 slot loop, the pass-2 slot loop and the code outside
them, and counts instruction classes in each: VALU (v_*), LDS (ds_*), VMEM (global_* / buffer_* / flat_* / scratch_*), SALU (s_* that
compute), SMEM (s_load_*) and the rest (waits, branches, priorities, barriers).  Within a region the instructions the compiler inlined
from the Karatsuba multiplier (gf233.cuh from GF_LDSK_BYTES_PER_WAVE to gf_mul3: gf_mul, gf_mul2 and what they call) are the
"products"; of everything else, what the source keeps behind a wave-uniform branch no wave of a real input takes (the blocks of
msm_rounds.cuh that open with `if (__any(`: the rare cases) is "rare", and what remains is the "rest" -- the instructions a slot
executes beside its products, which this table is for.

The slot loops are the two outermost loops of the kernel that rotate the wave priority (s_setprio inside: AFF_PRIO), in address order.  Counts are STATIC: a branch inside a loop body
counts whether a wave takes it or not.  The multiplier's row loops are rolled with three trips each (GF_K_LOOP), so the "x3" column
weighs every instruction of a loop nested in a slot loop three times per level: that is what a slot executes when every branch of the
body is taken.  A diagnostic, not a test."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "dv-pari_amd", "csrc")
KERNELS = ("k_affine_roundILb1ELb0ELb0E", "k_affine_roundILb0ELb0ELb0E")
CLASSES = ("VALU", "LDS", "VMEM", "SALU", "SMEM", "other")
BRANCHES = ("s_branch", "s_cbranch")


def product_lines():
    """[first, last] line of gf233.cuh that belongs to the Karatsuba multiplier"""
    first = last = None
    with open(os.path.join(CSRC, "gf233.cuh")) as f:
        for i, line in enumerate(f, 1):
            if first is None and "GF_LDSK_BYTES_PER_WAVE =" in line:
                first = i
            if last is None and line.startswith("GF_DEV void gf_mul3("):
                last = i - 1
    assert first and last and first < last, "gf233.cuh: the multiplier's section was not found"
    return first, last


def rare_lines():
    """the [first, last] line spans of msm_rounds.cuh's blocks that open with `if (__any(`"""
    spans, open_at, level = [], None, 0
    with open(os.path.join(CSRC, "msm_rounds.cuh")) as f:
        for i, line in enumerate(f, 1):
            code = line.split("//")[0]
            if open_at is None and code.strip().startswith("if (__any(") and code.rstrip().endswith("{"):
                open_at, level = i, 0
            if open_at is not None:
                level += code.count("{") - code.count("}")
                if level == 0:
                    spans.append((open_at, i))
                    open_at = None
    return spans


def compile_asm(extra):
    tmp = tempfile.mkdtemp(prefix="round_isa_")
    out = os.path.join(tmp, "msm.s")
    cmd = [os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "--offload-arch=gfx950", "-std=c++17", "-fPIC", "-x", "hip",
           os.path.join("dv-pari_amd", "csrc", "msm.hip"), "--cuda-device-only", "-S", "-gline-tables-only", "-o", out,
           "-Wno-pass-failed", "-Wno-int-to-pointer-cast", "-Wno-unused-command-line-argument"] + extra
    subprocess.check_call(cmd, cwd=ROOT)
    return out


def classify(mn):
    if mn.startswith("v_"):
        return "VALU"
    if mn.startswith("ds_"):
        return "LDS"
    if mn.startswith(("global_", "buffer_", "flat_", "scratch_")):
        return "VMEM"
    if mn.startswith("s_load"):
        return "SMEM"
    if mn.startswith(("s_waitcnt", "s_nop", "s_barrier", "s_endpgm", "s_setprio", "s_sleep", "s_code_end") + BRANCHES):
        return "other"
    if mn.startswith("s_"):
        return "SALU"
    return "other"


def kernel_body(lines, mangled):
    """(instructions, labels) of one kernel: instructions as (mnemonic, operands, part), labels name -> index of the next one"""
    lo, hi = product_lines()
    rare = rare_lines()
    frame = re.compile(r"gf233\.cuh:(\d+):")
    frame_k = re.compile(r"msm_rounds\.cuh:(\d+):")
    ins, labels, on, prod = [], {}, False, "rest"
    for ln in lines:
        if not on:
            on = ln.startswith("_ZN3dvp14" + mangled) and ln.rstrip().split(";")[0].rstrip().endswith(":")
            continue
        s = ln.strip()
        if s.startswith(".Lfunc_end"):
            break
        if s.startswith(".loc"):
            prod = ("products" if any(lo <= int(x) <= hi for x in frame.findall(s)) else
                    "rare" if any(a <= int(x) <= b for x in frame_k.findall(s) for a, b in rare) else "rest")
            continue
        m = re.match(r"(\.LBB\d+_\d+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if not s or s.startswith((".", ";")) or not ln.startswith("\t"):
            continue
        parts = s.split(";")[0].split(None, 1)
        ins.append((parts[0], parts[1] if len(parts) > 1 else "", prod))
    assert ins, "kernel not found: " + mangled
    return ins, labels


def sccs(nodes, succ):
    """strongly connected components of the graph restricted to `nodes` (Tarjan, iterative)"""
    index, low, on, stack, out, n = {}, {}, set(), [], [], 0
    for root in nodes:
        if root in index:
            continue
        work = [(root, iter([s for s in succ[root] if s in nodes]))]
        index[root] = low[root] = n; n += 1; stack.append(root); on.add(root)
        while work:
            v, it = work[-1]
            for w in it:
                if w not in index:
                    index[w] = low[w] = n; n += 1; stack.append(w); on.add(w)
                    work.append((w, iter([s for s in succ[w] if s in nodes])))
                    break
                if w in on:
                    low[v] = min(low[v], index[w])
            else:
                work.pop()
                if work:
                    low[work[-1][0]] = min(low[work[-1][0]], low[v])
                if low[v] == index[v]:
                    comp = set()
                    while True:
                        w = stack.pop(); on.discard(w); comp.add(w)
                        if w == v:
                            break
                    out.append(comp)
    return out


def loop_nest(ins, labels):
    """the kernel's loops from its control-flow graph: (depth of every instruction, the outermost loops as sets of instruction
    indices).  A loop is a strongly connected component; the loops nested in it are the components left once the edges into its
    entry blocks are cut"""
    starts = sorted(set([0] + list(labels.values()) + [i + 1 for i, x in enumerate(ins) if x[0].startswith(BRANCHES + ("s_endpgm",))]))
    starts = [s for s in starts if s < len(ins)]
    block_of = {}
    for b, s in enumerate(starts):
        for i in range(s, starts[b + 1] if b + 1 < len(starts) else len(ins)):
            block_of[i] = b
    succ = {b: set() for b in range(len(starts))}
    for b, s in enumerate(starts):
        last = (starts[b + 1] if b + 1 < len(starts) else len(ins)) - 1
        mn, ops, _ = ins[last]
        if mn.startswith(BRANCHES):
            t = labels.get(ops.strip())
            assert t is not None, "branch to an unknown label: " + ops
            if t < len(ins):
                succ[b].add(block_of[t])
        if not mn.startswith(("s_branch", "s_endpgm")) and b + 1 < len(starts):
            succ[b].add(b + 1)
    depth = dict.fromkeys(succ, 0)
    outer = []

    def descend(nodes, edges, level):
        for comp in sccs(nodes, edges):
            if len(comp) == 1 and next(iter(comp)) not in edges[next(iter(comp))]:
                continue
            for b in comp:
                depth[b] = level
            if level == 1:
                outer.append(comp)
            entries = {b for b in comp if any(b in edges[p] for p in nodes if p not in comp)} or {min(comp)}
            descend(comp, {b: {s for s in edges[b] if s in comp and s not in entries} for b in comp}, level + 1)

    descend(set(succ), succ, 1)
    return [depth[block_of[i]] for i in range(len(ins))], [{i for i in range(len(ins)) if block_of[i] in comp} for comp in outer]


def budget(ins, labels):
    depth, outer = loop_nest(ins, labels)
    slot = sorted((l for l in outer if any(ins[i][0] == "s_setprio" for i in l)), key=min)
    assert len(slot) == 2, f"{len(slot)} outermost loops hand the wave priority round, not two"
    regions = {"pass 1 loop": [], "pass 2 loop": [], "outside": []}
    for i in range(len(ins)):
        regions["pass 1 loop" if i in slot[0] else "pass 2 loop" if i in slot[1] else "outside"].append(i)
    rows = []
    for name, idx in regions.items():
        for part in ("products", "rest", "rare"):
            static = dict.fromkeys(CLASSES, 0)
            x3 = dict.fromkeys(CLASSES, 0)
            for i in idx:
                if ins[i][2] != part:
                    continue
                c = classify(ins[i][0])
                static[c] += 1
                x3[c] += 3 ** (depth[i] - 1) if name != "outside" else 0
            rows.append((name, part, static, x3))
    return rows


def main():
    args = sys.argv[1:]
    asm = None
    if args and args[0] == "--asm":
        asm, args = args[1], args[2:]
    with open(asm or compile_asm(args)) as f:
        lines = f.readlines()
    for mangled, shown in zip(KERNELS, ("k_affine_round<true,false,false>", "k_affine_round<false,false,false>")):
        ins, labels = kernel_body(lines, mangled)
        print(f"{shown}: {len(ins)} instructions")
        print(f"  {'region':<12} {'part':<9}" + "".join(f"{c:>7}" for c in CLASSES) + "   | x3:" + "".join(f"{c:>7}" for c in CLASSES[:4]))
        for name, part, static, x3 in budget(ins, labels):
            tail = "".join(f"{x3[c]:>7}" for c in CLASSES[:4]) if name != "outside" else ""
            print(f"  {name:<12} {part:<9}" + "".join(f"{static[c]:>7}" for c in CLASSES) + "   |    " + tail)


if __name__ == "__main__":
    main()
