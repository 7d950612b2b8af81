"""Static instruction counts of one collide_kernel instantiation, per phase of the step and per instruction class.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -fno-fast-math --cuda-device-only -S -g1 \
          -Rpass-analysis=kernel-resource-usage tactics2d_amd/csrc/t2d_collide.hip -o step.s 2> step.remarks
    python scripts/static_phase_counts.py step.s [--kernel ILb1ELi1ELb0ELb1ELb0ELb0ELi0ELb0ELb1EE] [--remarks step.remarks] [--json out.json] [--csrc DIR]

-g1 makes the assembler text carry one `.loc` per change of source position, with the chain of inlined call sites behind it
(`; t2d_geom_dev.h:88:5 @[ t2d_collide.hip:1351:40 @[ ... ] ]`).  An instruction belongs to the innermost position of that
chain that lies in one of the step's named functions (process_lane, compact_and_process, box_sweep, an integrator model, ...);
when none does, to the phase of the kernel body its outermost position lies in.  The phase borders are found by text in
the sources, not by line numbers, so the tool follows edits.  The default kernel is the chained fast instantiation with the
shape of 64-wide envs compiled in, <1, 1, 0, CHAIN, 0, 0, 0, 0, W64> (what `bench.py` times; its generic twin, and the name in
a tree from before the ninth template parameter: --kernel ...ELb0ELb0EE / ...ELb0EE).  Counts are STATIC (instructions in the
text), not what a wave executes.
"""
import argparse
import collections
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "tactics2d_amd", "csrc")

# (file, text that opens the range) in source order; a range ends where the next one of the same file opens.
# `fn` ranges win over `body` ranges: they are inlined functions / lambdas, found anywhere in the inlined-at chain.
ANCHORS = [
    ("t2d_collide.hip", "fn", "other helpers", "T2D_DEV Quad load_obb_lds("),
    ("t2d_collide.hip", "fn", "compact_and_process", "template <bool SWAP, bool RING = false, class F>"),
    ("t2d_collide.hip", "fn", "other helpers", "#ifdef T2D_TIMING\n#define T2D_MARK"),
    ("t2d_collide.hip", "body", "start-up", "__launch_bounds__((1 + PIPE) * kBlock"),
    ("t2d_collide.hip", "body", "integrator: call + state stores", "(SingleTrackDrift and euler point-mass lanes were integrated by drift_kernel"),
    ("t2d_collide.hip", "body", "pose", "double pre_tp = 0.0;"),
    ("t2d_collide.hip", "fn", "pair narrow (process_pair / process_ring)", "auto rad_of = [&](int i) -> double {"),
    ("t2d_collide.hip", "body", "stage plumbing", "const KernargView ev_args = late_args();"),
    ("t2d_collide.hip", "fn", "static narrow (process_static)", "auto process_static = [&](uint32_t e) {"),
    ("t2d_collide.hip", "fn", "process_lane", "// off-lane = not union(lanes).contains(pose), the oracle's definition"),
    ("t2d_collide.hip", "body", "stage plumbing", "int n_lane_polys = 0;"),
    ("t2d_collide.hip", "body", "pair sweep (ring)", "if (T2D_PROBE_SKIP & 1) {"),
    ("t2d_collide.hip", "body", "stage plumbing", "    T2D_MARK(4);\n"),
    ("t2d_collide.hip", "fn", "sweep_stage / box_sweep", "typedef float f2p __attribute__((ext_vector_type(2)));"),
    ("t2d_collide.hip", "body", "stage plumbing", "const f2p bxp = {-box_hi_x, box_lo_x}"),
    ("t2d_collide.hip", "body", "reduce / epilogue", "// ---------------- phase 3: reduce + status epilogue"),
    ("t2d_collide.hip", "body", "tail", "if (CHAIN) {   // this step of these envs is complete"),
    ("t2d_integrate_dev.h", "fn", "integrator: shared helpers", "namespace integ {"),
    ("t2d_integrate_dev.h", "fn", "integrator: kinematics", "template <int VARIANT, bool RESUM = false, typename PF>\nT2D_DEV StepOut step_kinematics("),
    ("t2d_integrate_dev.h", "fn", "integrator: dynamics", "template <int VARIANT, typename PF>\nT2D_DEV StepOut step_dynamics("),
    ("t2d_integrate_dev.h", "fn", "integrator: point mass", "template <typename PF>\nT2D_DEV StepOut step_pointmass("),
    ("t2d_integrate_dev.h", "fn", "integrator: call + state stores", "template <int VARIANT, bool RESUM = false, typename PF>\nT2D_DEV StepOut step_participant("),
]
PHASES = ["start-up", "integrator: kinematics", "integrator: dynamics", "integrator: point mass", "integrator: shared helpers",
          "integrator: call + state stores", "pose", "pair sweep (ring)", "pair narrow (process_pair / process_ring)",
          "sweep_stage / box_sweep", "compact_and_process", "static narrow (process_static)", "process_lane", "stage plumbing",
          "other helpers", "reduce / epilogue", "tail", "unattributed"]
CLASSES = ["salu", "branch", "exec", "wait", "lanes", "cndmask", "valu", "smem", "lds", "vmem", "other"]


def ranges(csrc):
    out = collections.defaultdict(list)   # file -> [(first line, kind, phase)]
    for fname, kind, phase, text in ANCHORS:
        src = open(os.path.join(csrc, fname)).read()
        at = src.find(text)
        if at < 0:
            sys.exit(f"anchor not found in {fname}: {text!r}")
        out[fname].append((src.count("\n", 0, at) + 1, kind, phase))
    for v in out.values():
        v.sort()
    return out


def lookup(rng, fname, line):
    hit = None
    for first, kind, phase in rng.get(fname, ()):
        if first <= line:
            hit = (kind, phase)
    return hit


def classify(op, rest):
    if op in ("s_waitcnt", "s_nop"):
        return "wait"
    if op.startswith("s_cbranch") or op == "s_branch":
        return "branch"
    if op.startswith("s_"):
        if "saveexec" in op or rest.split(",")[0].strip().startswith("exec"):
            return "exec"
        if op.startswith(("s_load", "s_buffer_load")):
            return "smem"
        if op.startswith(("s_barrier", "s_sleep", "s_setprio", "s_endpgm", "s_getreg", "s_memtime", "s_memrealtime", "s_sendmsg", "s_setpc", "s_swappc", "s_getpc")):
            return "other"
        return "salu"
    if op.startswith(("v_readlane", "v_writelane")):
        return "lanes"
    if op.startswith("v_"):
        return "valu"
    if op.startswith("ds_"):
        return "lds"
    if op.startswith(("global_", "flat_", "buffer_", "scratch_")):
        return "vmem"
    return "other"


LOC = re.compile(r"\.loc\s+\d+\s+\d+\s+\d+.*?;\s*(.*)$")
POS = re.compile(r"([\w.+-]+):(\d+):\d+")
INS = re.compile(r"^\t([a-z][a-z0-9_]+)(?:\s+(.*))?$")


def count(asm_path, kernel, csrc=CSRC):
    rng = ranges(csrc)
    tab = {p: collections.Counter() for p in PHASES}
    inside, phase = False, "unattributed"
    for raw in open(asm_path):
        line = raw.rstrip("\n")
        if not inside:
            if line.startswith("_ZN") and kernel in line and line.split(":")[0].endswith("ii"):
                inside = True
            continue
        if line.startswith(".Lfunc_end"):
            break
        m = LOC.search(line)
        if m:
            chain = [(f, int(n)) for f, n in POS.findall(m.group(1))]
            if chain and chain[-1][1] != 0:
                new = None
                for f, n in chain:   # innermost first
                    r = lookup(rng, f, n)
                    if r and r[0] == "fn":
                        new = r[1]
                        break
                if new is None:
                    r = lookup(rng, *chain[-1])
                    new = r[1] if r else None
                if new is not None:
                    phase = new
            continue
        m = INS.match(line)
        if not m or m.group(1).startswith("."):
            continue
        op, rest = m.group(1), m.group(2) or ""
        c = classify(op, rest)
        tab[phase][c] += 1
        if op.startswith("v_cndmask"):
            tab[phase]["cndmask"] += 1
    if not inside:
        sys.exit(f"kernel {kernel} not found in {asm_path}")
    return tab


def resources(remarks, kernel):
    out, on = {}, False
    for line in open(remarks):
        if "Function Name:" in line:
            on = kernel in line
        elif on:
            m = re.search(r"remark:\s+([\w /\[\]]+?):\s+(\S+) \[-Rpass", line)
            if m:
                out[m.group(1).strip()] = m.group(2)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("--kernel", default="collide_kernelILb1ELi1ELb0ELb1ELb0ELb0ELi0ELb0ELb1EE")
    ap.add_argument("--remarks")
    ap.add_argument("--json")
    ap.add_argument("--csrc", default=CSRC, help="the sources the assembly was compiled from (another commit's: a copy of its csrc/)")
    a = ap.parse_args()
    tab = count(a.asm, a.kernel, a.csrc)
    total = collections.Counter()
    print("| phase | " + " | ".join(CLASSES) + " |")
    print("|---|" + "---|" * len(CLASSES))
    for p in PHASES:
        if sum(tab[p].values()) == 0:
            continue
        total.update(tab[p])
        print(f"| {p} | " + " | ".join(str(tab[p][c]) for c in CLASSES) + " |")
    print("| **kernel** | " + " | ".join(str(total[c]) for c in CLASSES) + " |")
    print("\n(salu = scalar ALU incl. compares and moves; exec = saveexec and writes of exec; wait = s_waitcnt + s_nop; lanes = "
          "v_readlane + v_writelane; cndmask is also counted in valu)")
    res = resources(a.remarks, a.kernel) if a.remarks else {}
    if res:
        print("\nresources: " + ", ".join(f"{k} {v}" for k, v in res.items()))
    if a.json:
        with open(a.json, "w") as fh:
            json.dump({"kernel": a.kernel, "phases": {p: dict(tab[p]) for p in PHASES if tab[p]}, "kernel_total": dict(total),
                       "resources": res}, fh, indent=1)


if __name__ == "__main__":
    main()
