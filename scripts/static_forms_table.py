"""Resource lines and per-class static instruction counts of EVERY collide_kernel instantiation of one or two builds, as a table.

    python scripts/static_forms_table.py new.s new.remarks [--parent old.s old.remarks --parent-csrc OLD/tactics2d_amd/csrc]

(the files: see scripts/static_phase_counts.py for the hipcc line.)  With --parent, every instantiation the two builds share is
held equal -- resources and counts -- and the ones only the new build has (the W64 twins) are listed beside
the generic instantiation of the same form.  Exit status 1 when a shared instantiation differs.
"""
import argparse
import collections
import re
import sys

import static_phase_counts as S

KEYS = ("VGPRs", "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]", "Occupancy [waves/SIMD]")
SHOW = ("salu", "branch", "exec", "valu", "lanes", "wait", "smem", "lds", "vmem")


def kernels(remarks):
    names = []
    for line in open(remarks):
        m = re.search(r"Function Name: (\S*collide_kernel\S*)", line)
        if m and m.group(1) not in names:
            names.append(m.group(1))
    return names


def template_args(mangled):
    """'ILb1ELi1ELb0ELb1E...E' -> ('1', '1', '0', '1', ...): the instantiation's template arguments"""
    m = re.search(r"collide_kernelI((?:L[bi]n?\d+E)+)E", mangled)
    return tuple(a[2:-1].replace("n", "-") for a in re.findall(r"L[bi]n?\d+E", m.group(1)))


def facts(asm, remarks, csrc):
    out = {}
    for k in kernels(remarks):
        tab = S.count(asm, k, csrc)
        total = collections.Counter()
        for p in tab.values():
            total.update(p)
        res = S.resources(remarks, k)
        out[template_args(k)] = (tuple(res.get(x, "?") for x in KEYS), tuple(total[c] for c in SHOW))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("asm")
    ap.add_argument("remarks")
    ap.add_argument("--parent", nargs=2)
    ap.add_argument("--parent-csrc", default=S.CSRC)
    a = ap.parse_args()
    new = facts(a.asm, a.remarks, S.CSRC)
    old = facts(a.parent[0], a.parent[1], a.parent_csrc) if a.parent else {}
    bad = 0
    print("| <WITH_STATUS, FUSE, IOU, CHAIN, LOOP, SPLIT, PIPE, IDMF, W64> | VGPRs | scalar / vector spills | LDS B | waves/SIMD | "
          + " | ".join(SHOW) + " | parent |")
    print("|---|---|---|---|---|" + "---|" * (len(SHOW) + 1))
    for args in sorted(new, key=lambda t: (t[:8], t[8:])):
        res, cnt = new[args]
        w64 = len(args) > 8 and args[8] == "1"
        twin = old.get(args[:8]) if old else None
        verdict = ""
        if old:
            if w64:
                verdict = "new"
            elif twin is None:
                verdict = "not in the parent"
            elif twin == (res, cnt):
                verdict = "equal"
            else:
                verdict = f"DIFFERS: {twin}"
                bad += 1
        print(f"| {', '.join(args)} | {res[0]} | {res[1]} / {res[2]} | {res[3]} | {res[4]} | " + " | ".join(map(str, cnt)) + f" | {verdict} |")
    if old:
        print(f"\n{len(new)} instantiations, {len(old)} in the parent, {bad} shared ones differ")
    sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
