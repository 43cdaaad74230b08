"""Turns the `NORM_SWEEP` lines of tests/test_norm_sweep.py (`pytest -s`) into the tables of profiles/norm_accuracy.md.

    python tools/norm_accuracy.py emu.log hip.log > tables.md

Per backend, entry and output: the number of comparisons, the comparison that came nearest to its bound (ratio / bound), and the one with the
largest ratio e_kernel / max(e_torch_fp32, 4u); then one line per case with its branch and its worst comparison.
"""
import re
import sys

LINE = re.compile(r"NORM_SWEEP backend=(\S+) case=(\S+) branch=(\S+) entry=(\S+) out=(\S+) n=(\d+) e_kernel=(\S+) e_torch_fp32=(\S+) "
                  r"ratio=(\S+) bound=(\S+)")


def main(paths):
    rows = []
    for p in paths:
        for m in LINE.finditer(open(p, errors="replace").read()):
            b, case, branch, entry, out, n, ek, et, ratio, bound = m.groups()
            rows.append(dict(backend=b, case=case, branch=branch, entry=entry, out=out, n=int(n), ek=float(ek), et=float(et),
                             ratio=float(ratio), bound=float(bound)))
    for backend in sorted({r["backend"] for r in rows}):
        mine = [r for r in rows if r["backend"] == backend]
        print(f"\n## {backend}: worst comparison per entry and output ({len(mine)} comparisons)\n")
        print("| entry | output | comparisons | worst ratio | its bound M(n) | case | branch | e_kernel | e_torch_fp32 | nearest to its bound |")
        print("|---|---|---|---|---|---|---|---|---|---|")
        keys = []
        for r in mine:
            if (r["entry"], r["out"]) not in keys:
                keys.append((r["entry"], r["out"]))
        for entry, out in keys:
            grp = [r for r in mine if (r["entry"], r["out"]) == (entry, out)]
            w = max(grp, key=lambda r: r["ratio"])
            near = max(grp, key=lambda r: r["ratio"] / r["bound"])
            print(f"| `{entry}` | {out} | {len(grp)} | {w['ratio']:.2f} | {w['bound']:.2f} | {w['case']} | `{w['branch']}` | {w['ek']:.3e} | "
                  f"{w['et']:.3e} | {near['ratio']:.2f} / {near['bound']:.2f} ({near['case']}) |")
    print("\n## Every case: its branch and its worst comparison, per backend\n")
    print("| entry | case | branch | " + " | ".join(sorted({r["backend"] for r in rows})) + " |")
    print("|---|---|---|" + "---|" * len({r["backend"] for r in rows}))
    seen = []
    for r in rows:
        k = (r["entry"].replace("_stats_ex", "_stats"), r["case"], r["branch"])
        if k not in seen:
            seen.append(k)
    for entry, case, branch in seen:
        cells = []
        for backend in sorted({r["backend"] for r in rows}):
            grp = [r for r in rows if r["backend"] == backend and (r["entry"].replace("_stats_ex", "_stats"), r["case"], r["branch"]) == (entry, case, branch)]
            if not grp:
                cells.append("-")
                continue
            w = max(grp, key=lambda r: r["ratio"] / r["bound"])
            cells.append(f"{w['out']} {w['ratio']:.2f} / {w['bound']:.2f}")
        print(f"| `{entry}` | {case} | `{branch}` | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main(sys.argv[1:])
