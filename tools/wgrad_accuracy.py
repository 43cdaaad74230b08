"""Turns the `WGRAD_SWEEP` lines of tests/test_wgrad_sweep.py (`pytest -s`) into the tables of profiles/wgrad_accuracy.md.

    python tools/wgrad_accuracy.py emu.log hip.log > tables.md

Per backend and kernel family (the kernel of `adm_conv2d_wgrad` that ran, the reduce kernel of `adm_wgrad_reduce`, the small-channel entry and
output): the number of comparisons, the comparison with the largest ratio e_kernel / max(e_torch_fp32, 4u) and the one nearest to its bound;
then one line per case with its branch and its figure on each backend.
"""
import re
import sys

LINE = re.compile(r"WGRAD_SWEEP backend=(\S+) case=(\S+) branch=(\S+) entry=(\S+) out=(\S+) n=(\d+) e_kernel=(\S+) e_torch_fp32=(\S+) "
                  r"ratio=(\S+) bound=(\S+)")
KERNELS = {"k310": "conv_wgrad_kernel<3,1>", "k320": "conv_wgrad_kernel<3,2>", "k110": "conv_wgrad_kernel<1,1>",
           "k1300": "conv_wgrad_pf_kernel<3,false>", "k1301": "conv_wgrad_pf_kernel<3,true>", "k1100": "conv_wgrad_pf_kernel<1,false>",
           "k1101": "conv_wgrad_pf_kernel<1,true>", "k2304": "conv_wgrad_sp_kernel", "k2308": "conv_wgrad_sp8_kernel"}


def family(entry, out, branch):
    head = branch.split("-")[0]
    if entry == "adm_conv2d_wgrad":
        return KERNELS.get(head, head)
    if entry == "adm_wgrad_reduce":
        return "wgrad_reduce9_kernel" if head == "reduce9" else "wgrad_reduce_kernel"
    return f"{entry} {head} {out}"


def main(paths):
    rows = []
    for p in paths:
        for m in LINE.finditer(open(p, errors="replace").read()):
            b, case, branch, entry, out, n, ek, et, ratio, bound = m.groups()
            rows.append(dict(backend=b, case=case, branch=branch, entry=entry, out=out, n=int(n), ek=float(ek), et=float(et),
                             ratio=float(ratio), bound=float(bound), family=family(entry, out, branch)))
    backends = sorted({r["backend"] for r in rows})
    for backend in backends:
        mine = [r for r in rows if r["backend"] == backend]
        print(f"\n## {backend}: worst comparison per kernel ({len(mine)} comparisons)\n")
        print("| kernel | comparisons | worst ratio | its bound M(n) | case | branch | e_kernel | e_torch_fp32 | nearest to its bound |")
        print("|---|---|---|---|---|---|---|---|---|")
        keys = []
        for r in mine:
            if r["family"] not in keys:
                keys.append(r["family"])
        for fam in keys:
            grp = [r for r in mine if r["family"] == fam]
            w = max(grp, key=lambda r: r["ratio"])
            near = max(grp, key=lambda r: r["ratio"] / r["bound"])
            print(f"| `{fam}` | {len(grp)} | {w['ratio']:.2f} | {w['bound']:.2f} | {w['case']} | `{w['branch']}` | {w['ek']:.3e} | "
                  f"{w['et']:.3e} | {near['ratio']:.2f} / {near['bound']:.2f} ({near['case']}) |")
    print("\n## Every case: its branch and its worst comparison (ratio / bound), per backend\n")
    print("| entry | case | branch | " + " | ".join(backends) + " |")
    print("|---|---|---|" + "---|" * len(backends))
    seen = []
    for r in rows:
        k = (r["entry"], r["case"], r["branch"])
        if k not in seen:
            seen.append(k)
    for entry, case, branch in seen:
        cells = []
        for backend in backends:
            grp = [r for r in rows if r["backend"] == backend and (r["entry"], r["case"], r["branch"]) == (entry, case, branch)]
            if not grp:
                cells.append("-")
                continue
            w = max(grp, key=lambda r: r["ratio"] / r["bound"])
            cells.append(f"{w['out']} {w['ratio']:.2f} / {w['bound']:.2f}")
        print(f"| `{entry}` | {case} | `{branch}` | " + " | ".join(cells) + " |")


if __name__ == "__main__":
    main(sys.argv[1:])
