"""Turns the `CONV_SWEEP` lines of tests/test_conv_sweep.py (`pytest -s --durations=0`) into the tables of profiles/conv_accuracy.md.

    python tools/conv_accuracy.py emu.log hip.log > tables.md

Per kernel family (the first word of a case's branch) and backend: the worst ratio of g (whole tensor) and of h (per (sample, cout) plane) to
max(e_torch_fp32, 4u), the bound they stand under, the case that came nearest to its bound, and the room of the worst g under the older tests'
1e-4; then every case with the branch it ran; then the wall time of the file's tests per backend (the `--durations` lines).
"""
import re
import sys

KV = re.compile(r"(\w+)=(\S+)")
DUR = re.compile(r"^\s*([0-9.]+)s (call|setup|teardown)\s+(\S+)")


def family(branch):
    b = branch.split(":")[-1]
    for name in ("generic-split", "pf3-split", "cout-split", "cout-wide", "cin-wide", "generic", "pf3", "pf1", "cout", "cin"):
        if b.startswith(name + "-"):
            return name + ("+gn-finish" if b.endswith("-gnfinish") else "")
    return b


def main(paths):
    figs, seconds = [], {}
    for p in paths:
        for line in open(p, errors="replace"):
            m = DUR.match(line)
            if m and "test_conv_sweep.py" in m.group(3):
                backend = "hip" if "hip" in m.group(3).rsplit("[", 1)[-1] else "emu"
                seconds[backend] = seconds.get(backend, 0.0) + float(m.group(1))
            at = line.find("CONV_SWEEP ")
            if at < 0:
                continue
            d = dict(KV.findall(line[at:]))
            if "fig" in d:
                figs.append(d)
    backends = sorted({d["backend"] for d in figs})
    fams = list(dict.fromkeys(family(d["branch"]) for d in figs))
    print("| kernel family | backend | comparisons | worst g ratio | worst h ratio | bound there | nearest to its bound (case, figure, ratio / bound) | "
          "worst g | room under 1e-4 |")
    print("|---|---|---|---|---|---|---|---|---|")
    for f in fams:
        for b in backends:
            rows = [d for d in figs if family(d["branch"]) == f and d["backend"] == b and d["out"] == "out"]
            if not rows:
                continue
            wg = max((d for d in rows if d["fig"] == "g"), key=lambda d: float(d["ratio"]))
            wh = max((d for d in rows if d["fig"] == "h"), key=lambda d: float(d["ratio"]))
            near = max(rows, key=lambda d: float(d["ratio"]) / float(d["bound"]))
            eg = max(float(d["e_kernel"]) for d in rows if d["fig"] == "g")
            print(f"| {f} | {b} | {len(rows)} | {wg['ratio']} | {wh['ratio']} | {near['bound']} | {near['case']}, {near['fig']}, "
                  f"{float(near['ratio']) / float(near['bound']):.2f} | {eg:.2e} | {1e-4 / eg:.0f}x |")
    other = [d for d in figs if d["out"] != "out"]
    if other:
        print("\n| other output | backend | comparisons | worst ratio | bound there | case |")
        print("|---|---|---|---|---|---|")
        for o in dict.fromkeys(d["out"] for d in other):
            for b in backends:
                rows = [d for d in other if d["out"] == o and d["backend"] == b]
                if rows:
                    w = max(rows, key=lambda d: float(d["ratio"]) / float(d["bound"]))
                    print(f"| {o} | {b} | {len(rows)} | {w['ratio']} | {w['bound']} | {w['case']} |")
    print("\n| case | branch | " + " | ".join(f"{b}: g ratio | {b}: h ratio" for b in backends) + " | bound |")
    print("|---|---|" + "---|---|" * len(backends) + "---|")
    for case in dict.fromkeys(d["case"] for d in figs if d["out"] == "out"):
        rows = [d for d in figs if d["case"] == case and d["out"] == "out" and not d["branch"].endswith("-gnfinish")]
        cells = []
        for b in backends:
            for fig in ("g", "h"):
                cells.append(next((d["ratio"] for d in rows if d["backend"] == b and d["fig"] == fig), "-"))
        print(f"| {case} | `{rows[0]['branch']}` | " + " | ".join(cells) + f" | {rows[0]['bound']} |")
    print()
    for b in backends:
        n = len([d for d in figs if d["backend"] == b])
        print(f"{b}: {n} comparisons, {seconds.get(b, 0.0):.1f} s of test time (sum of the --durations lines)")


if __name__ == "__main__":
    main(sys.argv[1:])
