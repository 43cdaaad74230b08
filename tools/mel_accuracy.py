"""Turns the `MEL_SWEEP` lines of tests/test_mel_sweep.py (`pytest -s`) into the tables of profiles/mel_accuracy.md.

    python tools/mel_accuracy.py emu.log hip.log > tables.md

One line per case and setting with its branch and, per backend, the kernel's error (g over the tensor, h per column) and its ratio to
max(e_oracle, 4u); then the share of pixels near a rounding edge per image case.
"""
import re
import sys

KV = re.compile(r"(\w+)=(\S+)")


def main(paths):
    figs, shares, other = [], [], []
    for p in paths:
        for line in open(p, errors="replace"):
            at = line.find("MEL_SWEEP ")
            if at < 0:
                continue
            d = dict(KV.findall(line[at:]))
            (figs if "g_ratio" in d else shares if "near_edge_share" in d else other).append((d, line[at:].strip()))
    backends = sorted({d["backend"] for d, _ in figs})
    print("| case | setting | output | branch (" + " / ".join(backends) + ") | " +
          " | ".join(f"{b}: g, ratio | {b}: h, ratio" for b in backends) + " | bound | ceiling |")
    print("|---|---|---|---|" + "---|---|" * len(backends) + "---|---|")
    keys = list(dict.fromkeys((d["case"], d.get("setting", "-"), d["out"]) for d, _ in figs))
    for k in keys:
        rows = {d["backend"]: d for d, _ in figs if (d["case"], d.get("setting", "-"), d["out"]) == k}
        any_d = next(iter(rows.values()))
        cells = []
        for b in backends:
            d = rows.get(b)
            cells += [f"{d['g_kernel']}, {d['g_ratio']}", f"{d['h_kernel']}, {d['h_ratio']}"] if d else ["-", "-"]
        branch = " / ".join(dict.fromkeys(rows[b]["branch"] for b in backends if b in rows))
        print(f"| {k[0]} | {k[1]} | {k[2]} | `{branch}` | " + " | ".join(cells) + f" | {any_d['bound']} | {any_d.get('ceiling', '-')} |")
    worst = max(figs, key=lambda f: max(float(f[0]["g_ratio"]), float(f[0]["h_ratio"])) / float(f[0]["bound"]))
    print(f"\n{len(figs)} comparisons; nearest to its bound: {worst[1]}\n")
    print("| image case | precision | pixels | " + " | ".join(f"within 1e-3 of a rounding edge ({b})" for b in backends) + " |")
    print("|---|---|---|" + "---|" * len(backends))
    for case, dtype, pixels in dict.fromkeys((d["case"], d["dtype"], d["pixels"]) for d, _ in shares):
        cell = {d["backend"]: d["near_edge_share"] for d, _ in shares if (d["case"], d["dtype"], d["pixels"]) == (case, dtype, pixels)}
        print(f"| {case} | {dtype} | {pixels} | " + " | ".join(cell.get(b, "-") for b in backends) + " |")
    print()
    for _, line in other:
        print("    " + line)


if __name__ == "__main__":
    main(sys.argv[1:])
