"""Test helper: the kernels of csrc/k_unipc.hip as hipcc builds them for gfx950, from the compiler's resource-usage remarks
(the method of tests/sched_kernels.py). The step kernels are identified by the template arguments decoded from their mangled names,
`unipc_step_kernelILi<pred>ELb<thresholded>ELb<guided>E`.
"""
import functools
import os
import re
import subprocess

from sched_kernels import CSRC, HIPCC

UNIPC_KERNELS = {(p, t, g) for p in (0, 1, 2) for t in (0, 1) for g in (0, 1)}   # (pred, thresholded, guided)


@functools.lru_cache(maxsize=None)
def scratch_by_kernel():
    """{mangled kernel name: scratch bytes per lane} for every kernel of k_unipc.hip."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "k_unipc.hip", "-o", os.devnull,
                        "-Rpass-analysis=kernel-resource-usage"], cwd=CSRC, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    usage, name = {}, None
    for line in r.stderr.splitlines():
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            name = m.group(1)
        m = re.search(r"ScratchSize \[bytes/lane\]: (\d+)", line)
        if m and name:
            usage[name] = int(m.group(1))
    return usage


def assert_kernel_set_and_no_scratch():
    """Exactly the 12 step instantiations and nothing else, none of them named like a step of k_sched.hip, and no scratch."""
    usage = scratch_by_kernel()
    decoded = [re.search(r"unipc_step_kernelILi(\d)ELb([01])ELb([01])EE", k) for k in usage]
    assert all(decoded), [k for k, d in zip(usage, decoded) if not d]
    got = [tuple(int(v) for v in d.groups()) for d in decoded]
    assert len(got) == len(set(got)) == 12 and set(got) == UNIPC_KERNELS, sorted(set(got) ^ UNIPC_KERNELS)
    assert not any("sched_step" in k or "sched_threshold" in k for k in usage), list(usage)
    assert all(v == 0 for v in usage.values()), {k: v for k, v in usage.items() if v}
