"""Test helper: the kernels of csrc/k_sched.hip as hipcc builds them for gfx950, from the compiler's resource-usage remarks.

The file is compiled once per process; the three suites that pin its kernel set (test_thresholding, test_prediction_types,
test_device_noise) share the result. The step and selection kernels are identified by the template arguments decoded from their mangled
names, `sched_step_kernelILi<mode>ELi<pred>ELb<guided>ELb<philox>E` and `sched_threshold_kernelILi<pred>ELb<guided>E`.
"""
import functools
import os
import re
import shutil
import subprocess

HIPCC = shutil.which("hipcc") or "/opt/rocm/bin/hipcc"
CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "audio-diffusion_amd", "csrc")

PLAIN, THRESH, MULTISTEP = 0, 1, 2
# (mode, pred, guided, philox): plain and thresholded for the three prediction types, guided or not, with the noise stream or not (24);
# the multistep step for epsilon, guided or not, never with the noise stream (2)
STEP_KERNELS = ({(m, p, g, n) for m in (PLAIN, THRESH) for p in (0, 1, 2) for g in (0, 1) for n in (0, 1)} |
                {(MULTISTEP, 0, g, 0) for g in (0, 1)})
THRESHOLD_KERNELS = {(p, g) for p in (0, 1, 2) for g in (0, 1)}   # (pred, guided)


@functools.lru_cache(maxsize=None)
def scratch_by_kernel():
    """{mangled kernel name: scratch bytes per lane} for every kernel of k_sched.hip."""
    r = subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-c", "k_sched.hip", "-o", os.devnull,
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


def step_kernels(usage):
    """The (mode, pred, guided, philox) of every step kernel; a step kernel under any other name fails the decode."""
    names = [k for k in usage if "sched_step" in k]
    decoded = [re.search(r"sched_step_kernelILi(\d)ELi(\d)ELb([01])ELb([01])EE", k) for k in names]
    assert all(decoded), [k for k, d in zip(names, decoded) if not d]
    out = [tuple(int(v) for v in d.groups()) for d in decoded]
    assert len(set(out)) == len(out)
    return set(out)


def threshold_kernels(usage):
    """The (pred, guided) of every selection kernel."""
    names = [k for k in usage if "sched_threshold" in k]
    decoded = [re.search(r"sched_threshold_kernelILi(\d)ELb([01])EE", k) for k in names]
    assert all(decoded), [k for k, d in zip(names, decoded) if not d]
    out = [tuple(int(v) for v in d.groups()) for d in decoded]
    assert len(set(out)) == len(out)
    return set(out)


def assert_kernel_set_and_no_scratch():
    """Exactly the 26 step and the 6 selection instantiations, the fill and the training prologue, and no kernel of the file uses scratch."""
    usage = scratch_by_kernel()
    assert step_kernels(usage) == STEP_KERNELS, sorted(step_kernels(usage) ^ STEP_KERNELS)
    assert threshold_kernels(usage) == THRESHOLD_KERNELS, sorted(threshold_kernels(usage) ^ THRESHOLD_KERNELS)
    assert any("randn_fill_kernel" in k for k in usage), usage
    assert any("noise_and_velocity_kernel" in k for k in usage), usage
    assert len(usage) >= len(STEP_KERNELS) + len(THRESHOLD_KERNELS) + 2, usage
    assert all(v == 0 for v in usage.values()), {k: v for k, v in usage.items() if v}
