"""Test helper: selects which build of the kernel sources a test drives.

"emu" -> tests/emu/libadm_emu.so : the SAME kernel sources compiled by g++ against the fiber emulator
          (tests/emu/hip_emu.h); runs in the GPU-less container; tensors live on the CPU.
"hip" -> audio-diffusion_amd/audiodiffusion/libadm_hip.so : the product library on a real MI355X (-m gpu).
"""
import ctypes
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EMU_LIB = os.path.join(ROOT, "tests", "emu", "libadm_emu.so")
BUILD = os.path.join(ROOT, "audio-diffusion_amd", "csrc", "build.sh")

_built = False


def ensure_emu_built():
    global _built
    if not _built and os.environ.get("ADM_EMU_NOBUILD") != "1":    # spawned rank workers: the parent has built it already
        subprocess.run(["bash", BUILD, "emu"], check=True, capture_output=True)
        os.environ["ADM_EMU_NOBUILD"] = "1"                         # inherited by multiprocessing children
    _built = True
    return EMU_LIB


def select(backend):
    """Loads the library for `backend` and returns the torch device tensors must live on."""
    from audiodiffusion import _native
    if backend == "emu":
        _native.load(ensure_emu_built())
        return torch.device("cpu")
    assert torch.cuda.is_available(), "gpu tests need a MI355X"
    _native.load()  # product library; raises loudly if missing
    assert _native.is_device_build()
    return torch.device("cuda:0")


def spy_sample_loop(monkeypatch):
    """Observes the pipeline through what it hands to the loop's one entry point. -> a list that gains one dict per `adm_sample_loop*` call:
    "symbol" (the entry point's name) and, for adm_sample_loop_ex, every field of the adm_sample_loop_args it received (a pointer field is
    None when null)."""
    from audiodiffusion import _native
    real, calls = _native.lib(), []

    def record(handle, args, stream):
        fields = {name: getattr(args, name) for name, _ in args._fields_}   # (a null POINTER(...) field reads as a false pointer object)
        calls.append({"symbol": "adm_sample_loop_ex", **{k: (v if not isinstance(v, ctypes._Pointer) or v else None) for k, v in fields.items()}})
        return real.adm_sample_loop_ex(handle, args, stream)

    class Spy:
        def __getattr__(self, name):
            if name == "adm_sample_loop_ex":
                return record
            if name.startswith("adm_sample_loop"):
                calls.append({"symbol": name})
            return getattr(real, name)
    monkeypatch.setattr(_native, "lib", lambda: Spy())
    return calls


BACKENDS = [pytest.param("emu", id="emu"), pytest.param("hip", id="hip", marks=pytest.mark.gpu)]
