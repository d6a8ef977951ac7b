"""CPU checks of the boundary: the HIP library builds for gfx950, loads, and exports every symbol include/chmc.h
declares (no compute call is made: there is no GPU here); the package refuses to run without it."""
import ctypes
import os
import re
import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header_symbols():
    txt = open(os.path.join(ROOT, "include", "chmc.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    return sorted(set(re.findall(r"\b(chmc_[a-z_0-9]+)\s*\(", txt)))


def test_header_matches_python_binding():
    from manifold_mcmc_for_diffusions_amd import _lib
    assert header_symbols() == sorted(n for n, _, _ in _lib.SYMBOLS)


def test_hip_library_builds_loads_and_exports_every_symbol():
    from manifold_mcmc_for_diffusions_amd import _lib
    so = _lib.build()
    assert os.path.exists(so)
    cdll = ctypes.CDLL(so)
    for name in header_symbols():
        assert hasattr(cdll, name), name
    cdll.chmc_backend.restype = ctypes.c_char_p
    assert cdll.chmc_backend() == b"hip:gfx950"
    # gfx950 code object inside
    blob = open(so, "rb").read()
    assert b"gfx950" in blob


def test_library_exports_nothing_the_header_does_not_declare():
    """Every exported chmc_* symbol is part of the declared C ABI (no undeclared debugging entry points)."""
    import subprocess
    from manifold_mcmc_for_diffusions_amd import _lib
    so = _lib.build()
    out = subprocess.check_output(["nm", "-D", "--defined-only", so], text=True)
    exported = sorted({ln.split()[-1] for ln in out.splitlines() if ln.split() and ln.split()[-1].startswith("chmc_")})
    assert exported == header_symbols()


def test_no_fallback_without_gpu():
    """Creating a context must fail loudly when no HIP device is visible (this container has none)."""
    import torch
    if torch.cuda.is_available():
        pytest.skip("a GPU is visible")
    from manifold_mcmc_for_diffusions_amd import _lib
    from manifold_mcmc_for_diffusions_amd.context import ChmcContext
    saved = _lib._LIB
    _lib._LIB = None  # make sure the real library is what gets loaded
    try:
        with pytest.raises(RuntimeError, match="HIP|device"):
            ChmcContext("fhn", 0.2, 4, 2, np.zeros(6), sigma=0.1)
    finally:
        _lib._LIB = saved


def test_sequencing_is_one_text_for_both_builds():
    """csrc/chmc_api.inc (sequencing, C ABI) is compiled identically by the library and by the host emulation of tests/emu/:
    it has no CHMC_WAVE_KERNELS outside the RCCL block that closes it and names no __global__ kernel (k_*); every choice of
    a kernel per pass lives in csrc/chmc_passes.inc under one #ifdef."""
    csrc = os.path.join(ROOT, "manifold_mcmc_for_diffusions_amd", "csrc")

    def code(name):
        txt = open(os.path.join(csrc, name)).read()
        return re.sub(r"//[^\n]*", "", re.sub(r"/\*.*?\*/", "", txt, flags=re.S))

    api = code("chmc_api.inc")
    sequencing, rccl_opens, _ = api.rpartition("#ifdef CHMC_WAVE_KERNELS\n#include <dlfcn.h>\n#include <rccl/rccl.h>")
    assert rccl_opens, "the RCCL block no longer closes chmc_api.inc: check the whole file instead"
    assert "CHMC_WAVE_KERNELS" not in sequencing
    assert re.findall(r"\bk_[a-z0-9_]+", api) == []
    assert '#include "chmc_passes.inc"' in sequencing
    assert len(re.findall(r"^\s*#\s*if.*\bCHMC_WAVE_KERNELS\b", code("chmc_passes.inc"), flags=re.M)) == 1
    assert len(re.findall(r"^\s*#\s*ifdef\s+CHMC_WAVE_KERNELS\b", code("chmc_passes.inc"), flags=re.M)) == 1


def test_product_does_not_import_the_oracle():
    pkg = os.path.join(ROOT, "manifold_mcmc_for_diffusions_amd")
    for dirpath, _, files in os.walk(pkg):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".inc")):
                txt = open(os.path.join(dirpath, f)).read()
                assert "oracle" not in txt, f"{f} mentions the oracle"
