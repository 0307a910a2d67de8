"""Shared test configuration.

Markers: ``gpu`` tests need an MI355X (run on the GPU box: ``pytest -m gpu``); everything
else runs on the CPU-only build container.  Paths: the repo root (for ``oracle``) and the
package root ``dcol-trajectory-optimization_amd`` (for ``dcol_amd``, ``proximity``,
``primitives``, laid out like the reference's repository root).
"""
import glob
import os
import sys

import numpy as np
import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(REPO, "dcol-trajectory-optimization_amd")
GOLDEN = os.path.join(REPO, "tests", "golden")
for p in (PKG, REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

# parity tolerances (north star: alpha 1e-6 rel, gradient 1e-5 rel; SURVEY.md §7: the
# reference's own FD gradient is noisy at ~1e-7 of ||g||, so the gradient check is relative
# to ||g||_inf (floor 0.01), and alpha gets an absolute floor for alpha ~ 0)
ALPHA_RTOL = 1e-6
ALPHA_ATOL = 1e-12
GRAD_TOL = 1e-5


def pytest_configure(config):
    config.addinivalue_line("markers", "gpu: needs an AMD Instinct MI355X (HIP) device")
    config.addinivalue_line("markers", "slow: long-running")


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN, "*.npz")))


def load_golden(path):
    return dict(np.load(path, allow_pickle=False))


def alpha_close(a, ref):
    return np.abs(a - ref) <= ALPHA_RTOL * np.abs(ref) + ALPHA_ATOL


GRAD_FLOOR = 1e-2   # below ||g||_inf = 0.01 the bound is absolute (1e-7): the reference's own
                    # FD noise on analytic zeros is ~3e-8


def grad_close(g, ref):
    """Gradient within 1e-5 of ||ref||_inf (north star: 1e-5 rel), floored at ||g|| = 0.01."""
    return np.abs(g - ref).max(axis=-1) <= GRAD_TOL * np.maximum(np.abs(ref).max(axis=-1), GRAD_FLOOR)


def gpu_available():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


@pytest.fixture(scope="session")
def engine():
    if not gpu_available():
        pytest.skip("no GPU")
    from dcol_amd import Engine
    return Engine(device=0)


def _ensure_built():
    """Build lib/libdcol.so, lib/libdcol_altro.so and dcol_amd/_fastpair.so in-tree if a fresh
    checkout lacks them (hipcc cross-compiles for gfx950 without a GPU)."""
    import subprocess
    libs = [os.path.join(PKG, "lib", n) for n in ("libdcol.so", "libdcol_altro.so")]
    libs.append(os.path.join(PKG, "dcol_amd", "_fastpair.so"))
    if not all(os.path.exists(p) for p in libs):
        subprocess.run(["make", "-C", os.path.join(PKG, "csrc"), "-j8", "-s"], check=True)
    # the x86 build of the device solver (the emulated-kernel tests; no test skips for want of it)
    if not os.path.exists(os.path.join(REPO, "tests", "emul", "libdcol_emul.so")):
        subprocess.run(["make", "-C", os.path.join(REPO, "tests", "emul"), "-j8", "-s"], check=True)


_ensure_built()
