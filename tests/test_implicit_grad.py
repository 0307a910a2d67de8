"""DCOL_GRAD_IMPLICIT: the implicit-function derivative of the returned PDIP iterate through
the method's own normal matrix (no reference counterpart; north star "implicit-function
d alpha / d pose solve reusing the factorisation").

The reference's gradient (proximity_gradient.py:50-88) is the envelope form z'(dG x - dh)
evaluated by forward differences at the iterate PDIP returns (mu < 1e-6).  The implicit mode
differentiates the KKT system at that same iterate, linearised with the NT scaling the
method itself uses (ds = -W^2 dz): d alpha_j = -z'(dG_j v) - (G v)'W^-2 (dG_j x - dh_j),
v = (G'W^-2 G)^-1 e3.  Both tend to the derivative of the optimal value as mu -> 0; at the
default tolerance the implicit one is the closer of the two (measured below against central
differences of alpha* solved to mu < 1e-11).

CPU: the oracle's restatement (oracle/dcol_oracle.py implicit_gradient) against that true
derivative and against the emulated kernel (tests/emul).  GPU: the HIP kernel
against the oracle's restatement at the same iterate.
"""
import numpy as np
import pytest

import emul_lib
from conftest import golden_files, load_golden

GOLD = {p.split("/")[-1][:-4]: p for p in golden_files()}


def _pairs(name, n):
    d = load_golden(GOLD[name])
    ok = np.flatnonzero(d["status"] == 0)
    return d, ok[np.linspace(0, ok.size - 1, n).astype(int)]


def _oracle(d, i, tol=None):
    from oracle import dcol_oracle as O
    a, b = O.shape_from_table(d, d["s1"][i]), O.shape_from_table(d, d["s2"][i])
    p1, p2 = d["pose1"][i], d["pose2"][i]
    tol = float(d["tol"]) if tol is None else tol
    alpha, _, x, s, z, it, dims = O.proximity(a, p1[:3], p1[3:], b, p2[:3], p2[3:], tol)
    th = np.concatenate([p1, p2])
    return O, a, b, th, x, s, z, dims


def _true_derivative(O, a, b, th, step=1e-5):
    g = np.empty(12)
    for j in range(12):
        tp, tm = th.copy(), th.copy()
        tp[j] += step
        tm[j] -= step
        ap = O.proximity(a, tp[:3], tp[3:6], b, tp[6:9], tp[9:], 1e-11)[0]
        am = O.proximity(a, tm[:3], tm[3:6], b, tm[6:9], tm[9:], 1e-11)[0]
        g[j] = (ap - am) / (2 * step)
    return g


@pytest.mark.parametrize("name", ["scene_quad", "synthetic_mixed", "synthetic_polypoly"])
def test_oracle_implicit_closer_to_true_derivative_than_reference(name):
    """At the reference tolerance the implicit derivative is nearer the derivative of the
    optimal value than the reference's own gradient (the golden FD values): in the median
    and in the worst case of a sample (pair by pair either can be the closer one)."""
    d, idx = _pairs(name, 12)
    e_imp, e_ref = [], []
    for i in idx:
        O, a, b, th, x, s, z, dims = _oracle(d, i)
        g_imp = O.implicit_gradient(a, b, x, s, z, th, dims)
        g_true = _true_derivative(O, a, b, th)
        sc = max(np.abs(g_true).max(), 1.0)
        e_imp.append(np.abs(g_imp - g_true).max() / sc)
        e_ref.append(np.abs(d["grad"][i] - g_true).max() / sc)
    e_imp, e_ref = np.array(e_imp), np.array(e_ref)
    assert np.median(e_imp) <= np.median(e_ref), (e_imp, e_ref)
    assert e_imp.max() <= e_ref.max() + 1e-6, (e_imp, e_ref)
    assert e_imp.max() < 1e-3


@pytest.mark.parametrize("name", ["scene_quad", "scene_cone", "synthetic_mixed", "edge_cases"])
def test_emulated_kernel_implicit_matches_oracle(name):
    """The kernel's implicit mode (x86 build, LPP 1) against the oracle's restatement at the
    same pairs: within 1e-6 of max(|g|, 1) (the iterates agree to rounding; the restatement's
    dG / dh are central differences)."""
    d, idx = _pairs(name, 40)
    al, ct, gr, it, st = emul_lib.solve(d, 16, idx)
    assert np.all(st == 0)
    for j, i in enumerate(idx):
        O, a, b, th, x, s, z, dims = _oracle(d, i)
        ref = O.implicit_gradient(a, b, x, s, z, th, dims)
        assert np.abs(gr[j] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), (i, gr[j], ref)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_quad", "scene_cone", "scene_piano", "synthetic_mixed", "edge_cases",
                                  "large_polytopes"])
def test_gpu_implicit_matches_oracle(engine, name):
    """HIP kernel, grad='implicit', against the oracle's restatement (1e-6 of max(|g|, 1)),
    and within 5e-3 of max(|g|, 1) of the reference's own FD gradient where alpha* is
    differentiable (a different evaluation of the same derivative: see the module
    docstring; measured <= 2e-3, the reference's being the farther from the true one)."""
    from test_gpu_parity import register
    d, idx = _pairs(name, 48)
    s1, s2 = register(engine, d)
    res = engine.solve_host(s1[idx], s2[idx], d["pose1"][idx], d["pose2"][idx], tol=float(d["tol"]), grad="implicit")
    assert np.all(res.status == 0)
    for j, i in enumerate(idx):
        O, a, b, th, x, s, z, dims = _oracle(d, i)
        ref = O.implicit_gradient(a, b, x, s, z, th, dims)
        sc = max(np.abs(ref).max(), 1.0)
        assert np.abs(res.grad[j] - ref).max() <= 1e-6 * sc, (i, res.grad[j], ref)
        if d["alpha"][i] > 1e-2:    # alpha* ~ 0 (coincident centres in edge_cases) is not differentiable
            assert np.abs(res.grad[j] - d["grad"][i]).max() <= 5e-3 * sc
