"""What the tests of the case-4 streamed kernels share (tests/test_case4_stream.py,
tests/test_case4_stream_gpu.py): the fixture tests/golden/case4_huge/case4_rows.npz
(tests/golden/gen_case4_rows.py), its references and small helpers (test infrastructure)."""
import functools
import os

import numpy as np

from conftest import REPO, load_golden
from contact_jacobian_ref import contact_jacobian, tolerance

FIXTURE = os.path.join(REPO, "tests", "golden", "case4_huge", "case4_rows.npz")
OK, MAXITER, TOO_LARGE = 0, 1, 5
FD, ENVELOPE, CONTACT, IMPLICIT, JACOBIAN = 1, 2, 4, 16, 64
PLAN_CASE4, PLAN_JACOBIAN, PLAN_JACOBIAN_STREAM, PLAN_CASE4_STREAM = 1, 8, 16, 32
REGISTER_ROWS = 32      # the case-4 register kernels' largest bucket
COND_EXCUSE = 1e10      # a pair may miss its Jacobian tolerance only above this cond(H) ...
EXCUSED_SHARE = 0.10    # ... and at most this share of the pairs


@functools.lru_cache(maxsize=None)
def fixture():
    """the fixture: loaded once, shared, never modified"""
    return load_golden(FIXTURE)


def solvable():
    return np.flatnonzero(fixture()["expect_status"] == 0)


def streamed():
    """the pairs the streamed kernels take: above the register buckets, up to the cap"""
    d = fixture()
    return np.flatnonzero((d["expect_status"] == 0) & (d["rows"] > REGISTER_ROWS))


def iterate(i):
    """the oracle's solution of fixture pair i at the fixture's tolerance"""
    from oracle import dcol_oracle as O
    d = fixture()
    a, b = O.shape_from_table(d, d["s1"][i]), O.shape_from_table(d, d["s2"][i])
    p1, p2 = d["pose1"][i], d["pose2"][i]
    _, _, x, s, z, _, dims = O.proximity(a, p1[:3], p1[3:], b, p2[:3], p2[3:], float(d["tol"]), case4=True)
    return O, a, b, x, s, z, np.concatenate([p1, p2]), dims


@functools.lru_cache(maxsize=None)
def implicit_reference(i):
    O, a, b, x, s, z, th, dims = iterate(i)
    g = O.implicit_gradient(a, b, x, s, z, th, dims, case4=True)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def restated(i):
    """(J, cond(H), tolerance) of fixture pair i by the NumPy restatement: computed once, shared
    by the tests, never modified"""
    O, a, b, x, s, z, th, dims = iterate(i)
    J, cond = contact_jacobian(O, a, b, x, s, z, th, dims, case4=True)
    J.setflags(write=False)
    return J, cond, tolerance(O, a, b, x, s, z, th, dims, J, case4=True)


def check_against_restatement(idx, jac):
    """The rule of tests/test_stream_jacobian.py with the excuse the case-4 fixture needs: the
    error is within contact_jacobian_ref.tolerance(...); a pair may miss it only where
    cond(H) > 1e10, and at most 10 % of the pairs may be so excused.  Every figure is printed
    before the assertions."""
    rows = fixture()["rows"]
    bad, excused = [], []
    for j, i in enumerate(idx):
        J, cond, tol = restated(int(i))
        sc = max(np.abs(J).max(), 1.0)
        err = np.abs(jac[j] - J).max()
        print(f"pair {int(i)} rows {int(rows[i])}: err {err / sc:.2e} tol {tol / sc:.2e} cond(H) {cond:.1e}")
        if not err <= tol:     # (NaN fails)
            (excused if cond > COND_EXCUSE else bad).append((int(i), int(rows[i]), float(err / sc), float(tol / sc), float(cond)))
    print(f"excused (cond(H) > {COND_EXCUSE:g}): {excused}")
    assert not bad, bad
    assert len(excused) <= EXCUSED_SHARE * len(idx), excused


def check_solution(d, idx, al, ct, gr, it, st):
    """status, iteration counts and the project tolerances against the fixture's oracle values on
    the solvable pairs idx (gr None: no gradient to compare)"""
    from conftest import alpha_close, grad_close
    np.testing.assert_array_equal(st, d["expect_status"][idx])
    np.testing.assert_array_equal(it, d["iters"][idx])
    assert np.all(alpha_close(al, d["alpha"][idx]))
    assert np.all(np.abs(ct - d["contact"][idx]) <= 1e-6 * np.maximum(np.abs(d["contact"][idx]), 1.0))
    if gr is not None:
        assert np.all(grad_close(gr, d["grad"][idx]))


def check_implicit(idx, gr):
    rows = fixture()["rows"]
    for j, i in enumerate(idx):
        ref = implicit_reference(int(i))
        assert np.abs(gr[j] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), (int(i), int(rows[i]), gr[j], ref)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def register(engine, d):
    from dcol_amd import spec_from_arrays
    ids = np.array([engine.register(spec_from_arrays(d, k)) for k in range(len(d["type"]))], dtype=np.int32)
    return ids[d["s1"]], ids[d["s2"]]


def soa(x):
    import torch
    return torch.from_numpy(np.ascontiguousarray(x.T)).cuda()
