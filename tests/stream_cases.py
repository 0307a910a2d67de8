"""What the tests of the streamed-row solver share (tests/test_stream_rows*.py,
tests/test_stream_jacobian*.py): the fixture tests/golden/huge/huge_rows.npz, its references,
a set of descriptors around the row limits, and small helpers (test infrastructure)."""
import functools
import os

import numpy as np

import emul_lib
from conftest import REPO, load_golden
from contact_jacobian_ref import contact_jacobian, tolerance

HUGE = os.path.join(REPO, "tests", "golden", "huge", "huge_rows.npz")
TOO_LARGE, UNSUPPORTED = 5, 2
# the in-process collective stand-in (DCOL_RCCL_LIB; tests/test_native_ranks.py)
FAKE = os.path.join(REPO, "tests", "fake_rccl", "libdcol_fake_rccl.so")


@functools.lru_cache(maxsize=None)
def huge():
    """the fixture: loaded once, shared, never modified"""
    return load_golden(HUGE)


def ok_pairs():
    d = huge()
    return np.flatnonzero((d["expect_status"] == 0) & (d["status"] == 0))


def iterate(d, i):
    """the oracle's solution of pair i of a golden-layout table at the table's tolerance"""
    from oracle import dcol_oracle as O
    a, b = O.shape_from_table(d, d["s1"][i]), O.shape_from_table(d, d["s2"][i])
    p1, p2 = d["pose1"][i], d["pose2"][i]
    _, _, x, s, z, _, dims = O.proximity(a, p1[:3], p1[3:], b, p2[:3], p2[3:], float(d["tol"]))
    return O, a, b, x, s, z, np.concatenate([p1, p2]), dims


def implicit_reference(d, i):
    O, a, b, x, s, z, th, dims = iterate(d, i)
    return O.implicit_gradient(a, b, x, s, z, th, dims)


@functools.lru_cache(maxsize=None)
def restated(i):
    """(J, cond(H), tolerance) of fixture pair i: computed once, shared by the tests, never
    modified"""
    O, a, b, x, s, z, th, dims = iterate(huge(), i)
    J, cond = contact_jacobian(O, a, b, x, s, z, th, dims)
    J.setflags(write=False)
    return J, cond, tolerance(O, a, b, x, s, z, th, dims, J)


def check_against_restatement(idx, jac):
    """The rule of tests/test_stream_jacobian.py's docstring for the fixture pairs idx and their
    kernel results; every figure is printed before the assertion"""
    rows = huge()["rows"]
    worst = (0.0, -1)
    bad = []
    for j, i in enumerate(idx):
        J, cond, tol = restated(int(i))
        sc = max(np.abs(J).max(), 1.0)
        err = np.abs(jac[j] - J).max()
        print(f"pair {int(i)} rows {int(rows[i])}: err {err / sc:.2e} tol {tol / sc:.2e} cond(H) {cond:.1e}")
        if not err <= tol:     # (NaN fails)
            bad.append((int(i), int(rows[i]), float(err / sc), float(tol / sc), float(cond)))
        if np.isfinite(err) and err / tol > worst[0]:
            worst = (float(err / tol), int(i))
    print(f"worst err / tolerance {worst[0]:.3f} at pair {worst[1]}")
    assert not bad, bad


def shape_set():
    """descriptors: polytopes of 6, 34, 122, 123, 512, 513 faces (poly[k]), a capsule, a
    cylinder, a 36-gon, a sphere"""
    from dcol_amd import ShapeSpec, make_descs
    rng = np.random.default_rng(3)
    specs, ids = [], {}

    def poly(k):
        A = np.vstack([np.eye(3), -np.eye(3), rng.normal(size=(k - 6, 3))])
        A /= np.linalg.norm(A, axis=1, keepdims=True)
        return ShapeSpec(0, A=A, b=rng.uniform(0.4, 1.3, k))
    for k in (6, 34, 122, 123, 512, 513):
        ids[k] = len(specs)
        specs.append(poly(k))
    t = np.linspace(0, 2 * np.pi, 36, endpoint=False)
    for name, sp in (("cap", ShapeSpec(3, R=0.3, L=1.0)), ("cyl", ShapeSpec(4, R=0.3, L=1.0)),
                     ("gon", ShapeSpec(5, A=np.stack([np.cos(t), np.sin(t)], 1), b=np.full(36, 0.6), R=0.2)),
                     ("sph", ShapeSpec(1, R=0.5))):
        ids[name] = len(specs)
        specs.append(sp)
    descs, keep = make_descs(specs)
    return descs, keep, len(specs), ids


def plan(descs, n, s1, s2, options=0, simds=256):
    """(buckets, launch form, perm) of the plan of (s1, s2) under the default policy"""
    L = emul_lib.plan(descs, n, s1, s2, simds, options)
    return L["buckets"], L["form"], L["perm"]


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
