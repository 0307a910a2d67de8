"""What the tests of the contact-point Jacobian share (tests/test_contact_jacobian.py,
tests/test_stream_jacobian_gpu.py): sampled pairs of the golden sets, their restated Jacobians
and their engine shape ids (test infrastructure)."""
import functools

import numpy as np

from conftest import golden_files, load_golden
from contact_jacobian_ref import contact_jacobian, tolerance

GOLD = {p.split("/")[-1][:-4]: p for p in golden_files()}


@functools.lru_cache(maxsize=None)
def golden_set(name):
    return load_golden(GOLD[name])


def sample_pairs(name, n):
    d = golden_set(name)
    ok = np.flatnonzero(d["status"] == 0)
    return d, ok[np.linspace(0, ok.size - 1, n).astype(int)]


def iterate(d, i, tol=None, case4=False):
    from oracle import dcol_oracle as O
    a, b = O.shape_from_table(d, d["s1"][i]), O.shape_from_table(d, d["s2"][i])
    p1, p2 = d["pose1"][i], d["pose2"][i]
    tol = float(d["tol"]) if tol is None else tol
    _, _, x, s, z, _, dims = O.proximity(a, p1[:3], p1[3:], b, p2[:3], p2[3:], tol, case4)
    return O, a, b, x, s, z, np.concatenate([p1, p2]), dims


@functools.lru_cache(maxsize=None)
def restated(name, i, case4=False):
    """(J, cond(H), tolerance) of pair i of a golden set: computed once, shared by the tests"""
    O, a, b, x, s, z, th, dims = iterate(golden_set(name), i, case4=case4)
    J, cond = contact_jacobian(O, a, b, x, s, z, th, dims, case4)
    J.setflags(write=False)
    return J, cond, tolerance(O, a, b, x, s, z, th, dims, J, case4)


_IDS = {}


def registered(engine, d):
    """engine shape ids of a golden table's pairs (registered once per engine and table)"""
    from dcol_amd import spec_from_arrays
    key = (id(engine), id(d))
    if key not in _IDS:
        _IDS[key] = (engine, d, np.array([engine.register(spec_from_arrays(d, k)) for k in range(len(d["type"]))],
                                         dtype=np.int32))
    ids = _IDS[key][2]
    return ids[d["s1"]], ids[d["s2"]]
