"""Binding of tests/emul/libdcol_emul.so: the x86 builds of the device solvers
(csrc/dcol_device.hpp), classify(), the plan policy (csrc/dcol_plan.hpp) and the order hint's
permutation rule -- what the CPU tests check the kernels with (test infrastructure)."""
import ctypes
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
DIR = os.path.join(HERE, "emul")
for _p in (os.path.join(REPO, "dcol-trajectory-optimization_amd"), REPO):
    if _p not in sys.path:
        sys.path.insert(0, _p)

INSTANCES = ("register", "jac", "stream", "stream_jac")
CLASS_KEYS = ("status", "N", "nsoc", "o", "omax", "lpp", "oe", "stream")
BUCKET_COLS = ("kind", "N", "nsoc", "omax", "lpp", "oe", "flags", "code", "stream", "lane")
MAX_BUCKETS = 256
# PlanPolicy's fields in declaration order, with their defaults
POLICY = {"no_ball": 0, "no_box": 0, "no_cone": 0, "small_plan_lanes": 0, "pack_lanes": -1, "small_fanout": 0,
          "latency_per_launch": 0, "no_fanout": 0, "fused_key_order": 0, "side_streams": 3, "side_streams_large": 2}

_i32, _i64, _P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
_SIGNATURES = {
    "dcol_emul_error": (ctypes.c_char_p, []),
    "dcol_emul_max_rows": (ctypes.c_int, []),
    "dcol_emul_batch": (ctypes.c_int, [_i32, _P, _i32, _i64] + [_P] * 4 + [ctypes.c_double, _i32, _i32, _i32] + [_P] * 6),
    "dcol_emul_classify": (ctypes.c_int, [_P, _i32, _i32, _i32, _i32, _i32, _P]),
    "dcol_emul_plan": (ctypes.c_int, [_P, _i32, _i32, _i64, _P, _P, _i32, _P, _i32] + [_P] * 8),
    "dcol_emul_hint_order": (None, [_P, _i32, _P]),
}
_lib = None


class EmulError(Exception):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


def load():
    """The library, made current first -- and with it the sanitizer programs DIR/stream_asan
    and DIR/stream_jac_asan.  build() has made them, or conftest on a fresh checkout: make
    does nothing then, also in a copy of the tree without the objects under DIR/build (the
    Makefile's .SECONDARY).  After an edit of a source or a csrc header, or with a library left
    by an older checkout, it rebuilds what is stale."""
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", DIR, "-j8", "-s"], check=True)
        _lib = ctypes.CDLL(os.path.join(DIR, "libdcol_emul.so"))
        for name, (res, args) in _SIGNATURES.items():
            getattr(_lib, name).restype, getattr(_lib, name).argtypes = res, args
    return _lib


def _check(rc):
    if rc != 0:
        raise EmulError(rc, load().dcol_emul_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


_descs = {}


def descs_of(tab):
    """(descriptor array, count) of an array-form shape table (the golden files' layout).  The
    last few tables' are kept, with the table and the arrays the descriptors point into: use
    them before asking for another table's."""
    from dcol_amd import make_descs, spec_from_arrays
    if id(tab) not in _descs:
        if len(_descs) >= 8:
            del _descs[next(iter(_descs))]
        n = len(tab["type"])
        _descs[id(tab)] = (tab, n) + make_descs([spec_from_arrays(tab, k) for k in range(n)])
    return _descs[id(tab)][2], _descs[id(tab)][1]


def solve(d, flags, idx=None, tol=None, max_iter=50, instance="register", case4=False):
    """The pairs idx (None: all) of a golden-layout table with its pairs (s1, s2, pose1, pose2;
    tol: None takes d["tol"]) through one lane per pair of the x86 solver `instance`: (alpha,
    contact, grad, iters, status), with jac [B, 4, 12] after grad for the Jacobian instances
    (-7 where a run without DCOL_JACOBIAN leaves it unwritten)."""
    descs, n = descs_of(d)
    idx = slice(None) if idx is None else idx
    s1, s2 = np.ascontiguousarray(d["s1"][idx], np.int32), np.ascontiguousarray(d["s2"][idx], np.int32)
    p1, p2 = np.ascontiguousarray(d["pose1"][idx], np.float64), np.ascontiguousarray(d["pose2"][idx], np.float64)
    tol = float(d["tol"]) if tol is None else tol
    B = len(s1)
    al, ct, gr = np.empty(B), np.empty((B, 3)), np.empty((B, 12))
    jc = np.full((B, 4, 12), -7.0) if "jac" in instance else None
    it, st = np.empty(B, np.int32), np.empty(B, np.int32)
    _check(load().dcol_emul_batch(INSTANCES.index(instance), descs, n, B, _ptr(s1), _ptr(s2), _ptr(p1), _ptr(p2), tol,
                                  max_iter, flags, int(case4), _ptr(al), _ptr(ct), _ptr(gr), _ptr(jc), _ptr(it), _ptr(st)))
    return (al, ct, gr, it, st) if jc is None else (al, ct, gr, jc, it, st)


def classify(descs, n, a, b, case4=False, jac=False):
    """classify() of shapes a and b of a descriptor array; jac: as a DCOL_PLAN_JACOBIAN plan does"""
    out = np.zeros(8, np.int32)
    _check(load().dcol_emul_classify(descs, n, a, b, int(case4), int(jac), _ptr(out)))
    return dict(zip(CLASS_KEYS, out.tolist()))


def max_rows():
    return load().dcol_emul_max_rows()


def plan(descs, n, s1, s2, simds, options=0, policy=None):
    """What the plan of (s1, s2) launches on a device with simds SIMDs: buckets (dicts of
    BUCKET_COLS, pairs, slot0, rows), form, streams and launches as the dcol_plan_* getters
    compute them, lanes, small, perm, issue, segs (vid, lpp, block0, slot0, n), fused_blocks.
    policy: the fields of POLICY to set otherwise."""
    s1, s2 = np.ascontiguousarray(s1, np.int32), np.ascontiguousarray(s2, np.int32)
    B = len(s1)
    pol = np.array([{**POLICY, **(policy or {})}[k] for k in POLICY], np.int64)
    info = np.zeros((MAX_BUCKETS, len(BUCKET_COLS)), np.int32)
    pairs, slot0, rows = (np.zeros(MAX_BUCKETS, np.int64) for _ in range(3))
    head = np.zeros(9, np.int64)
    perm = np.full(max(B, 1), -1, np.int32)
    issue = np.zeros(MAX_BUCKETS, np.int32)
    segs = np.zeros((MAX_BUCKETS, 5), np.int64)
    _check(load().dcol_emul_plan(descs, n, simds, B, _ptr(s1), _ptr(s2), options, _ptr(pol), MAX_BUCKETS, _ptr(info),
                                 _ptr(pairs), _ptr(slot0), _ptr(rows), _ptr(head), _ptr(perm), _ptr(issue), _ptr(segs)))
    nb, form, streams, launches, lanes, small, nseg, blocks, nissue = (int(v) for v in head)
    buckets = [dict(zip(BUCKET_COLS, info[i].tolist()), pairs=int(pairs[i]), slot0=int(slot0[i]), rows=int(rows[i]))
               for i in range(nb)]
    return {"buckets": buckets, "form": form, "streams": streams, "launches": launches, "lanes": lanes,
            "small": bool(small), "perm": perm[:B].copy(), "issue": issue[:nissue].tolist(), "segs": segs[:nseg].tolist(),
            "fused_blocks": blocks}


def hint_order(h):
    """order[p] = the slot of a window of hint bytes h that takes position p (-1: none)"""
    h = np.ascontiguousarray(h, np.uint8)
    o = np.full(len(h), -1, np.int32)
    load().dcol_emul_hint_order(_ptr(h), len(h), _ptr(o))
    return o
