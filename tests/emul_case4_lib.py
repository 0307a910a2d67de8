"""Binding of tests/emul_case4/libdcol_emul_case4.so: the x86 builds of the case-4 streamed
instances (csrc/dcol_device.hpp StreamSolver<7, 2>, <8, 2>), and classify() and the plan policy
under DCOL_PLAN_CASE4_STREAM, which the entries of tests/emul_lib.py have no argument for (test
infrastructure of tests/test_case4_stream*.py)."""
import ctypes
import os
import subprocess

import numpy as np

import emul_lib
from emul_lib import BUCKET_COLS, CLASS_KEYS, MAX_BUCKETS, EmulError, descs_of

DIR = os.path.join(emul_lib.HERE, "emul_case4")
ASAN = os.path.join(DIR, "case4_stream_asan")

_i32, _i64, _P = ctypes.c_int32, ctypes.c_int64, ctypes.c_void_p
_SIGNATURES = {
    "dcol_emul_case4_error": (ctypes.c_char_p, []),
    "dcol_emul_case4_batch": (ctypes.c_int, [_P, _i32, _i64] + [_P] * 4 + [ctypes.c_double, _i32, _i32] + [_P] * 6),
    "dcol_emul_case4_classify": (ctypes.c_int, [_P] + [_i32] * 7 + [_P]),
    "dcol_emul_case4_plan": (ctypes.c_int, [_P, _i32, _i32, _i64, _P, _P, _i32, _i32] + [_P] * 6),
}
_lib = None


def load():
    """The library, made current first -- and with it the sanitizer program ASAN (build() has
    made both; make then does nothing)."""
    global _lib
    if _lib is None:
        subprocess.run(["make", "-C", DIR, "-j2", "-s"], check=True)
        _lib = ctypes.CDLL(os.path.join(DIR, "libdcol_emul_case4.so"))
        for name, (res, args) in _SIGNATURES.items():
            getattr(_lib, name).restype, getattr(_lib, name).argtypes = res, args
    return _lib


def _check(rc):
    if rc != 0:
        raise EmulError(rc, load().dcol_emul_case4_error().decode())


def _ptr(a):
    return None if a is None else a.ctypes.data


def solve(d, flags, idx=None, tol=None, max_iter=50, jac=False):
    """The pairs idx (None: all) of a golden-layout table with its pairs through one lane per pair
    of the x86 case-4 streamed solver: (alpha, contact, grad, iters, status); jac=True: its
    Jacobian copies, with jac [B, 4, 12] after grad."""
    descs, n = descs_of(d)
    idx = slice(None) if idx is None else idx
    s1, s2 = np.ascontiguousarray(d["s1"][idx], np.int32), np.ascontiguousarray(d["s2"][idx], np.int32)
    p1, p2 = np.ascontiguousarray(d["pose1"][idx], np.float64), np.ascontiguousarray(d["pose2"][idx], np.float64)
    tol = float(d["tol"]) if tol is None else tol
    B = len(s1)
    al, ct, gr = np.empty(B), np.empty((B, 3)), np.empty((B, 12))
    jc = np.full((B, 4, 12), -7.0) if jac else None
    it, st = np.empty(B, np.int32), np.empty(B, np.int32)
    _check(load().dcol_emul_case4_batch(descs, n, B, _ptr(s1), _ptr(s2), _ptr(p1), _ptr(p2), tol, max_iter, flags,
                                        _ptr(al), _ptr(ct), _ptr(gr), _ptr(jc), _ptr(it), _ptr(st)))
    return (al, ct, gr, it, st) if jc is None else (al, ct, gr, jc, it, st)


def classify(descs, n, a, b, case4=True, part=True, stream=True, case4_stream=True):
    """classify() of shapes a and b of a descriptor array, every parameter given"""
    out = np.zeros(8, np.int32)
    _check(load().dcol_emul_case4_classify(descs, n, a, b, int(case4), int(part), int(stream), int(case4_stream), _ptr(out)))
    return dict(zip(CLASS_KEYS, out.tolist()))


def plan(descs, n, s1, s2, options, simds=256):
    """(buckets, launch form, perm) of the plan of (s1, s2) under the default policy, options as
    dcol_plan_create_ex takes them (DCOL_PLAN_CASE4_STREAM = 32 included)"""
    s1, s2 = np.ascontiguousarray(s1, np.int32), np.ascontiguousarray(s2, np.int32)
    B = len(s1)
    info = np.zeros((MAX_BUCKETS, len(BUCKET_COLS)), np.int32)
    pairs, slot0, rows = (np.zeros(MAX_BUCKETS, np.int64) for _ in range(3))
    head = np.zeros(2, np.int64)
    perm = np.full(max(B, 1), -1, np.int32)
    _check(load().dcol_emul_case4_plan(descs, n, simds, B, _ptr(s1), _ptr(s2), options, MAX_BUCKETS, _ptr(info), _ptr(pairs),
                                       _ptr(slot0), _ptr(rows), _ptr(head), _ptr(perm)))
    buckets = [dict(zip(BUCKET_COLS, info[i].tolist()), pairs=int(pairs[i]), slot0=int(slot0[i]), rows=int(rows[i]))
               for i in range(int(head[0]))]
    return buckets, int(head[1]), perm[:B].copy()
