"""Binding of the x86 build of the plan policy (tests/emul_plan: csrc/dcol_plan.hpp plan_layout)
for tests/test_plan_layout.py (test infrastructure).

As a program -- `python plan_emul.py RECORD ENV_JSON` -- it replays the plans RECORD holds for
one environment setting and prints their layouts as JSON: the variables dcol_host.hpp reads
itself (DCOL_NO_PART) are read once per process, so such a replay needs a fresh one."""
import ctypes
import json
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (os.path.join(REPO, "dcol-trajectory-optimization_amd"), REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import plan_cases  # noqa: E402

ERR_ARG = -1
FORMS = ("buckets", "fused", "packed")
MAX_BUCKETS = 256
# PlanPolicy's fields in declaration order, with their defaults
POLICY = {"no_ball": 0, "no_box": 0, "no_cone": 0, "small_plan_lanes": 0, "pack_lanes": -1, "small_fanout": 0,
          "latency_per_launch": 0, "no_fanout": 0, "fused_key_order": 0, "side_streams": 3, "side_streams_large": 2}
# the variables dcol_host.hpp reads from the environment itself
HOST_VARS = ("DCOL_NO_PART", "DCOL_LPP", "DCOL_SPLIT")


class PlanError(Exception):
    def __init__(self, code, message):
        super().__init__(message)
        self.code = code


def policy_of(env):
    """PlanPolicy::from_env of an environment (the variables HOST_VARS aside)"""
    p = dict(POLICY)
    for var, field in (("DCOL_NO_BALL", "no_ball"), ("DCOL_NO_BOX", "no_box"), ("DCOL_NO_CONE", "no_cone"),
                       ("DCOL_SMALL_FANOUT", "small_fanout"), ("DCOL_LATENCY_PER_LAUNCH", "latency_per_launch"),
                       ("DCOL_NO_FANOUT", "no_fanout")):
        p[field] = int(var in env)
    for var, field in (("DCOL_SMALL_PLAN_LANES", "small_plan_lanes"), ("DCOL_PACK_LANES", "pack_lanes"),
                       ("DCOL_SIDE_STREAMS", "side_streams"), ("DCOL_SIDE_STREAMS_LARGE", "side_streams_large")):
        if var in env:
            p[field] = int(env[var])
    if "DCOL_FUSED_ORDER" in env:
        p["fused_key_order"] = int(int(env["DCOL_FUSED_ORDER"]) == 0)
    return p


_lib = None


def load():
    global _lib
    if _lib is None:
        d = os.path.join(HERE, "emul_plan")
        # (built by build(); a fresh checkout that ran no build() makes it here, like conftest's libraries)
        subprocess.run(["make", "-C", d, "-s"], check=True)
        _lib = ctypes.CDLL(os.path.join(d, "libdcol_plan_emul.so"))
        _lib.dcol_emul_plan.restype = ctypes.c_int
    return _lib


_descs = {}


def descs_of(tab):
    """(descriptor array, count) of an array-form shape table, kept alive per table"""
    from dcol_amd import make_descs, spec_from_arrays
    if id(tab) not in _descs:
        n = len(tab["type"])
        _descs[id(tab)] = (tab, n) + make_descs([spec_from_arrays(tab, k) for k in range(n)])
    return _descs[id(tab)][2], _descs[id(tab)][1]


def layout(tab, s1, s2, simds, options=0, policy=None):
    """What the plan of (s1, s2) over tab launches on a device with simds SIMDs: buckets (rows
    of plan_cases.BUCKET_KEYS), bucket_lane, launch_form / num_streams / num_launches as the
    C-ABI getters give them, lanes, small, perm, issue, segs (vid, lpp, block0, slot0, n),
    fused_blocks"""
    lib = load()
    descs, n = descs_of(tab)
    s1 = np.ascontiguousarray(s1, np.int32)
    s2 = np.ascontiguousarray(s2, np.int32)
    B = len(s1)
    pol = np.array([{**POLICY, **(policy or {})}[k] for k in POLICY], np.int64)
    info = np.zeros((MAX_BUCKETS, 8), np.int32)
    pairs = np.zeros(MAX_BUCKETS, np.int64)
    lane = np.zeros(MAX_BUCKETS, np.int32)
    head = np.zeros(9, np.int64)
    perm = np.full(max(B, 1), -1, np.int32)
    issue = np.zeros(MAX_BUCKETS, np.int32)
    segs = np.zeros((MAX_BUCKETS, 5), np.int64)
    err = ctypes.create_string_buffer(256)
    P = ctypes.c_void_p
    rc = lib.dcol_emul_plan(descs, ctypes.c_int32(n), ctypes.c_int32(simds), ctypes.c_int64(B), P(s1.ctypes.data),
                            P(s2.ctypes.data), ctypes.c_int32(options), P(pol.ctypes.data), ctypes.c_int32(MAX_BUCKETS),
                            P(info.ctypes.data), P(pairs.ctypes.data), P(lane.ctypes.data), P(head.ctypes.data),
                            P(perm.ctypes.data), P(issue.ctypes.data), P(segs.ctypes.data), err, ctypes.c_int32(len(err)))
    if rc != 0:
        raise PlanError(rc, err.value.decode())
    nb, form, streams, launches, lanes, small, nseg, blocks, nissue = (int(v) for v in head)
    return {"buckets": [info[i].tolist() + [int(pairs[i])] for i in range(nb)], "bucket_lane": lane[:nb].tolist(),
            "launch_form": FORMS[form], "num_streams": streams, "num_launches": launches, "lanes": lanes,
            "small": bool(small), "perm": perm[:B].copy(), "issue": issue[:nissue].tolist(),
            "segs": segs[:nseg].tolist(), "fused_blocks": blocks}


RECORDED = ("buckets", "num_launches", "num_streams", "launch_form")


def replay(rec, plan):
    """a recorded plan rebuilt through the emulator: its RECORDED fields"""
    s1, s2 = plan_cases.pairs(plan["table"], plan["B"], rec["pair_seed"])
    got = layout(plan_cases.table(plan["table"]), s1, s2, rec["simds"], plan["options"], policy_of(plan["env"]))
    return {k: got[k] for k in RECORDED}


if __name__ == "__main__":
    with open(sys.argv[1]) as f:
        record = json.load(f)
    want = json.loads(sys.argv[2])
    assert all(os.environ.get(k) == v for k, v in want.items())
    print(json.dumps([replay(record, p) for p in record["plans"] if p["env"] == want]))
