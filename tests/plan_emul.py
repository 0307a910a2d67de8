"""The x86 build of the plan policy (tests/emul_lib.plan: csrc/dcol_plan.hpp plan_layout) in the
form tests/plan_layouts.json records, for tests/test_plan_layout.py (test infrastructure).

As a program -- `python plan_emul.py RECORD ENV_JSON` -- it replays the plans RECORD holds for
one environment setting and prints their layouts as JSON: the variables dcol_host.hpp reads
itself (DCOL_NO_PART) are read once per process, so such a replay needs a fresh one."""
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for _p in (os.path.join(REPO, "dcol-trajectory-optimization_amd"), REPO, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import emul_lib  # noqa: E402
import plan_cases  # noqa: E402

POLICY, PlanError, load = emul_lib.POLICY, emul_lib.EmulError, emul_lib.load
ERR_ARG = -1
FORMS = ("buckets", "fused", "packed")
# the variables dcol_host.hpp reads from the environment itself
HOST_VARS = ("DCOL_NO_PART", "DCOL_LPP", "DCOL_SPLIT")


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


def layout(tab, s1, s2, simds, options=0, policy=None):
    """What the plan of (s1, s2) over tab launches on a device with simds SIMDs: buckets (rows
    of plan_cases.BUCKET_KEYS: as dcol_plan_bucket gives them, a reject bucket's kernel fields
    and a solve bucket's code zero), bucket_lane, launch_form / num_streams / num_launches as
    the C-ABI getters give them, lanes, small, perm, issue, segs (vid, lpp, block0, slot0, n),
    fused_blocks"""
    L = emul_lib.plan(*emul_lib.descs_of(tab), s1, s2, simds, options, policy)
    rows = []
    for b in L["buckets"]:
        solve = b["kind"] == 0
        rows.append([b["kind"]] + [b[k] if solve else 0 for k in ("N", "nsoc", "omax", "lpp", "oe", "flags")]
                    + [0 if solve else b["code"], b["pairs"]])
    return {"buckets": rows, "bucket_lane": [b["lane"] for b in L["buckets"]], "launch_form": FORMS[L["form"]],
            "num_streams": L["streams"], "num_launches": L["launches"],
            **{k: L[k] for k in ("lanes", "small", "perm", "issue", "segs", "fused_blocks")}}


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
