"""The plan policy (csrc/dcol_plan.hpp plan_layout: which kernel copy, lane count, launch form
and stream each pair of a batch gets) through its x86 build (tests/emul) -- no GPU.

* tests/plan_layouts.json (tools/record_plan_layouts.py: what the library's plans launched on
  the device, over the grid of tests/plan_cases.py) replays field for field.
* Properties of what the C-ABI does not expose: the permutation, the segments, the issue
  order, the streams.
* The policy assertions of tests/test_plan_buckets.py, which runs them through the C-ABI on
  the device."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import plan_cases
import plan_emul

pytestmark = pytest.mark.skipif(any(os.environ.get(k) for k in plan_cases.POLICY_VARS),
                                reason="plan policy overridden by the environment")

with open(os.path.join(plan_emul.HERE, "plan_layouts.json")) as _f:
    RECORD = json.load(_f)
SIMDS = RECORD["simds"]
CASE4, NO_FUSE = 1, 2


def _id(i):
    p = RECORD["plans"][i]
    return "-".join([p["table"], str(p["B"]), f"o{p['options']}"] + [f"{k}={v}" for k, v in p["env"].items()])


_child = {}


def _replay_in_child(env):
    """the layouts of the record's plans under env, from a fresh process with env set"""
    key = json.dumps(env, sort_keys=True)
    if key not in _child:
        plan_emul.load()   # built before the child needs it
        r = subprocess.run([sys.executable, plan_emul.__file__, os.path.join(plan_emul.HERE, "plan_layouts.json"),
                            json.dumps(env)], env={**os.environ, **env}, check=True, capture_output=True, text=True)
        plans = [p for p in RECORD["plans"] if p["env"] == env]
        _child[key] = dict(zip((id(p) for p in plans), json.loads(r.stdout)))
    return _child[key]


def test_record_covers_the_grid():
    want = [(json.dumps(env, sort_keys=True), t, B, o) for env in ({},) + plan_cases.ENVS for t, B, o in plan_cases.grid(env)]
    got = [(json.dumps(p["env"], sort_keys=True), p["table"], p["B"], p["options"]) for p in RECORD["plans"]]
    assert got == want
    assert len(RECORD["commit"]) == 40 and RECORD["pair_seed"] == plan_cases.PAIR_SEED


@pytest.mark.parametrize("i", range(len(RECORD["plans"])), ids=_id)
def test_recorded_plan_replays(i):
    """Every recorded plan, rebuilt with the recorded SIMD count and policy, field for field"""
    plan = RECORD["plans"][i]
    if any(k in plan["env"] for k in plan_emul.HOST_VARS):   # read once per process by dcol_host.hpp
        got = _replay_in_child(plan["env"])[id(plan)]
    else:
        got = plan_emul.replay(RECORD, plan)
    for k in plan_emul.RECORDED:
        assert got[k] == plan[k], k


# ------------------------------------------------------------------ what the C-ABI does not expose
def _per_pair_cost(b):
    """dcol_plan.hpp bucket_cost / n of a bucket row, operation for operation"""
    _, N, nsoc, omax, _, _, flags, _, n = b
    dense_soc = nsoc > 0 and not (flags & (2 | 4))
    per_pair = 0.0806 * omax + 0.127 * nsoc + 0.0139 * N * N + (0.143 * nsoc if dense_soc else 0.0)
    cost = float(n) * per_pair * (0.5 if nsoc == 0 else 1.0)
    return cost, cost / float(n)


@pytest.mark.parametrize("options", plan_cases.OPTIONS)
@pytest.mark.parametrize("B", [1, 200, 2_000, 150_000])
@pytest.mark.parametrize("name", ["mixed", "random"])
def test_layout_properties(name, B, options):
    s1, s2 = plan_cases.pairs(name, B)
    L = plan_emul.layout(plan_cases.table(name), s1, s2, SIMDS, options)
    bk, perm = L["buckets"], L["perm"].astype(np.int64)
    n = np.array([b[8] for b in bk], np.int64)
    solve = [i for i, b in enumerate(bk) if b[0] == 0]
    assert np.all(n > 0)
    # perm: a permutation of range(B); the buckets' slot ranges tile [0, B) in bucket order
    assert np.array_equal(np.sort(perm), np.arange(B))
    slot0 = np.concatenate([[0], np.cumsum(n)])
    assert slot0[-1] == B
    # ascending within a bucket (the sort is stable)
    inner = np.ones(B, bool)
    inner[slot0[:-1]] = False
    assert np.all(np.diff(perm)[inner[1:]] > 0)
    # pairs with equal (s1, s2) share a bucket
    bucket_of = np.empty(B, np.int64)
    bucket_of[perm] = np.searchsorted(slot0, np.arange(B), side="right") - 1
    key = s1.astype(np.int64) * len(plan_cases.table(name)["type"]) + s2
    order = np.argsort(key, kind="stable")
    same = np.diff(key[order]) == 0
    assert np.all(np.diff(bucket_of[order])[same] == 0)
    # a fused or packed layout: one segment per solve bucket, in non-increasing per-pair cost,
    # block0 the running sum of ceil(n lpp / 64) (one wave per workgroup: dcol_launch.hpp
    # kBlock), fused_blocks its total
    assert (L["launch_form"] == "buckets") == (not L["segs"])
    if options & NO_FUSE:
        assert L["launch_form"] == "buckets"
    if L["segs"]:
        by_slot0 = {int(slot0[i]): i for i in solve}
        seg_bucket = [by_slot0[s[3]] for s in L["segs"]]
        assert sorted(seg_bucket) == solve
        block = 0
        for s, i in zip(L["segs"], seg_bucket):
            assert s[1] == bk[i][4] and s[4] == bk[i][8] and s[0] >= 0 and s[2] == block
            block += -(-s[4] * s[1] // 64)
        assert L["fused_blocks"] == block
        per_pair = [_per_pair_cost(bk[i])[1] for i in seg_bucket]
        assert all(a >= b for a, b in zip(per_pair, per_pair[1:]))
        assert L["num_streams"] == 1 and L["lanes"] == 1
    # issue: empty (as built), or the rejects first (in bucket order) and then the solves in
    # non-increasing cost
    if L["issue"]:
        rejects = [i for i, b in enumerate(bk) if b[0] != 0]
        assert L["issue"][:len(rejects)] == rejects
        tail = L["issue"][len(rejects):]
        assert sorted(tail) == solve
        cost = [_per_pair_cost(bk[i])[0] for i in tail]
        assert all(a >= b for a, b in zip(cost, cost[1:]))
    else:
        assert len(solve) < 2 or L["segs"]
    # streams: rejects on the caller's; every bucket launched by itself on one of the plan's
    # (a fused or packed layout launches no solve bucket by itself)
    assert all(L["bucket_lane"][i] == 0 for i, b in enumerate(bk) if b[0] != 0)
    if not L["segs"]:
        assert all(0 <= l < L["lanes"] for l in L["bucket_lane"])
        assert L["num_streams"] == L["lanes"] <= 4


@pytest.mark.parametrize("where,bad", [(5, 10**6), (0, -1), (199, 64)])
def test_shape_id_out_of_range(where, bad):
    tab = plan_cases.table("prisms")
    s1, s2 = (a.copy() for a in plan_cases.pairs("prisms", 200))
    (s1 if where % 2 else s2)[where] = bad
    with pytest.raises(plan_emul.PlanError) as e:
        plan_emul.layout(tab, s1, s2, SIMDS)
    assert e.value.code == plan_emul.ERR_ARG and str(e.value).endswith(f"at pair {where}")


# ------------------------------------------------------------------ twins of tests/test_plan_buckets.py
def _solves(L):
    return [dict(zip(plan_cases.BUCKET_KEYS, b)) for b in L["buckets"] if b[0] == 0]


def test_benchmark_batch_is_one_padding_free_two_lane_bucket():
    import bench
    s1, s2 = bench.pairs(100_000, 64, 0)[:2]
    L = plan_emul.layout(bench.shape_table(64, 0), s1, s2, SIMDS)
    assert L["buckets"] == [[0, 4, 0, 12, 2, 0, 9, 0, 100_000]] and L["num_launches"] == 1


def test_box_needs_exact_axis_pairs():
    import bench
    tab = bench.shape_table(4, 0)
    tab["A_pool"] = tab["A_pool"].copy()
    tab["A_pool"][6 + 4] = [0.0, -1.0, 1e-12]           # shape 1: face 4 no longer -face 1
    tab["A_pool"][12:18] = tab["A_pool"][12:18][[0, 3, 1, 4, 2, 5]]   # shape 2: pairs interleaved
    s1 = np.array([0, 0, 1, 2, 3], np.int32)
    s2 = np.array([3, 1, 0, 3, 0], np.int32)
    b = {(x["flags"], x["pairs"]) for x in _solves(plan_emul.layout(tab, s1, s2, SIMDS))}
    assert b == {(9, 2), (1, 3)}, b


def _polygon_box(B, seed=0):
    tab = plan_cases.table("mixed")
    rng = np.random.default_rng(seed)
    s1 = rng.choice(np.flatnonzero(tab["type"] == 5), B).astype(np.int32)
    s2 = rng.choice(np.flatnonzero(tab["type"] == 0), B).astype(np.int32)
    return plan_emul.layout(tab, s1, s2, SIMDS)


def test_large_polygon_box_plan_takes_the_row_partitioned_bucket():
    b = _solves(_polygon_box(200_000))
    assert len(b) == 1
    assert (b[0]["N"], b[0]["nsoc"], b[0]["omax"], b[0]["oe"], b[0]["lpp"]) == (6, 1, 11, 5, 1)


@pytest.mark.parametrize("B", [1, 1000])
def test_small_polygon_box_plan_skips_one_lane_buckets(B):
    b = _solves(_polygon_box(B))
    assert b and all(not (x["oe"] > 0 and x["lpp"] < 2) for x in b)
    assert all(x["oe"] == 0 and x["lpp"] >= 4 for x in b)


def test_fanout_width_by_plan_size():
    import bench
    tab = plan_cases.table("mixed")
    s1, s2 = bench.mixed_pairs(tab, 1_000_000, seed=3)[:2]
    big = plan_emul.layout(tab, s1, s2, SIMDS)
    assert len(_solves(big)) > 4 and big["num_streams"] == 3 and big["launch_form"] == "buckets"
    mid = plan_emul.layout(tab, s1[:150_000], s2[:150_000], SIMDS)
    assert len(_solves(mid)) > 4 and mid["launch_form"] == "packed" and mid["num_streams"] == 1 and mid["num_launches"] == 1
    key = lambda b: (b["N"], b["nsoc"], b["omax"], b["lpp"], b["oe"], b["flags"])  # noqa: E731
    assert {key(b) for b in _solves(mid)} <= {key(b) for b in _solves(big)}
    small = plan_emul.layout(tab, s1[:2000], s2[:2000], SIMDS, NO_FUSE)
    assert len(_solves(small)) > 4 and small["num_streams"] == 4 and small["launch_form"] == "buckets"
    one = plan_emul.layout(tab, s1[:2000], s2[:2000], SIMDS)
    assert one["launch_form"] in ("fused", "packed") and one["num_streams"] == 1 and one["num_launches"] == 1
    s1, s2 = bench.pairs(100_000, 64, 0)[:2]
    p1 = plan_emul.layout(bench.shape_table(64, 0), s1, s2, SIMDS)
    assert p1["num_streams"] == 1 and p1["launch_form"] == "buckets"
