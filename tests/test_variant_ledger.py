"""The variant ledger: every compiled copy of the solver (csrc/variants.py, per launch form:
tests/variant_ledger.py) is launched by a case of tests/variant_cases.py or stands in
variant_ledger.UNREACHABLE with a reason checked here -- no GPU: the cases' plans come from the
x86 build of the plan policy, one fresh process per environment (DCOL_LPP, DCOL_NO_PART and
DCOL_SPLIT are read once per process).  tests/test_variant_parity_gpu.py runs the same cases on
the device and holds the device's layouts to these."""
import os
import shutil

import numpy as np
import pytest

import variant_cases as VC
import variant_ledger as VL

import plan_cases  # noqa: E402

pytestmark = pytest.mark.skipif(any(os.environ.get(k) for k in plan_cases.POLICY_VARS + VC.HOST_VARS),
                                reason="plan policy overridden by the environment")

_plans = {}


def plans():
    """{case id: variant_cases.evaluate(case)} of every case"""
    if not _plans:
        for env, todo in VC.env_groups():
            for c, r in zip(todo, VC.evaluate_in_child(env, todo)):
                _plans[c["id"]] = r
    return _plans


def launched(skip=None):
    return {tuple(x) for i, r in plans().items() if i != skip for x in r["copies"]}


def universe(v=None):
    return {(f, i) for f in VL.FORMS for i in range(len(VL.compiled(f, v)))}


def test_lists_match_the_generated_include():
    """compiled() against csrc/dcol_variants.inc, macro by macro: the counts, and for the fused and
    packed switches the case ids"""
    import re
    with open(os.path.join(os.path.dirname(VL.VARIANTS_PY), "dcol_variants.inc")) as f:
        text = f.read()
    rows = {}
    for name, body in re.findall(r"#define (DCOL_\w+)\(X\) \\\n((?:    X\(.*\) \\\n)*)", text):
        rows[name] = [tuple(int(t) for t in m.split(",")) for m in re.findall(r"X\(([^)]*)\)", body)]
    per_variant = sum(len(rows[f"DCOL_{k}VARIANTS"]) for k in ("", "FULL_", "BOX_", "BOX_FD_", "FULL_CONE_", "BALL_", "CONE_",
                                                               "PART_", "SPLIT_"))
    assert len(VL.compiled("buckets")) == per_variant
    assert [(i,) + tuple(c)[:5] + ((c.oe,) if c.oe else ()) for i, c in enumerate(VL.compiled("fused"))] == \
        rows["DCOL_FUSED_VARIANTS"] + rows["DCOL_FUSED_PART_VARIANTS"]
    assert [(i,) + tuple(c)[:6] for i, c in enumerate(VL.compiled("packed"))] == rows["DCOL_PACKED_VARIANTS"]
    assert [tuple(c)[:4] + (c.wps, 0) for c in VL.compiled("jac")] == rows["DCOL_JAC_VARIANTS"]
    assert VL.compiled("server") == VL.compiled("fused")


@pytest.mark.parametrize("g", range(len(VC.env_groups())), ids=[VC.group_id(e) for e, _ in VC.env_groups()])
def test_cases_plan_as_recorded(g):
    """Every case of the group: the plan has the case's form, every bucket has a copy to launch,
    and the restated fused_vid / packed_vid give the case ids plan_layout put in the segments"""
    env, todo = VC.env_groups()[g]
    for c in todo:
        r = plans()[c["id"]]
        assert not r["unlaunchable"], (c, r["unlaunchable"])
        assert r["form"] == ("fused" if c["form"] == "server" else c["form"]), (c, r["form"])
        assert all(i >= 0 for _, i in r["copies"]), c
        if r["form"] in ("fused", "packed"):
            assert r["vids"] and all(a == b for a, b in r["vids"]), (c, r["vids"])
            assert len(r["vids"]) <= 64   # kMaxFusedSegs
        if c["form"] == "server":   # each pair's one-pair plan takes the case its bucket has in the fused plan
            assert len(c["groups"]) == 2 and sorted(a for a, _ in r["vids"]) == sorted(r["server_vids"]), (c, r)
        solve = [b for b in r["buckets"] if b["kind"] == "solve"]
        assert len(solve) == len(r["buckets"])
        if c["form"] != "server":
            assert all(b["pairs"] >= VC.PER_BUCKET // 2 for b in solve) and sum(n for _, _, n in c["groups"]) % VC.PER_BUCKET == 0


def test_every_copy_is_launched_or_listed():
    dead = VL.unreachable()
    got = launched()
    assert not (got & dead), sorted(got & dead)
    missing = universe() - got - dead
    assert not missing, [(f, tuple(VL.compiled(f)[i])) for f, i in sorted(missing)]
    counts = {f: (sum(1 for x in got if x[0] == f), len(VL.compiled(f))) for f in VL.FORMS}
    print("launched / compiled per form:", counts, "unreachable:", len(dead))


def test_every_case_is_needed():
    """each case launches a copy no other case does: deleting any one leaves a copy unlaunched"""
    owners = {}
    for i, r in plans().items():
        for x in r["copies"]:
            owners.setdefault(tuple(x), []).append(i)
    sole = {v[0] for v in owners.values() if len(v) == 1}
    assert sole == set(plans()), sorted(set(plans()) - sole)


def test_a_new_config_line_fails_the_ledger(tmp_path):
    """a scratch copy of variants.py with one more CONFIG entry compiles a copy no case launches"""
    src = tmp_path / "variants.py"
    shutil.copy(VL.VARIANTS_PY, src)
    text = src.read_text().replace("    (4, 0, 16): [(4, 2)],", "    (4, 0, 16): [(4, 2), (8, 1)],")
    assert text != src.read_text()
    src.write_text(text)
    v = VL.load_variants(str(src))
    now = {(f, tuple(c)) for f in VL.FORMS for c in VL.compiled(f, v)}
    have = {(f, tuple(VL.compiled(f)[i])) for f, i in launched() | VL.unreachable()}
    assert ("buckets", (4, 0, 16, 8, 0, 0, 1)) in now - have and ("buckets", (4, 0, 16, 8, 1, 0, 1)) in now - have


def test_unreachable_reasons():
    """Every UNREACHABLE entry: no bucket of well-posed pairs launches it (variant_ledger.reachable
    over the brute-force classification sweep); and nothing else is beyond such buckets."""
    sweep = [tuple(r) for r in VC.sweep_classes()] + [tuple(r) for r in VC.sweep_classes({"DCOL_NO_PART": "1"})]
    can = VL.reachable(sweep)
    dead = VL.unreachable("classify")
    assert not (can & dead), [(f, tuple(VL.compiled(f)[i])) for f, i in sorted(can & dead)]
    assert launched() | VL.unreachable("oracle") <= can
    # the shapes the issue names: no pair of well-posed shapes has these classes at all
    classes = {r[5:9] for r in sweep}
    assert (7, 2, 4, 0) not in classes and (8, 2, 4, 0) not in classes and (6, 2, 2, 0) not in classes


def test_unreachable_for_want_of_a_reference():
    """The "oracle" entries are the copies of (4, 0, 4), whose pairs are polytope pairs of at most
    four faces together.  With fewer than four, at none of 300 poses (drawn as the cases' are) does
    the C oracle find a proper optimum: a non-zero status, alpha below ALPHA_MIN (the degenerate
    alpha = 0), or an answer without one Newton iteration (an unbounded problem its first
    convergence test let through).  With exactly four -- four rows in four unknowns -- the oracle's
    own iteration count is decided by rounding (variant_ledger.UNREACHABLE_ORACLE): over the poses
    it solves, the count is 0 at some and not at others, with nothing else about the pair changed."""
    from oracle import c_oracle
    every = {(f, i) for f in VL.FORMS for i, c in enumerate(VL.compiled(f)) if (c.N, c.nsoc, c.omax) == (4, 0, 4)}
    assert VL.unreachable("oracle") == every
    tab = VC.table()
    poly = np.flatnonzero(tab["type"] == VC.POLYTOPE)
    zero = some = 0
    for a in poly:
        for b in poly:
            rows = tab["nh"][a] + tab["nh"][b]
            if rows > 4:
                continue
            case = {"groups": [[int(a), int(b), 300]], "form": "buckets", "options": 0}
            ref = c_oracle.run_batch(tab, *VC.pairs_of(case, 0), want_grad=False)
            good = (ref["status"] == 0) & (ref["alpha"] >= VC.ALPHA_MIN)
            if rows < 4:
                assert not np.any(good & (ref["iters"] >= 1)), (a, b)
            else:
                zero += int(np.sum(good & (ref["iters"] == 0)))
                some += int(np.sum(good & (ref["iters"] > 0)))
    assert zero > 0 and some > 0, (zero, some)


def test_seeds_follow_the_rule():
    """Each case's pose seed is variant_cases.pick_seed's -- the oracle solves every pair at it and
    at no smaller one -- and a case redraws exactly when it holds an unbounded shape; the redrawn
    cases' recorded poses are what pairs_of draws"""
    unb = VC.unbounded()
    for c in VC.cases():
        assert c.get("redraw", False) == any(a in unb or b in unb for a, b, _ in c["groups"]), c["id"]
        if c["seed"] or c.get("redraw") or c["form"] == "jac":
            assert VC.pick_seed(c) == c["seed"], c["id"]   # (the others: test_oracle_solves_every_pair, at seed 0)
        if c.get("redraw"):
            rec = VC.pairs_of(c)
            now = VC.pairs_of({k: v for k, v in c.items() if k != "id"})
            assert all(np.array_equal(x, y) for x, y in zip(rec, now)), c["id"]


def test_oracle_solves_every_pair():
    """No pair is excused: the oracle returns status 0 on every pair of every case -- the C oracle,
    for the DCOL_PLAN_CASE4 cases the NumPy oracle's extension, whose recorded reference
    (tests/golden/variants/case4_ref.npz) is its own output.  Half-spaces, slabs and wedges appear
    only in cases this holds for, like every other shape."""
    from oracle import dcol_oracle as O
    unb = VC.unbounded()
    used = False
    for c in VC.cases():
        s1, s2, p1, p2 = VC.pairs_of(c)
        used = used or bool(set(s1.tolist() + s2.tolist()) & unb)
        if c["options"] & VC.CASE4:
            ref = VC.reference(c)
            now = O.run_batch(VC.table(), s1, s2, p1, p2, want_grad=False, case4=True)
            assert np.array_equal(now["alpha"], ref["alpha"]) and np.array_equal(now["iters"], ref["iters"]), c["id"]
        else:
            ref = VC.oracle(c)
        assert np.all(ref["status"] == 0), (c["id"], c["groups"])
        assert c["seed"] == 0 or c.get("redraw") or c["form"] == "jac" or not VC.solves(c, 0)
        if c.get("redraw"):
            assert ref["alpha"].min() >= VC.ALPHA_MIN, c["id"]
    assert used


def test_jacobian_cases_are_well_conditioned():
    """The filter of tests/test_contact_jacobian.py (a pair may miss its tolerance only where
    cond(H) > COND_MAX) leaves out at most 10 % of any Jacobian copy's pairs, on the restatement
    alone"""
    from oracle import dcol_oracle as O
    from contact_jacobian_ref import contact_jacobian
    COND_MAX = 1e10   # tests/test_contact_jacobian.py
    tab = VC.table()
    for c in VC.cases():
        if c["form"] != "jac":
            continue
        s1, s2, p1, p2 = VC.pairs_of(c)
        c4 = bool(c["options"] & VC.CASE4)
        bad = 0
        for i in range(len(s1)):
            a, b = O.shape_from_table(tab, int(s1[i])), O.shape_from_table(tab, int(s2[i]))
            _, _, x, s, z, _, dims = O.proximity(a, p1[i, :3], p1[i, 3:], b, p2[i, :3], p2[i, 3:], 1e-6, c4)
            bad += contact_jacobian(O, a, b, x, s, z, np.concatenate([p1[i], p2[i]]), dims, c4)[1] > COND_MAX
        assert bad <= 0.1 * len(s1), (c["id"], bad)
