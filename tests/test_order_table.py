"""The launch-order table of the hinted solve launches (dcol_device.hpp hint_fill_window,
dcol_capi.cpp plan_hints) in the headline kernel's launch form: small box x box plans under
DCOL_SMALL_PLAN_LANES=1 (one bucket at 2 lanes per pair; without the variable a small plan
never launches that variant).

tests/order_table_child.py runs in two fresh processes, with the hint and under
DCOL_NO_ORDER_HINT=1.  Six consecutive runs per plan (the order a run uses comes from the
counts of the run two before it, so each buffer parity is rewritten at least twice) and a
captured run replayed three times at new poses: every output must be bitwise equal to the
no-hint process's, no prefilled sentinel may survive (a slot nobody solved), and the runs at
the golden poses must give the goldens' status and iteration counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import golden_files, load_golden

import order_table_child as child

KEYS = ("alpha", "contact", "grad", "iters", "status")


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(with the hint, without): the child's arrays from two fresh processes, run side by side"""
    d = tmp_path_factory.mktemp("order_table")
    procs = []
    for tag, off in (("hint", None), ("nohint", "1")):
        env = {k: v for k, v in os.environ.items()
               if k not in ("DCOL_NO_ORDER_HINT", "DCOL_HINT_WAVES", "DCOL_HINT_FILL_WINDOWS", "DCOL_LIB")}
        env["DCOL_SMALL_PLAN_LANES"] = "1"
        if off:
            env["DCOL_NO_ORDER_HINT"] = off
        f = str(d / f"{tag}.npz")
        procs.append((f, subprocess.Popen([sys.executable, child.__file__, f], env=env)))
    out = []
    for f, p in procs:
        assert p.wait(timeout=300) == 0
        out.append(dict(np.load(f)))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _no_sentinel(r, tag):
    for k in KEYS:
        a = r[f"{tag}.{k}"]
        assert not np.any(a == (child.SENT_I if a.dtype == np.int32 else child.SENT_F)), (tag, k)


def _equal(hint, nohint, tag):
    _no_sentinel(hint, tag)
    _no_sentinel(nohint, tag)
    for k in KEYS:
        np.testing.assert_array_equal(_bits(hint[f"{tag}.{k}"]), _bits(nohint[f"{tag}.{k}"]), err_msg=f"{tag}.{k}")


@pytest.mark.gpu
def test_children_ran_the_throughput_configuration(runs):
    for r in runs:
        assert set(r["forms"].tolist()) == {"buckets"}     # the launch form that carries the hint
        assert r["nbuckets"].tolist() == [1] * len(r["nbuckets"])
        assert r["lanes"].tolist() == [2] * len(r["lanes"])   # the box x box bucket at 2 lanes per pair


@pytest.mark.gpu
@pytest.mark.parametrize("B", child.POLY_B)
def test_six_runs_bitwise_equal_and_every_slot_solved_once(runs, B):
    hint, nohint = runs
    for r in range(child.RUNS):
        _equal(hint, nohint, f"poly{B}.run{r}")
    # golden poses: run 0 (the identity order) and run 5 (the order of a perturbed run's counts)
    d = load_golden([p for p in golden_files() if p.endswith("synthetic_polypoly.npz")][0])
    K = -(-B // len(d["status"]))
    st, it = np.tile(d["status"], K)[:B], np.tile(d["iters"], K)[:B]
    for r in child.GOLDEN_RUNS:
        np.testing.assert_array_equal(hint[f"poly{B}.run{r}.status"], st)
        ok = st == 0
        np.testing.assert_array_equal(hint[f"poly{B}.run{r}.iters"][ok], it[ok])
    # the counts the runs left, and with them the orders, differed from run to run
    if B > 1:
        assert any(np.any(hint[f"poly{B}.run{r}.iters"] != hint[f"poly{B}.run{r + 1}.iters"]) for r in range(4))


@pytest.mark.gpu
def test_captured_run_replayed_at_new_poses(runs):
    hint, nohint = runs
    for r in range(child.REPLAYS):
        _equal(hint, nohint, f"graph.replay{r}")
    _equal(hint, nohint, "graph.after")
    # (the replays solved different poses: their outputs differ from one another)
    assert np.any(hint["graph.replay0.alpha"] != hint["graph.replay1.alpha"])
