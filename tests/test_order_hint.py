"""The window-local order hint of the solve launches (dcol_device.hpp hint_position /
hint_wave_slot, dcol_capi.cpp plan_hints): it only changes which lane group of which wave
solves which pair.

CPU: the permutation rule in its scalar form (tests/emul), on random bytes.
GPU: tests/order_hint_child.py runs the same scenarios in two fresh processes, with the
hint and under DCOL_NO_ORDER_HINT=1; every output of every run must be bitwise equal, no
prefilled sentinel may survive (a slot nobody solved), and the runs at the golden poses must
give the goldens' status and iteration counts."""
import os
import subprocess
import sys

import numpy as np
import pytest

import emul_lib
from conftest import golden_files, load_golden

import order_hint_child as child

KEYS = ("alpha", "contact", "grad", "iters", "status")


# ------------------------------------------------------------------ CPU: the rule
@pytest.fixture(scope="module")
def hint_order():
    return emul_lib.hint_order


PPW = (64, 32, 16, 8)   # pairs per wave at 1, 2, 4, 8 lanes per pair
LENGTHS = sorted({1, 31, 32, 33, 255, 256} | {ww * p for ww in (4, 8, 16) for p in PPW} | {p - 1 for p in PPW})


def _byte_arrays(n, rng):
    yield "random", rng.integers(0, 256, n)
    yield "counts", rng.integers(4, 13, n)              # what a run leaves: a few distinct counts
    yield "extremes", rng.choice([0, 255], n)
    yield "clamped", rng.integers(60, 70, n)             # around the clamp at 63
    yield "ascending", np.minimum(np.arange(n), 255)


@pytest.mark.parametrize("n", LENGTHS)
def test_rule_is_stable_descending_permutation(hint_order, n):
    rng = np.random.default_rng(n)
    for name, h in _byte_arrays(n, rng):
        o = hint_order(h)
        assert sorted(o.tolist()) == list(range(n)), name       # a permutation of the window's slots
        key = np.minimum(np.asarray(h, np.int64), 63)
        ko = key[o]
        assert np.all(np.diff(ko) <= 0), name                   # descending
        same = np.diff(ko) == 0
        assert np.all(np.diff(o)[same] > 0), name               # stable: equal keys keep slot order
        np.testing.assert_array_equal(o, np.argsort(-key, kind="stable"), err_msg=name)
        # the waves' shares (rank r takes positions [r * ppw, (r + 1) * ppw)): together every
        # slot exactly once, no wave faster than a later one's slowest pair
        for ppw in PPW:
            shares = [o[a:a + ppw] for a in range(0, n, ppw)]
            assert sorted(np.concatenate(shares).tolist()) == list(range(n))
            assert all(key[a].min() >= key[b].max() for a, b in zip(shares, shares[1:]))


@pytest.mark.parametrize("n", LENGTHS)
@pytest.mark.parametrize("value", [0, 3, 63, 64, 255])
def test_rule_is_identity_for_constant_bytes(hint_order, n, value):
    np.testing.assert_array_equal(hint_order(np.full(n, value)), np.arange(n))


# ------------------------------------------------------------------ GPU
@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """(with the hint, without): the child's arrays from two fresh processes, run side by side"""
    d = tmp_path_factory.mktemp("order_hint")
    procs = []
    for tag, off in (("hint", None), ("nohint", "1")):
        env = {k: v for k, v in os.environ.items() if k not in ("DCOL_NO_ORDER_HINT", "DCOL_HINT_WAVES")}
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


CASES = [f"poly{B}" for B in child.POLY_B] + ["mixed"]


@pytest.mark.gpu
def test_children_ran_hinted_launch_forms(runs):
    for r in runs:
        assert set(r["forms"].tolist()) == {"buckets"}    # the launch form that carries the hint
        assert len(r["lanes"]) >= 2                       # several lanes-per-pair settings ran


@pytest.mark.gpu
@pytest.mark.parametrize("case", CASES)
def test_bitwise_equal_and_every_slot_solved_once(runs, case):
    hint, nohint = runs
    for r in range(child.RUNS):
        tag = f"{case}.run{r}"
        _no_sentinel(hint, tag)
        _no_sentinel(nohint, tag)
        for k in KEYS:
            np.testing.assert_array_equal(_bits(hint[f"{tag}.{k}"]), _bits(nohint[f"{tag}.{k}"]), err_msg=f"{tag}.{k}")
    # the orders differed from run to run: the counts the runs left did
    if case not in ("poly1",):
        assert any(np.any(hint[f"{case}.run{r}.iters"] != hint[f"{case}.run{r + 1}.iters"]) for r in range(3))
    # golden poses (first run: zero hints; last run: the hints of a perturbed run)
    name = "synthetic_mixed.npz" if case == "mixed" else "synthetic_polypoly.npz"
    d = load_golden([p for p in golden_files() if p.endswith(name)][0])
    B = len(hint[f"{case}.run0.status"])
    K = -(-B // len(d["status"]))
    st, it = np.tile(d["status"], K)[:B], np.tile(d["iters"], K)[:B]
    for r in (0, child.RUNS - 1):
        np.testing.assert_array_equal(hint[f"{case}.run{r}.status"], st)
        ok = st == 0
        np.testing.assert_array_equal(hint[f"{case}.run{r}.iters"][ok], it[ok])


@pytest.mark.gpu
def test_max_iter_3_then_uncapped(runs):
    hint, nohint = runs
    _no_sentinel(hint, "cap3")
    assert np.all(hint["cap3.status"] == 1) and np.all(hint["cap3.iters"] == 3)
    assert np.all(np.isnan(hint["cap3.alpha"])) and np.all(np.isnan(hint["cap3.grad"]))
    _no_sentinel(hint, "aftercap")
    for k in KEYS:
        np.testing.assert_array_equal(_bits(hint[f"aftercap.{k}"]), _bits(nohint[f"aftercap.{k}"]), err_msg=k)
        np.testing.assert_array_equal(_bits(hint[f"aftercap.{k}"]), _bits(nohint[f"poly1000.run0.{k}"]), err_msg=k)


@pytest.mark.gpu
def test_two_streams_equal_their_serial_results(runs):
    hint, nohint = runs
    for rnd in range(3):
        for j in (0, 1):
            tag = f"two.round{rnd}.stream{j}"
            _no_sentinel(hint, tag)
            for k in KEYS:   # stream j ran the poses of the serial case's run j
                np.testing.assert_array_equal(_bits(hint[f"{tag}.{k}"]), _bits(nohint[f"poly1000.run{j}.{k}"]),
                                              err_msg=f"{tag}.{k}")
