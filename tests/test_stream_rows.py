"""Pairs above 128 orthant rows: the streamed-row solver (csrc/dcol_device.hpp StreamSolver),
its classification and plan policy, on the CPU.

Fixture tests/golden/huge/huge_rows.npz (tests/golden/gen_huge_rows.py): 152 pairs of 129 to
1,025 rows run through the reference -- every streamed (N, NSOC), the row totals at which the
slot loop changes shape (129, 192 / 193, 256 / 257, 1,012, 1,024), the pairs one row past the
cap and a few case-4 pairs.  The x86 build (tests/emul, one lane walking every row)
is held to the project tolerances of DESIGN.md section 4: status and iteration counts equal,
alpha 1e-6 relative, contact 1e-6 max(|x|, 1), gradient 1e-5 max(|g|_inf, 0.01); the implicit
mode to 1e-6 max(|g|, 1) of the oracle's restatement (tests/test_implicit_grad.py's bound)."""
import os
import re
import subprocess

import numpy as np
import pytest

import emul_lib
from conftest import REPO, alpha_close, grad_close, load_golden
from stream_cases import HUGE, TOO_LARGE, UNSUPPORTED, implicit_reference, plan, shape_set


@pytest.fixture(scope="module")
def huge():
    return load_golden(HUGE)


def stream_emul(d, idx, flags, tol=None, max_iter=50):
    return emul_lib.solve(d, flags, idx, tol, max_iter, instance="stream")


@pytest.fixture(scope="module")
def fd_run(huge):
    """the x86 streamed solver on the whole fixture, FD gradient + contact (shared, not modified)"""
    return stream_emul(huge, np.arange(len(huge["s1"])), 1 | 4)


# ---------------------------------------------------------------- 1. the checker
def test_fixture_contents(huge):
    d = huge
    ok = d["expect_status"] == 0
    rows = d["rows"]
    assert 120 <= len(rows) <= 160 and os.path.getsize(HUGE) <= 300 * 1024
    assert {129, 192, 193, 256, 257, 1012, 1024} <= set(rows[ok].tolist())
    assert rows[ok].min() >= 129 and rows[ok].max() == 1024
    assert set(rows[d["expect_status"] == TOO_LARGE].tolist()) == {1025}
    assert (d["expect_status"] == UNSUPPORTED).sum() >= 4
    assert int(d["replaced"]) <= 0.05 * int(d["draws"])
    # every streamed (N, NSOC) occurs, in both orders
    t1, t2 = d["type"][d["s1"]], d["type"][d["s2"]]
    for a, b in ((0, 0), (0, 1), (0, 2), (3, 0), (4, 0), (5, 0), (5, 1), (5, 2)):
        assert np.any(ok & (t1 == a) & (t2 == b)) and np.any(ok & (t1 == b) & (t2 == a)), (a, b)
    assert np.any(np.abs(d["r_offset"][d["type"] == 0]).sum(axis=1) > 0)


def test_oracle_reproduces_fixture(huge):
    """The NumPy oracle has no row limit: it reproduces the reference bit for bit here as on
    the <= 128-row fixtures (tests/test_oracle_golden.py), so it can stand in for it."""
    from oracle import dcol_oracle as O
    d = huge
    out = O.run_batch(d, d["s1"], d["s2"], d["pose1"], d["pose2"], float(d["tol"]), True)
    np.testing.assert_array_equal(out["status"], d["status"])
    ok = d["status"] == 0
    np.testing.assert_array_equal(out["iters"][ok], d["iters"][ok])
    np.testing.assert_array_equal(out["alpha"][ok], d["alpha"][ok])
    np.testing.assert_array_equal(out["contact"][ok], d["contact"][ok])
    np.testing.assert_array_equal(out["grad"][ok], d["grad"][ok])


# ---------------------------------------------------------------- 2. the x86 streamed solver
def test_stream_solver_matches_reference_fd(huge, fd_run):
    d = huge
    al, ct, gr, it, st = fd_run
    np.testing.assert_array_equal(st, d["expect_status"])
    ok = d["expect_status"] == 0
    np.testing.assert_array_equal(it[ok], d["iters"][ok])
    assert np.all(alpha_close(al[ok], d["alpha"][ok]))
    assert np.all(np.abs(ct[ok] - d["contact"][ok]) <= 1e-6 * np.maximum(np.abs(d["contact"][ok]), 1.0))
    assert np.all(grad_close(gr[ok], d["grad"][ok]))
    assert np.all(np.isnan(al[~ok])) and np.all(np.isnan(gr[~ok]))


def test_stream_solver_envelope(huge, fd_run):
    """Closed form of the derivative the reference takes by forward differences: the bound
    the envelope tests of the <= 128-row fixtures use (tests/test_emul_golden.py)."""
    d = huge
    idx = np.arange(len(d["s1"]))
    al, ct, gr, it, st = stream_emul(d, idx, 2 | 4)
    ok = d["expect_status"] == 0
    np.testing.assert_array_equal(st, d["expect_status"])
    np.testing.assert_array_equal(it[ok], d["iters"][ok])
    np.testing.assert_array_equal(al[ok], fd_run[0][ok])       # the gradient mode does not touch the solve
    assert np.all(grad_close(gr[ok], d["grad"][ok]))


def test_stream_solver_implicit(huge):
    d = huge
    idx = np.flatnonzero(d["expect_status"] == 0)
    al, ct, gr, it, st = stream_emul(d, idx, 16)
    assert np.all(st == 0)
    for j, i in enumerate(idx):
        ref = implicit_reference(d, i)
        assert np.abs(gr[j] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), (i, int(d["rows"][i]), gr[j], ref)


def test_stream_solver_max_iter(huge):
    d = huge
    idx = np.flatnonzero(d["expect_status"] == 0)
    al, ct, gr, it, st = stream_emul(d, idx, 1 | 4, max_iter=3)
    assert np.all(st == 1) and np.all(it == 3)
    assert np.all(np.isnan(al)) and np.all(np.isnan(gr)) and np.all(np.isnan(ct))


def test_stream_solver_tight_tolerance(huge):
    """tol = 1e-10 on a dozen pairs spread over the fixture: the iterate sequence stays the
    oracle's for the extra iterations too."""
    from oracle import dcol_oracle as O
    d = huge
    ok = np.flatnonzero(d["expect_status"] == 0)
    idx = ok[np.linspace(0, ok.size - 1, 12).astype(int)]
    al, ct, gr, it, st = stream_emul(d, idx, 4, tol=1e-10)
    ref = O.run_batch(d, d["s1"][idx], d["s2"][idx], d["pose1"][idx], d["pose2"][idx], 1e-10, False)
    np.testing.assert_array_equal(st, ref["status"])
    np.testing.assert_array_equal(it, ref["iters"])
    assert np.all(ref["iters"] > d["iters"][idx])
    assert np.all(alpha_close(al, ref["alpha"]))


# ---------------------------------------------------------------- 3. classify and the plan policy
def test_classify_row_limits():
    descs, keep, n, k = shape_set()
    c = emul_lib.classify(descs, n, k[122], k[6])                 # 128 rows: the bucket it had
    assert (c["status"], c["o"], c["omax"], c["lpp"], c["stream"]) == (0, 128, 128, 16, 0)
    c = emul_lib.classify(descs, n, k[123], k[6])                 # 129: streamed
    assert (c["status"], c["o"], c["omax"], c["lpp"], c["stream"]) == (0, 129, 1024, 64, 1)
    c = emul_lib.classify(descs, n, k[512], k[512])               # the cap
    assert (c["status"], c["o"], c["stream"]) == (0, 1024, 1)
    c = emul_lib.classify(descs, n, k[512], k[513])               # one past it
    assert (c["status"], c["o"], c["stream"]) == (TOO_LARGE, 1025, 0)
    for a, b in ((k["cap"], k[512]), (k[513], k["gon"]), (k["sph"], k[513])):   # every other (N, NSOC)
        assert emul_lib.classify(descs, n, a, b)["stream"] == 1
    # case 4 at 40 rows (36-gon x cylinder): past the extension's 32-row list, and stays so
    c4 = emul_lib.classify(descs, n, k["gon"], k["cyl"], case4=True)
    assert (c4["status"], c4["o"], c4["stream"]) == (TOO_LARGE, 40, 0)
    assert emul_lib.classify(descs, n, k["gon"], k["cyl"])["status"] == UNSUPPORTED
    # a Jacobian plan's classification has no streamed copy
    assert emul_lib.classify(descs, n, k[123], k[6], jac=True)["status"] == TOO_LARGE
    assert emul_lib.classify(descs, n, k[122], k[6], jac=True)["status"] == 0
    assert emul_lib.max_rows() == 1024


def test_plan_with_streamed_bucket():
    """Streamed slots in descending row count; a plan with a streamed bucket is never fused or
    packed, small (a handful of pairs: the fused form otherwise) or mid-size (the packed form
    otherwise); the other buckets keep what they get without the streamed pairs."""
    descs, keep, n, k = shape_set()
    small = [(k[6], k[6]), (k[6], k["sph"]), (k["cap"], k[6]), (k["sph"], k["sph"])]
    big = [(k[123], k[6]), (k[512], k[512]), (k[6], k[123]), (k[512], k[123]), (k[123], k[123]), (k[34], k[123])]
    nrow = {k[6]: 6, k[34]: 34, k[123]: 123, k[512]: 512}
    for reps, form_without in ((1, 1), (3000, 2)):
        base = small * reps
        b0, form0, _ = plan(descs, n, [p[0] for p in base], [p[1] for p in base])
        assert form0 == form_without                       # fused / packed without streamed pairs
        mixed = []
        for i, p in enumerate(base):                       # the streamed pairs interleaved
            mixed.append(p)
            if i < len(big):
                mixed.append(big[i])
        mixed += big[len(base):]
        s1, s2 = [p[0] for p in mixed], [p[1] for p in mixed]
        b1, form1, perm = plan(descs, n, s1, s2)
        assert form1 == 0                                  # DCOL_FORM_BUCKETS
        st = [b for b in b1 if b["stream"]]
        assert len(st) == 1 and st[0]["N"] == 4 and st[0]["nsoc"] == 0
        assert (st[0]["omax"], st[0]["lpp"], st[0]["pairs"], st[0]["flags"]) == (1024, 64, len(big), 0)
        seg = perm[st[0]["slot0"]:st[0]["slot0"] + st[0]["pairs"]]
        r = [nrow[s1[i]] + nrow[s2[i]] for i in seg]
        assert r == sorted(r, reverse=True) and r[0] == 1024 and r[-1] == 129
        assert st[0]["rows"] == sum((x + 63) // 64 * 64 for x in r)
        assert sorted(perm.tolist()) == list(range(len(mixed)))
        # the register buckets are those of the plan without the streamed pairs
        key = lambda b: (b["kind"], b["N"], b["nsoc"], b["omax"], b["lpp"], b["oe"], b["flags"], b["pairs"])  # noqa: E731
        assert sorted(key(b) for b in b1 if not b["stream"]) == sorted(key(b) for b in b0)
    # a Jacobian plan keeps such pairs out
    bj, formj, _ = plan(descs, n, [k[123], k[6]], [k[6], k[6]], options=8)
    assert formj == 0 and not any(b["stream"] for b in bj)
    assert [b["code"] for b in bj if b["kind"] == 1] == [TOO_LARGE]


# ---------------------------------------------------------------- 4. header <-> binding
def test_header_constant_matches_binding():
    import dcol_amd
    text = open(os.path.join(REPO, "include", "dcol.h")).read()
    m = re.search(r"#define\s+DCOL_MAX_PAIR_ROWS\s+(\d+)", text)
    assert m and int(m.group(1)) == dcol_amd.MAX_PAIR_ROWS == dcol_amd._lib.MAX_PAIR_ROWS == 1024
    assert int(re.search(r"#define\s+DCOL_ABI_VERSION\s+(\d+)", text).group(1)) == dcol_amd._lib.ABI_VERSION == 5
    with pytest.raises(ValueError, match="1024 rows"):
        dcol_amd.raise_for_status(TOO_LARGE)


# ---------------------------------------------------------------- 5. the sanitizer run
def test_standalone_sanitizer_run():
    """tests/emul/stream_asan: the x86 solver and a main of its own under
    the host address and undefined-behaviour sanitizers, on shapes it makes itself at 129, 192,
    193, 1,023 and 1,024 rows in the three gradient modes; no Python in that process, nothing
    preloaded."""
    emul_lib.load()   # (makes the program too)
    r = subprocess.run([os.path.join(emul_lib.DIR, "stream_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    rows = {int(m) for m in re.findall(r"rows\s+(\d+)", r.stdout)}
    assert rows == {129, 192, 193, 1023, 1024}
    assert len(re.findall(r"status 0", r.stdout)) == 3 * 18 and "NON-FINITE" not in r.stdout
