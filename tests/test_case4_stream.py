"""Case-4 pairs of 33 to 1,024 orthant rows (polygon x capsule / cylinder / polygon): the
streamed-row solver's case-4 instances (csrc/dcol_device.hpp StreamSolver, N >= 7), their
classification and plan policy under DCOL_PLAN_CASE4_STREAM, on the CPU.

Fixture tests/golden/case4_huge/case4_rows.npz (tests/golden/gen_case4_rows.py): 192 pairs of 32
to 1,027 rows, the NumPy oracle's own values (the reference raises for case 4), pinned here to
brute-force geometry.  A capsule brings 2 orthant rows, a cylinder 4, an n-gon n; the row totals
are those at which the slot loop changes shape -- 32 (the last register bucket), 33 (the first
streamed count, one partial slot), 64 / 65, 128 / 129, 400, 1,023 (odd tail), 1,024 (the cap) --
and 1,025 to 1,027 (DCOL_TOO_LARGE), each with the polygon first and second where the pair has
two orders.  The x86 build (tests/emul_case4, one lane walking every row) is held to the project
tolerances of DESIGN.md section 4: status and iteration counts equal, alpha 1e-6 relative,
contact 1e-6 max(|x|, 1), gradient 1e-5 max(|g|_inf, 0.01); the implicit mode to 1e-6 max(|g|, 1)
of the oracle's restatement; the Jacobian copies under case4_stream_cases.check_against_restatement.
"""
import os
import re
import subprocess

import numpy as np
import pytest

import emul_case4_lib as E
from case4_stream_cases import (CONTACT, ENVELOPE, FD, FIXTURE, IMPLICIT, JACOBIAN, MAXITER, PLAN_CASE4, PLAN_CASE4_STREAM,
                                PLAN_JACOBIAN, PLAN_JACOBIAN_STREAM, TOO_LARGE, bits, check_against_restatement,
                                check_implicit, check_solution, fixture, solvable, streamed)
from conftest import REPO
from geometry_bruteforce import min_scaling
from test_case4 import body


@pytest.fixture(scope="module")
def fd_run():
    """the x86 case-4 streamed solver on the whole fixture, FD gradient + contact (shared, not modified)"""
    return E.solve(fixture(), FD | CONTACT)


def jac_pairs():
    """poses 0 and 3 of every streamed pair of the fixture"""
    d = fixture()
    return np.array([i for i in streamed() if i % 6 in (0, 3)])


# ---------------------------------------------------------------- 1. the checker
def test_fixture_contents():
    d = fixture()
    ok = d["expect_status"] == 0
    rows = d["rows"]
    assert len(rows) == 192 and os.path.getsize(FIXTURE) <= 300 * 1024
    assert {32, 33, 34, 35, 64, 65, 128, 129, 400, 1023, 1024} <= set(rows[ok].tolist())
    assert rows[ok].max() == 1024 and set(rows[~ok].tolist()) == {1025, 1026, 1027}
    assert np.all(d["status"] == 0) and int(d["replaced"]) <= 0.05 * int(d["draws"])
    assert 7 <= d["iters"][ok].min() and d["iters"][ok].max() <= 20
    t1, t2 = d["type"][d["s1"]], d["type"][d["s2"]]
    for a, b in ((5, 3), (3, 5), (5, 4), (4, 5), (5, 5)):                  # both orders, streamed
        assert np.any(ok & (t1 == a) & (t2 == b) & (rows == 33)), (a, b)
    for a, b in ((5, 4), (4, 5), (5, 5), (5, 3)):
        assert np.any(ok & (t1 == a) & (t2 == b) & (rows == 1024)), (a, b)
    assert np.any(np.abs(d["r_offset"]).sum(axis=1) > 0)


def test_oracle_reproduces_fixture():
    from oracle import dcol_oracle as O
    d = fixture()
    idx = np.arange(0, len(d["s1"]), 6)
    out = O.run_batch(d, d["s1"][idx], d["s2"][idx], d["pose1"][idx], d["pose2"][idx], float(d["tol"]), True, case4=True)
    for k in ("status", "iters", "alpha", "contact", "grad"):
        np.testing.assert_array_equal(out[k], d[k][idx], err_msg=k)


def test_oracle_matches_bruteforce_geometry():
    """tests/test_case4.py's rule at tol = 1e-11, one pose each of 16 x 17, cyl x 31, 33 x cap,
    cap x 31, 64 x 65 and 512 x 512 (1,024 rows): the oracle's point lies in both shapes scaled
    by its alpha, and no point needs a smaller scaling."""
    from oracle import dcol_oracle as O
    d = fixture()
    nh, ty = d["nh"], d["type"]
    name = lambda k: {3: "cap", 4: "cyl"}.get(int(ty[k]), int(nh[k]))  # noqa: E731
    want = [(16, 17), ("cyl", 31), (33, "cap"), ("cap", 31), (64, 65), (512, 512)]
    idx = []
    for w in want:
        hit = [i for i in range(len(d["s1"])) if (name(d["s1"][i]), name(d["s2"][i])) == w]
        idx.append(hit[0])
    idx = np.array(idx)
    assert 1024 in d["rows"][idx].tolist()
    out = O.run_batch(d, d["s1"][idx], d["s2"][idx], d["pose1"][idx], d["pose2"][idx], tol=1e-11, want_grad=False, case4=True)
    assert (out["status"] == O.ST_OK).all()
    for j, i in enumerate(idx):
        b1, b2 = body(d, int(d["s1"][i]), d["pose1"][i]), body(d, int(d["s2"][i]), d["pose2"][i])
        a, c = out["alpha"][j], out["contact"][j]
        g = max(b1.gauge(c), b2.gauge(c))
        a_bf, _ = min_scaling(b1, b2, starts=[c])
        print(f"pair {int(i)} {want[j]}: alpha {a:.12g} gauge - alpha {g - a:.2e} brute force - alpha {a_bf - a:.2e}")
        assert g <= a * (1 + 1e-9) + 1e-12, (int(i), want[j])
        assert abs(a_bf - a) <= 1e-8 * max(1.0, a), (int(i), want[j], a_bf, a)


# ---------------------------------------------------------------- 2. the x86 streamed solver
def test_stream_solver_matches_fixture_fd(fd_run):
    d = fixture()
    al, ct, gr, it, st = fd_run
    np.testing.assert_array_equal(st, d["expect_status"])
    ok = solvable()
    check_solution(d, ok, al[ok], ct[ok], gr[ok], it[ok], st[ok])
    big = d["expect_status"] == TOO_LARGE
    assert big.sum() == 30 and np.all(d["rows"][big] > 1024)
    assert np.all(np.isnan(al[big])) and np.all(np.isnan(gr[big])) and np.all(np.isnan(ct[big]))


def test_stream_solver_envelope(fd_run):
    d, ok = fixture(), solvable()
    al, ct, gr, it, st = E.solve(d, ENVELOPE | CONTACT, ok)
    check_solution(d, ok, al, ct, gr, it, st)
    np.testing.assert_array_equal(bits(al), bits(fd_run[0][ok]))       # the gradient mode does not touch the solve


def test_stream_solver_implicit(fd_run):
    d, ok = fixture(), solvable()
    al, ct, gr, it, st = E.solve(d, IMPLICIT | CONTACT, ok)
    check_solution(d, ok, al, ct, None, it, st)
    np.testing.assert_array_equal(bits(al), bits(fd_run[0][ok]))
    check_implicit(ok, gr)


def test_stream_solver_max_iter():
    d, ok = fixture(), solvable()
    al, ct, gr, it, st = E.solve(d, FD | CONTACT, ok, max_iter=3)
    assert np.all(st == MAXITER) and np.all(it == 3)
    assert np.all(np.isnan(al)) and np.all(np.isnan(gr)) and np.all(np.isnan(ct))


# ---------------------------------------------------------------- 3. the x86 Jacobian copies
def test_jacobian_copies_match_restatement(fd_run):
    d, idx = fixture(), jac_pairs()
    al, ct, gr, jc, it, st = E.solve(d, FD | CONTACT | JACOBIAN, idx, jac=True)
    assert np.all(st == 0)
    np.testing.assert_array_equal(it, d["iters"][idx])
    for name, a, b in (("alpha", al, fd_run[0][idx]), ("contact", ct, fd_run[1][idx]), ("grad", gr, fd_run[2][idx])):
        np.testing.assert_array_equal(bits(a), bits(b), err_msg=name)   # the plain instance's, bitwise
    check_against_restatement(idx, jc)
    # without a gradient flag the phase forms the z aggregates itself: the same J, bitwise
    sub = idx[::4]
    jc2 = E.solve(d, CONTACT | JACOBIAN, sub, jac=True)[3]
    np.testing.assert_array_equal(bits(jc2), bits(jc[::4]))


# ---------------------------------------------------------------- 4. classify and the plan policy
def shape_ids():
    d = fixture()
    descs, n = E.descs_of(d)
    k = {{3: "cap", 4: "cyl"}.get(int(t), int(h)): i for i, (t, h) in enumerate(zip(d["type"], d["nh"]))}
    return descs, n, k


def test_classify_case4_stream():
    descs, n, k = shape_ids()
    c = E.classify(descs, n, k[28], k["cyl"])                          # 32 rows: the register bucket it had
    assert (c["status"], c["N"], c["nsoc"], c["o"], c["omax"], c["stream"]) == (0, 7, 2, 32, 32, 0)
    assert c == E.classify(descs, n, k[28], k["cyl"], case4_stream=False)
    c = E.classify(descs, n, k[29], k["cyl"])                          # 33: streamed
    assert (c["status"], c["N"], c["nsoc"], c["o"], c["omax"], c["lpp"], c["stream"]) == (0, 7, 2, 33, 1024, 64, 1)
    c = E.classify(descs, n, k[16], k[17])
    assert (c["status"], c["N"], c["nsoc"], c["o"], c["omax"], c["lpp"], c["stream"]) == (0, 8, 2, 33, 1024, 64, 1)
    c = E.classify(descs, n, k[512], k[512])                           # the cap
    assert (c["status"], c["o"], c["stream"]) == (0, 1024, 1)
    c = E.classify(descs, n, k[512], k[513])                           # one past it
    assert (c["status"], c["o"], c["stream"]) == (TOO_LARGE, 1025, 0)
    # without the new parameter, or with stream off (a Jacobian plan without its streamed copies): as before
    for kw in (dict(case4_stream=False), dict(stream=False, part=False)):
        c = E.classify(descs, n, k[29], k["cyl"], **kw)
        assert (c["status"], c["o"], c["stream"]) == (TOO_LARGE, 33, 0)
    assert E.classify(descs, n, k[29], k["cyl"], case4=False)["status"] == 2          # UNSUPPORTED
    # capsule / cylinder pairs -- case-4 (6, 2) -- never stream
    c = E.classify(descs, n, k["cyl"], k["cap"])
    assert (c["status"], c["N"], c["stream"]) == (0, 6, 0)


def test_plan_with_case4_streamed_buckets():
    """40 rows (36-gon x cylinder, tests/stream_cases.py) with options 1 | 32: a streamed (7, 2)
    bucket at omax 1024, lpp 64, form 0; with option 1 alone a TOO_LARGE reject bucket, as today;
    option 32 alone an argument error.  Slots in descending row count; the register buckets are
    those of the plan without the streamed pairs."""
    from stream_cases import shape_set
    descs, keep, n, k = shape_set()
    b, form, _ = E.plan(descs, n, [k["gon"]], [k["cyl"]], PLAN_CASE4 | PLAN_CASE4_STREAM)
    assert form == 0 and len(b) == 1
    assert (b[0]["kind"], b[0]["N"], b[0]["nsoc"], b[0]["omax"], b[0]["lpp"], b[0]["stream"], b[0]["flags"]) == (0, 7, 2, 1024, 64, 1, 0)
    b, form, _ = E.plan(descs, n, [k["gon"]], [k["cyl"]], PLAN_CASE4)
    assert [(x["kind"], x["code"]) for x in b] == [(1, TOO_LARGE)]
    with pytest.raises(E.EmulError, match="needs DCOL_PLAN_CASE4"):
        E.plan(descs, n, [k["gon"]], [k["cyl"]], PLAN_CASE4_STREAM)
    # a Jacobian plan streams them only with DCOL_PLAN_JACOBIAN_STREAM as well
    b, _, _ = E.plan(descs, n, [k["gon"]], [k["cyl"]], PLAN_CASE4 | PLAN_CASE4_STREAM | PLAN_JACOBIAN)
    assert [(x["kind"], x["code"]) for x in b] == [(1, TOO_LARGE)]
    b, _, _ = E.plan(descs, n, [k["gon"]], [k["cyl"]], PLAN_CASE4 | PLAN_CASE4_STREAM | PLAN_JACOBIAN | PLAN_JACOBIAN_STREAM)
    assert [(x["kind"], x["N"], x["stream"]) for x in b] == [(0, 7, 1)]

    d = fixture()
    descs, n, k = shape_ids()
    small = [(k["cap"], k["cyl"]), (k[16], k["cap"]), (k["cyl"], k[17]), (k[16], k[16]), (k[28], k["cyl"])]
    big_idx = streamed()[::6]
    big = list(zip(d["s1"][big_idx].tolist(), d["s2"][big_idx].tolist()))
    for reps in (1, 3000):
        base = small * reps
        b0, _, _ = E.plan(descs, n, [p[0] for p in base], [p[1] for p in base], PLAN_CASE4)
        mixed = []
        for i, p in enumerate(base):
            mixed.append(p)
            if i < len(big):
                mixed.append(big[i])
        mixed += big[len(base):]
        s1, s2 = [p[0] for p in mixed], [p[1] for p in mixed]
        b1, form1, perm = E.plan(descs, n, s1, s2, PLAN_CASE4 | PLAN_CASE4_STREAM)
        assert form1 == 0
        st = [x for x in b1 if x["stream"]]
        assert sorted((x["N"], x["nsoc"]) for x in st) == [(7, 2), (8, 2)]
        assert all((x["omax"], x["lpp"], x["flags"]) == (1024, 64, 0) for x in st)
        assert sum(x["pairs"] for x in st) == len(big)
        rows_of = lambda s: {3: 2, 4: 4}.get(int(d["type"][s]), int(d["nh"][s]))  # noqa: E731
        for x in st:
            seg = perm[x["slot0"]:x["slot0"] + x["pairs"]]
            r = [rows_of(s1[i]) + rows_of(s2[i]) for i in seg]
            assert r == sorted(r, reverse=True) and r[-1] > 32
            assert x["rows"] == sum((v + 63) // 64 * 64 for v in r)
        assert sorted(perm.tolist()) == list(range(len(mixed)))
        key = lambda x: (x["kind"], x["N"], x["nsoc"], x["omax"], x["lpp"], x["oe"], x["flags"], x["pairs"])  # noqa: E731
        assert sorted(key(x) for x in b1 if not x["stream"]) == sorted(key(x) for x in b0)
        # without the option those pairs are rejected, the rest unchanged
        b2, _, _ = E.plan(descs, n, s1, s2, PLAN_CASE4)
        assert [(x["code"], x["pairs"]) for x in b2 if x["kind"] == 1] == [(TOO_LARGE, len(big))]


# ---------------------------------------------------------------- 5. header <-> binding
def test_header_constants_match_binding():
    import dcol_amd
    from dcol_amd import _lib
    text = open(os.path.join(REPO, "include", "dcol.h")).read()
    assert int(re.search(r"DCOL_PLAN_CASE4_STREAM\s*=\s*(\d+)", text).group(1)) == _lib.PLAN_CASE4_STREAM == 32
    assert int(re.search(r"DCOL_CASE4_STREAM\s*=\s*(\d+)", text).group(1)) == _lib.CASE4_STREAM == 256
    assert int(re.search(r"#define\s+DCOL_ABI_VERSION\s+(\d+)", text).group(1)) == _lib.ABI_VERSION == 5
    # the flag collides with no kernel flag bit (csrc/dcol_device.hpp F_*)
    dev = open(os.path.join(REPO, "dcol-trajectory-optimization_amd", "csrc", "dcol_device.hpp")).read()
    fbits = [int(v) for v in re.findall(r"\bF_[A-Z_]+ = (\d+)", dev)]
    assert fbits and not any(v & _lib.CASE4_STREAM for v in fbits)
    with pytest.raises(ValueError, match="1024 rows.*DCOL_PLAN_CASE4_STREAM.*128 with the contact-point Jacobian"):
        dcol_amd.raise_for_status(TOO_LARGE)
    from dcol_amd.engine import case4_mode
    assert (case4_mode(False), case4_mode(True), case4_mode(1), case4_mode("stream")) == (False, True, True, "stream")
    with pytest.raises(ValueError, match="case4 must be"):
        case4_mode("streamed")


# ---------------------------------------------------------------- 6. the sanitizer run
def test_standalone_sanitizer_run():
    """tests/emul_case4/case4_stream_asan: the x86 case-4 instances and a main of its own under
    the host address and undefined-behaviour sanitizers, on shapes it makes itself at 33, 65,
    1,023 and 1,024 rows, in the three gradient modes and with the Jacobian; no Python in that
    process, nothing preloaded."""
    E.load()   # (makes the program too)
    r = subprocess.run([E.ASAN], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    assert {int(m) for m in re.findall(r"rows\s+(\d+)", r.stdout)} == {33, 65, 1023, 1024}
    assert {m for m in re.findall(r"\(N, NSOC\) \((\d), 2\)", r.stdout)} == {"7", "8"}
    assert len(re.findall(r"streamed 1 status 0", r.stdout)) == 5 * 12 and "NON-FINITE" not in r.stdout
