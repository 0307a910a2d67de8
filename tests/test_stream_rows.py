"""Pairs above 128 orthant rows: the streamed-row solver (csrc/dcol_device.hpp StreamSolver),
its classification and plan policy, on the CPU.

Fixture tests/golden/huge/huge_rows.npz (tests/golden/gen_huge_rows.py): 152 pairs of 129 to
1,025 rows run through the reference -- every streamed (N, NSOC), the row totals at which the
slot loop changes shape (129, 192 / 193, 256 / 257, 1,012, 1,024), the pairs one row past the
cap and a few case-4 pairs.  The x86 build (tests/emul_stream, one lane walking every row)
is held to the project tolerances of DESIGN.md section 4: status and iteration counts equal,
alpha 1e-6 relative, contact 1e-6 max(|x|, 1), gradient 1e-5 max(|g|_inf, 0.01); the implicit
mode to 1e-6 max(|g|, 1) of the oracle's restatement (tests/test_implicit_grad.py's bound)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

from conftest import REPO, alpha_close, grad_close, load_golden

HUGE = os.path.join(REPO, "tests", "golden", "huge", "huge_rows.npz")
DIR = os.path.join(REPO, "tests", "emul_stream")
LIB = os.path.join(DIR, "libdcol_stream_emul.so")
TOO_LARGE, UNSUPPORTED = 5, 2
P = ctypes.c_void_p


@pytest.fixture(scope="module")
def huge():
    return load_golden(HUGE)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(LIB):
        subprocess.run(["make", "-C", DIR, "-s", "libdcol_stream_emul.so"], check=True)
    return ctypes.CDLL(LIB)


def _descs(d):
    from dcol_amd import make_descs, spec_from_arrays
    specs = [spec_from_arrays(d, k) for k in range(len(d["type"]))]
    descs, keep = make_descs(specs)
    return descs, keep, len(specs)


def stream_emul(lib, d, idx, flags, tol=None, max_iter=50):
    descs, keep, n = _descs(d)
    B = len(idx)
    s1 = np.ascontiguousarray(d["s1"][idx], np.int32)
    s2 = np.ascontiguousarray(d["s2"][idx], np.int32)
    p1 = np.ascontiguousarray(d["pose1"][idx])
    p2 = np.ascontiguousarray(d["pose2"][idx])
    al, ct, gr = np.empty(B), np.empty((B, 3)), np.empty((B, 12))
    it, st = np.empty(B, np.int32), np.empty(B, np.int32)
    rc = lib.dcol_emul_stream_batch(descs, ctypes.c_int32(n), ctypes.c_int64(B), P(s1.ctypes.data), P(s2.ctypes.data),
                                    P(p1.ctypes.data), P(p2.ctypes.data),
                                    ctypes.c_double(float(d["tol"]) if tol is None else tol), ctypes.c_int32(max_iter),
                                    ctypes.c_int32(flags), P(al.ctypes.data), P(ct.ctypes.data), P(gr.ctypes.data),
                                    P(it.ctypes.data), P(st.ctypes.data))
    assert rc == 0
    return al, ct, gr, it, st


@pytest.fixture(scope="module")
def fd_run(lib, huge):
    """the x86 streamed solver on the whole fixture, FD gradient + contact (shared, not modified)"""
    return stream_emul(lib, huge, np.arange(len(huge["s1"])), 1 | 4)


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


def test_stream_solver_envelope(lib, huge, fd_run):
    """Closed form of the derivative the reference takes by forward differences: the bound
    the envelope tests of the <= 128-row fixtures use (tests/test_emul_golden.py)."""
    d = huge
    idx = np.arange(len(d["s1"]))
    al, ct, gr, it, st = stream_emul(lib, d, idx, 2 | 4)
    ok = d["expect_status"] == 0
    np.testing.assert_array_equal(st, d["expect_status"])
    np.testing.assert_array_equal(it[ok], d["iters"][ok])
    np.testing.assert_array_equal(al[ok], fd_run[0][ok])       # the gradient mode does not touch the solve
    assert np.all(grad_close(gr[ok], d["grad"][ok]))


def implicit_reference(d, i):
    from oracle import dcol_oracle as O
    a, b = O.shape_from_table(d, d["s1"][i]), O.shape_from_table(d, d["s2"][i])
    p1, p2 = d["pose1"][i], d["pose2"][i]
    _, _, x, s, z, _, dims = O.proximity(a, p1[:3], p1[3:], b, p2[:3], p2[3:], float(d["tol"]))
    return O.implicit_gradient(a, b, x, s, z, np.concatenate([p1, p2]), dims)


def test_stream_solver_implicit(lib, huge):
    d = huge
    idx = np.flatnonzero(d["expect_status"] == 0)
    al, ct, gr, it, st = stream_emul(lib, d, idx, 16)
    assert np.all(st == 0)
    for j, i in enumerate(idx):
        ref = implicit_reference(d, i)
        assert np.abs(gr[j] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), (i, int(d["rows"][i]), gr[j], ref)


def test_stream_solver_max_iter(lib, huge):
    d = huge
    idx = np.flatnonzero(d["expect_status"] == 0)
    al, ct, gr, it, st = stream_emul(lib, d, idx, 1 | 4, max_iter=3)
    assert np.all(st == 1) and np.all(it == 3)
    assert np.all(np.isnan(al)) and np.all(np.isnan(gr)) and np.all(np.isnan(ct))


def test_stream_solver_tight_tolerance(lib, huge):
    """tol = 1e-10 on a dozen pairs spread over the fixture: the iterate sequence stays the
    oracle's for the extra iterations too."""
    from oracle import dcol_oracle as O
    d = huge
    ok = np.flatnonzero(d["expect_status"] == 0)
    idx = ok[np.linspace(0, ok.size - 1, 12).astype(int)]
    al, ct, gr, it, st = stream_emul(lib, d, idx, 4, tol=1e-10)
    ref = O.run_batch(d, d["s1"][idx], d["s2"][idx], d["pose1"][idx], d["pose2"][idx], 1e-10, False)
    np.testing.assert_array_equal(st, ref["status"])
    np.testing.assert_array_equal(it, ref["iters"])
    assert np.all(ref["iters"] > d["iters"][idx])
    assert np.all(alpha_close(al, ref["alpha"]))


# ---------------------------------------------------------------- 3. classify and the plan policy
def _shape_set():
    """descriptors: polytopes of 6, 34, 122, 123, 512, 513 faces (poly[k]), a capsule, a
    cylinder, a 36-gon, a sphere"""
    from dcol_amd import ShapeSpec, make_descs
    rng = np.random.default_rng(3)
    specs, ids = [], {}

    def poly(k):
        A = np.vstack([np.eye(3), -np.eye(3), rng.normal(size=(k - 6, 3))])
        A /= np.linalg.norm(A, axis=1, keepdims=True)
        return ShapeSpec(0, A=A, b=rng.uniform(0.4, 1.3, k))
    for k in (6, 34, 122, 123, 512, 513):
        ids[k] = len(specs)
        specs.append(poly(k))
    t = np.linspace(0, 2 * np.pi, 36, endpoint=False)
    for name, sp in (("cap", ShapeSpec(3, R=0.3, L=1.0)), ("cyl", ShapeSpec(4, R=0.3, L=1.0)),
                     ("gon", ShapeSpec(5, A=np.stack([np.cos(t), np.sin(t)], 1), b=np.full(36, 0.6), R=0.2)),
                     ("sph", ShapeSpec(1, R=0.5))):
        ids[name] = len(specs)
        specs.append(sp)
    descs, keep = make_descs(specs)
    return descs, keep, len(specs), ids


def _classify(lib, descs, n, a, b, case4=False, jac=False):
    out = (ctypes.c_int32 * 8)()
    assert lib.dcol_emul_stream_classify(descs, ctypes.c_int32(n), ctypes.c_int32(a), ctypes.c_int32(b),
                                         ctypes.c_int32(case4), ctypes.c_int32(jac), out) == 0
    return dict(zip(("status", "N", "nsoc", "o", "omax", "lpp", "oe", "stream"), list(out)))


def test_classify_row_limits(lib):
    descs, keep, n, k = _shape_set()
    c = _classify(lib, descs, n, k[122], k[6])                 # 128 rows: the bucket it had
    assert (c["status"], c["o"], c["omax"], c["lpp"], c["stream"]) == (0, 128, 128, 16, 0)
    c = _classify(lib, descs, n, k[123], k[6])                 # 129: streamed
    assert (c["status"], c["o"], c["omax"], c["lpp"], c["stream"]) == (0, 129, 1024, 64, 1)
    c = _classify(lib, descs, n, k[512], k[512])               # the cap
    assert (c["status"], c["o"], c["stream"]) == (0, 1024, 1)
    c = _classify(lib, descs, n, k[512], k[513])               # one past it
    assert (c["status"], c["o"], c["stream"]) == (TOO_LARGE, 1025, 0)
    for a, b in ((k["cap"], k[512]), (k[513], k["gon"]), (k["sph"], k[513])):   # every other (N, NSOC)
        assert _classify(lib, descs, n, a, b)["stream"] == 1
    # case 4 at 40 rows (36-gon x cylinder): past the extension's 32-row list, and stays so
    c4 = _classify(lib, descs, n, k["gon"], k["cyl"], case4=True)
    assert (c4["status"], c4["o"], c4["stream"]) == (TOO_LARGE, 40, 0)
    assert _classify(lib, descs, n, k["gon"], k["cyl"])["status"] == UNSUPPORTED
    # a Jacobian plan's classification has no streamed copy
    assert _classify(lib, descs, n, k[123], k[6], jac=True)["status"] == TOO_LARGE
    assert _classify(lib, descs, n, k[122], k[6], jac=True)["status"] == 0
    assert lib.dcol_emul_stream_max_rows() == 1024


def _plan(lib, descs, n, s1, s2, options=0, simds=256):
    B = len(s1)
    s1 = np.ascontiguousarray(s1, np.int32)
    s2 = np.ascontiguousarray(s2, np.int32)
    info = np.zeros((64, 10), np.int32)
    pairs, slot0, rows = np.zeros(64, np.int64), np.zeros(64, np.int64), np.zeros(64, np.int64)
    head, perm = np.zeros(2, np.int64), np.zeros(B, np.int32)
    rc = lib.dcol_emul_stream_plan(descs, ctypes.c_int32(n), ctypes.c_int32(simds), ctypes.c_int64(B), P(s1.ctypes.data),
                                   P(s2.ctypes.data), ctypes.c_int32(options), ctypes.c_int32(64), P(info.ctypes.data),
                                   P(pairs.ctypes.data), P(slot0.ctypes.data), P(rows.ctypes.data), P(head.ctypes.data),
                                   P(perm.ctypes.data))
    assert rc == 0
    nb = int(head[0])
    cols = ("kind", "N", "nsoc", "omax", "lpp", "oe", "flags", "code", "stream", "lane")
    buckets = [dict(zip(cols, info[i].tolist()), pairs=int(pairs[i]), slot0=int(slot0[i]), rows=int(rows[i]))
               for i in range(nb)]
    return buckets, int(head[1]), perm


def test_plan_with_streamed_bucket(lib):
    """Streamed slots in descending row count; a plan with a streamed bucket is never fused or
    packed, small (a handful of pairs: the fused form otherwise) or mid-size (the packed form
    otherwise); the other buckets keep what they get without the streamed pairs."""
    descs, keep, n, k = _shape_set()
    small = [(k[6], k[6]), (k[6], k["sph"]), (k["cap"], k[6]), (k["sph"], k["sph"])]
    big = [(k[123], k[6]), (k[512], k[512]), (k[6], k[123]), (k[512], k[123]), (k[123], k[123]), (k[34], k[123])]
    nrow = {k[6]: 6, k[34]: 34, k[123]: 123, k[512]: 512}
    for reps, form_without in ((1, 1), (3000, 2)):
        base = small * reps
        b0, form0, _ = _plan(lib, descs, n, [p[0] for p in base], [p[1] for p in base])
        assert form0 == form_without                       # fused / packed without streamed pairs
        mixed = []
        for i, p in enumerate(base):                       # the streamed pairs interleaved
            mixed.append(p)
            if i < len(big):
                mixed.append(big[i])
        mixed += big[len(base):]
        s1, s2 = [p[0] for p in mixed], [p[1] for p in mixed]
        b1, form1, perm = _plan(lib, descs, n, s1, s2)
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
    bj, formj, _ = _plan(lib, descs, n, [k[123], k[6]], [k[6], k[6]], options=8)
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
    """tests/emul_stream/stream_asan: the x86 solver and a main of its own under
    the host address and undefined-behaviour sanitizers, on shapes it makes itself at 129, 192,
    193, 1,023 and 1,024 rows in the three gradient modes; no Python in that process, nothing
    preloaded."""
    subprocess.run(["make", "-C", DIR, "-s", "stream_asan"], check=True)
    r = subprocess.run([os.path.join(DIR, "stream_asan")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "ERROR" not in r.stderr and "runtime error" not in r.stderr
    rows = {int(m) for m in re.findall(r"rows\s+(\d+)", r.stdout)}
    assert rows == {129, 192, 193, 1023, 1024}
    assert len(re.findall(r"status 0", r.stdout)) == 3 * 18 and "NON-FINITE" not in r.stdout
