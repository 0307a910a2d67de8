"""Case-4 pairs of 33 to 1,024 orthant rows on the GPU: the case-4 streamed kernels
(csrc/dcol_kernels_stream_c4.hip, dcol_kernels_stream_c4_jac.hip) through Engine with
case4="stream" (DCOL_PLAN_CASE4_STREAM / DCOL_CASE4_STREAM), plans, the contact-point Jacobian, the
record path and the codegen twin.  Expected values: the NumPy oracle's, from
tests/golden/case4_huge/case4_rows.npz (see tests/test_case4_stream.py), at the project tolerances
of DESIGN.md section 4."""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

from case4_stream_cases import (FIXTURE, REGISTER_ROWS, TOO_LARGE, bits, check_against_restatement, check_implicit,
                                check_solution, fixture, register, soa, solvable, streamed)
from conftest import PKG, REPO, golden_files, load_golden

pytestmark = pytest.mark.gpu

XCHECK_LIB = os.path.join(PKG, "lib_xcheck", "libdcol.so")
KEYS = ("status", "iters", "alpha", "contact", "grad")


@pytest.fixture(scope="module")
def ids(engine):
    return register(engine, fixture())


@pytest.fixture(scope="module")
def fd_run(engine, ids):
    """the whole fixture through Engine.solve_host, FD gradient + contact (shared, not modified)"""
    d = fixture()
    return engine.solve_host(ids[0], ids[1], d["pose1"], d["pose2"], tol=float(d["tol"]), grad="fd", case4="stream")


def run_mode(engine, ids, mode, **kw):
    d = fixture()
    return engine.solve_host(ids[0], ids[1], d["pose1"], d["pose2"], tol=float(d["tol"]), grad=mode, **kw)


# ---------------------------------------------------------------- 1. the fixture through Engine
def test_fixture_three_modes(engine, ids, fd_run):
    d, ok = fixture(), solvable()
    big = d["expect_status"] == TOO_LARGE
    res = {"fd": fd_run, "envelope": run_mode(engine, ids, "envelope", case4="stream"),
           "implicit": run_mode(engine, ids, "implicit", case4="stream")}
    for mode, r in res.items():
        np.testing.assert_array_equal(r.status, d["expect_status"], err_msg=mode)
        check_solution(d, ok, r.alpha[ok], r.contact[ok], None if mode == "implicit" else r.grad[ok], r.iters[ok], r.status[ok])
        assert big.sum() == 30 and np.all(np.isnan(r.alpha[big])) and np.all(np.isnan(r.grad[big])) and np.all(np.isnan(r.contact[big]))
        np.testing.assert_array_equal(bits(r.alpha[ok]), bits(fd_run.alpha[ok]), err_msg=mode)   # the mode does not touch the solve
    check_implicit(ok, res["implicit"].grad[ok])


def test_fixture_max_iter(engine, ids):
    d, ok = fixture(), solvable()
    res = engine.solve_host(ids[0][ok], ids[1][ok], d["pose1"][ok], d["pose2"][ok], max_iter=3, grad="fd", case4="stream")
    assert np.all(res.status == 1) and np.all(res.iters == 3)
    assert np.all(np.isnan(res.alpha)) and np.all(np.isnan(res.grad))


# ---------------------------------------------------------------- 2. options and mixed plans
def test_without_the_option_nothing_changes(engine, ids, fd_run):
    """case4=True: TOO_LARGE above 32 rows, as before; the pairs of at most 32 rows bitwise what
    case4="stream" gives them.  Option 32 alone: DCOL_ERR_ARG."""
    from dcol_amd import _lib
    d = fixture()
    res = run_mode(engine, ids, "fd", case4=True)
    above = d["rows"] > REGISTER_ROWS
    assert np.all(res.status[above] == TOO_LARGE) and np.all(np.isnan(res.alpha[above])) and np.all(np.isnan(res.grad[above]))
    assert (~above).sum() == 18 and np.all(res.status[~above] == 0)
    for k in KEYS:
        np.testing.assert_array_equal(bits(getattr(res, k)[~above]), bits(getattr(fd_run, k)[~above]), err_msg=k)
    res = run_mode(engine, ids, None)
    assert np.all(res.status == 2)                                     # UNSUPPORTED, the reference's behaviour
    lib = _lib.load()
    s1, s2 = np.ascontiguousarray(ids[0]), np.ascontiguousarray(ids[1])
    for opts, code in ((_lib.PLAN_CASE4_STREAM, _lib.ERR_ARG), (_lib.PLAN_CASE4_STREAM | _lib.PLAN_NO_FUSE, _lib.ERR_ARG)):
        h = ctypes.c_void_p()
        rc = lib.dcol_plan_create_ex(engine.table.handle, len(s1), ctypes.c_void_p(s1.ctypes.data), ctypes.c_void_p(s2.ctypes.data),
                                     opts, ctypes.byref(h))
        assert rc == code and not h.value
        assert b"DCOL_PLAN_CASE4_STREAM needs DCOL_PLAN_CASE4" in lib.dcol_last_error()
    with pytest.raises(ValueError, match="case4 must be"):
        engine.plan(s1, s2, case4="streamed")
    assert engine.plan(s1, s2, case4=True) is not engine.plan(s1, s2, case4="stream")   # the cache tells them apart
    assert engine.plan(s1, s2, case4="stream").case4 == "stream"


def test_mixed_plan_bitwise(engine, ids):
    """The fixture's pairs interleaved with 300 pairs of synthetic_mixed and 60 pairs of the small
    case-4 table (tests/case4_shapes.py), sentinel-filled outputs: every slot written; the pairs
    of at most 32 rows and every pair of cases 1-3 bitwise what a case4=True plan gives them; the
    streamed pairs bitwise those of a plan of theirs alone."""
    import torch
    from case4_shapes import case4_table
    from dcol_amd import alloc_outputs
    d = fixture()
    m = load_golden([p for p in golden_files() if p.endswith("synthetic_mixed.npz")][0])
    rng = np.random.default_rng(5)
    c = case4_table(rng)
    nc = 60
    c.update(s1=rng.integers(0, len(c["type"]), nc).astype(np.int32), s2=rng.integers(0, len(c["type"]), nc).astype(np.int32),
             pose1=np.hstack([rng.uniform(-1.5, 1.5, (nc, 3)), rng.uniform(-1, 1, (nc, 3))]),
             pose2=np.hstack([rng.uniform(-1.5, 1.5, (nc, 3)), rng.uniform(-1, 1, (nc, 3))]))
    m1, m2 = register(engine, m)
    c1, c2 = register(engine, c)
    h1, h2 = register(engine, d)                                   # (ids of the table as it stands now)
    nh, nm = len(h1), 300
    B = nh + nm + nc
    assert B % 64 != 0
    kind = np.full(B, 1)                                           # 0 fixture, 1 synthetic_mixed, 2 small case 4
    kind[np.round(np.linspace(0, B - 1, nh)).astype(int)] = 0
    rest = np.flatnonzero(kind == 1)
    kind[rest[np.round(np.linspace(0, rest.size - 1, nc)).astype(int)]] = 2
    s1, s2, p1, p2 = np.empty(B, np.int32), np.empty(B, np.int32), np.empty((B, 6)), np.empty((B, 6))
    for kd, (a, b, q1, q2) in enumerate(((h1, h2, d["pose1"], d["pose2"]), (m1[:nm], m2[:nm], m["pose1"][:nm], m["pose2"][:nm]),
                                         (c1, c2, c["pose1"], c["pose2"]))):
        s1[kind == kd], s2[kind == kd], p1[kind == kd], p2[kind == kd] = a, b, q1, q2
    is_streamed = np.zeros(B, bool)
    is_streamed[np.flatnonzero(kind == 0)[streamed()]] = True

    def run(sel, case4):
        plan = engine.plan(s1[sel], s2[sel], cache=False, case4=case4)
        out = alloc_outputs(int(sel.sum()), torch.device("cuda", 0))
        for v in out.values():                                     # sentinels: a slot nobody writes keeps them
            v.fill_(-7 if v.dtype == torch.int32 else 12345.0)
        plan.run(soa(p1[sel]), soa(p2[sel]), grad="fd", out=out)
        torch.cuda.synchronize()
        return plan, {k: (v.cpu().numpy().T if v.dim() == 2 else v.cpu().numpy()) for k, v in out.items()}

    plan, mixed = run(np.ones(B, bool), "stream")
    assert plan.launch_form == "buckets"
    st = [b for b in plan.buckets() if b["kind"] == "solve" and b["omax"] == 1024]
    assert sorted((b["N"], b["nsoc"]) for b in st) == [(7, 2), (8, 2)] and all(b["lpp"] == 64 for b in st)
    assert sum(b["pairs"] for b in st) == int(is_streamed.sum()) == streamed().size
    assert not np.any(mixed["status"] == -7) and not np.any(mixed["iters"] == -7)
    for k in ("alpha", "contact", "grad"):
        assert not np.any(mixed[k] == 12345.0), k
    np.testing.assert_array_equal(mixed["status"][kind == 0], d["expect_status"])
    c4 = m["status"][:nm] == 2                                      # (its case-4 pairs, which the option solves)
    np.testing.assert_array_equal(mixed["status"][kind == 1][~c4], m["status"][:nm][~c4])
    assert c4.any() and np.all(mixed["status"][kind == 1][c4] != 2)
    assert (mixed["status"][kind == 2] == 0).mean() > 0.9
    _, plain = run(np.ones(B, bool), True)
    assert np.all(plain["status"][is_streamed] == TOO_LARGE)
    _, alone = run(is_streamed, "stream")
    for k in KEYS:
        np.testing.assert_array_equal(bits(mixed[k][~is_streamed]), bits(plain[k][~is_streamed]), err_msg=f"register buckets: {k}")
        np.testing.assert_array_equal(bits(mixed[k][is_streamed]), bits(alone[k]), err_msg=f"streamed buckets: {k}")


# ---------------------------------------------------------------- 3. the contact-point Jacobian
def test_jacobian(engine, ids, fd_run):
    """jacobian="stream", case4="stream" on poses 0 and 3 of every streamed pair: J under
    case4_stream_cases.check_against_restatement; alpha, contact and status bitwise the plain
    run's.  Without jacobian="stream" those pairs are TOO_LARGE with NaN Jacobians."""
    d = fixture()
    idx = np.array([i for i in streamed() if i % 6 in (0, 3)])
    args = (ids[0][idx], ids[1][idx], d["pose1"][idx], d["pose2"][idx])
    res = engine.solve_host(*args, tol=float(d["tol"]), grad="fd", case4="stream", jacobian="stream")
    assert np.all(res.status == 0)
    for k in KEYS:
        np.testing.assert_array_equal(bits(getattr(res, k)), bits(getattr(fd_run, k)[idx]), err_msg=k)
    check_against_restatement(idx, res.jac)
    res = engine.solve_host(*args, tol=float(d["tol"]), grad="fd", case4="stream", jacobian=True)
    assert np.all(res.status == TOO_LARGE) and np.all(np.isnan(res.jac)) and np.all(np.isnan(res.alpha))
    # a device-resident plan with both options: the streamed buckets, and run(jacobian=True) writes the same J
    import torch
    plan = engine.plan(args[0], args[1], cache=False, case4="stream", jacobian="stream")
    assert sorted((b["N"], b["omax"], b["lpp"]) for b in plan.buckets()) == [(7, 1024, 64), (8, 1024, 64)]
    out = plan.run(soa(args[2]), soa(args[3]), tol=float(d["tol"]), grad="fd", jacobian=True)
    torch.cuda.synchronize()
    jac = out["jac"].cpu().numpy().T.reshape(-1, 4, 12)
    res = engine.solve_host(*args, tol=float(d["tol"]), grad="fd", case4="stream", jacobian="stream")
    np.testing.assert_array_equal(bits(jac), bits(res.jac))


# ---------------------------------------------------------------- 4. record path
def test_record_path(engine, ids):
    """rec set and the SoA outputs null (dcol_prox_batch_multi_gpu in place at world 1, records
    only): the 14-double records equal the SoA run's values bitwise."""
    import torch
    from dcol_amd.dist import REC, NativeComm, unpack
    d = fixture()
    plan = engine.plan(ids[0], ids[1], cache=False, case4="stream")
    p1, p2 = soa(d["pose1"]), soa(d["pose2"])
    n = plan.B
    comm = NativeComm(NativeComm.unique_id(), 1, 0, 0)
    try:
        junk = torch.full((n + 3, REC), 3.0, dtype=torch.float64, device="cuda")
        none_out, rec = comm.solve_gather(plan, p1, p2, cap=n + 3, grad="fd", rec_all=junk, in_place=True, soa=False)
        ref = plan.run(p1, p2, grad="fd", contact=False)
        torch.cuda.synchronize()
    finally:
        comm.close()
    assert none_out is None
    rec = rec.cpu().numpy()
    assert np.all(rec[n:].view(np.uint64) == np.uint64(0xFFFFFFFFFFFFFFFF))
    u = unpack(rec[:n])
    np.testing.assert_array_equal(u["status"], d["expect_status"])
    np.testing.assert_array_equal(u["status"], ref["status"].cpu().numpy())
    np.testing.assert_array_equal(u["iters"], ref["iters"].cpu().numpy())
    np.testing.assert_array_equal(bits(u["alpha"]), bits(ref["alpha"].cpu().numpy()))
    np.testing.assert_array_equal(bits(u["grad"]), bits(ref["grad"].cpu().numpy().T))


# ---------------------------------------------------------------- 5. codegen twin
_TWIN_SCRIPT = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[3]]
from dcol_amd import Engine, spec_from_arrays
d = dict(np.load(sys.argv[4]))
eng = Engine(device=0)
ids = np.array([eng.register(spec_from_arrays(d, k)) for k in range(len(d["type"]))], np.int32)
out = {}
for mode in ("fd", "envelope", "implicit"):
    r = eng.solve_host(ids[d["s1"]], ids[d["s2"]], d["pose1"], d["pose2"], tol=float(d["tol"]), grad=mode, case4="stream")
    out.update({f"{mode}_{k}": getattr(r, k) for k in ("status", "iters", "alpha", "contact", "grad")})
np.savez(sys.argv[1], **out)
"""


@pytest.mark.skipif(not os.path.exists(XCHECK_LIB), reason="lib_xcheck not built (make -C csrc xcheck)")
def test_codegen_twin(tmp_path, engine, ids, fd_run):
    """lib_xcheck -- the same sources under the other machine schedule -- agrees bitwise with
    the product library on the fixture, in the three gradient modes."""
    env = {k: v for k, v in os.environ.items() if k not in ("DCOL_NO_BALL", "DCOL_NO_CONE", "DCOL_LPP")}
    env["DCOL_LIB"] = XCHECK_LIB
    f = str(tmp_path / "twin.npz")
    subprocess.run([sys.executable, "-c", _TWIN_SCRIPT, f, PKG, REPO, FIXTURE], check=True, env=env, timeout=300)
    twin = dict(np.load(f))
    for mode in ("fd", "envelope", "implicit"):
        r = fd_run if mode == "fd" else run_mode(engine, ids, mode, case4="stream")
        for k in KEYS:
            np.testing.assert_array_equal(bits(getattr(r, k)), bits(twin[f"{mode}_{k}"]), err_msg=f"{mode} {k}")
