"""The contact-point Jacobian of pairs of 129 to 1,024 orthant rows on the GPU: the streamed-row
kernels' Jacobian copies (csrc/dcol_kernels_stream_jac.hip) through Engine.solve_host(
jacobian="stream"), plans made with DCOL_PLAN_JACOBIAN | DCOL_PLAN_JACOBIAN_STREAM, the drop-in
and a captured graph.  Expected values: the fixture tests/golden/huge/huge_rows.npz at the parity
tolerances of tests/test_stream_rows_gpu.py, and the NumPy restatement under the rule of
tests/test_stream_jacobian.py (err <= tolerance for every compared pair, none excused)."""
import ctypes

import numpy as np
import pytest

import jacobian_cases
from conftest import alpha_close, grad_close
from contact_jacobian_ref import contact_jacobian, tolerance
from stream_cases import TOO_LARGE, UNSUPPORTED, bits, check_against_restatement, huge, ok_pairs, register, soa

pytestmark = pytest.mark.gpu

KEYS = ("status", "iters", "alpha", "contact", "grad")
ORDERS = ((0, 0), (0, 1), (1, 0), (0, 2), (2, 0), (3, 0), (0, 3), (4, 0), (0, 4), (5, 0), (0, 5), (5, 1), (1, 5),
          (5, 2), (2, 5))


def selection(n=48):
    """n pairs of ok: one of each of 129, 192, 193, 1,012 and 1,024 rows and one of every
    primitive-type order (every streamed (N, NSOC), both orders), the rest spread over ok"""
    d, ok = huge(), ok_pairs()
    t1, t2 = d["type"][d["s1"]], d["type"][d["s2"]]
    sel = []
    for r in (129, 192, 193, 1012, 1024):
        sel.append(int(ok[d["rows"][ok] == r][0]))
    for a, b in ORDERS:
        sel.append(int(ok[(t1[ok] == a) & (t2[ok] == b)][0]))
    sel = list(dict.fromkeys(sel))
    for i in ok[np.linspace(0, ok.size - 1, n).astype(int)]:
        if len(sel) >= n:
            break
        if int(i) not in sel:
            sel.append(int(i))
    assert len(sel) == n
    return np.array(sorted(sel))


@pytest.fixture(scope="module")
def ids(engine):
    return register(engine, huge())


@pytest.fixture(scope="module")
def full_run(engine, ids):
    """the whole fixture through solve_host(jacobian="stream"), FD gradient (shared, not modified)"""
    d = huge()
    return engine.solve_host(ids[0], ids[1], d["pose1"], d["pose2"], tol=float(d["tol"]), grad="fd", jacobian="stream")


# ---------------------------------------------------------------- 1. the fixture
def test_gpu_fixture_jacobian(full_run):
    """48 pairs: status, iters, alpha, contact and grad at the parity tolerances, J under the
    restatement rule.  Where the wave can go wrong and the one-lane x86 build cannot: a last
    slot with one live lane (129 rows), exactly full slots (192), the SOC share added once
    after the reduction (every NSOC > 0 instance)."""
    d, res = huge(), full_run
    idx = selection()
    rows = set(d["rows"][idx].tolist())
    assert {129, 192, 193, 1012, 1024} <= rows
    assert res.jac.shape == (len(d["s1"]), 4, 12)
    np.testing.assert_array_equal(res.status[idx], 0)
    np.testing.assert_array_equal(res.iters[idx], d["iters"][idx])
    assert np.all(alpha_close(res.alpha[idx], d["alpha"][idx]))
    assert np.all(np.abs(res.contact[idx] - d["contact"][idx]) <= 1e-6 * np.maximum(np.abs(d["contact"][idx]), 1.0))
    assert np.all(grad_close(res.grad[idx], d["grad"][idx]))
    check_against_restatement(idx, res.jac[idx])


# ---------------------------------------------------------------- 2. guarded window, 3. bitwise
def _small_pairs(engine, n):
    """n pairs of at most 128 rows (synthetic_mixed) -> (s1, s2, pose1, pose2, [(name, index)])"""
    m, midx = jacobian_cases.sample_pairs("synthetic_mixed", n)
    a, b = jacobian_cases.registered(engine, m)
    return a[midx], b[midx], m["pose1"][midx], m["pose2"][midx], [("synthetic_mixed", int(i)) for i in midx]


def _mixed_batch(engine, ids, big, n_small):
    """the fixture pairs `big` followed by n_small register pairs"""
    d = huge()
    a, b, p1, p2, small = _small_pairs(engine, n_small)
    s1 = np.concatenate([ids[0][big], a]).astype(np.int32)
    s2 = np.concatenate([ids[1][big], b]).astype(np.int32)
    return s1, s2, np.vstack([d["pose1"][big], p1]), np.vstack([d["pose2"][big], p2]), small


def _run_plan(engine, plan, p1, p2, jacobian, guard=False):
    """plan.run(grad="fd", contact) -> outputs as numpy ([B, ...]); guard: jac is rows 48..96
    of a [144, B] buffer of sentinels, and nothing may land outside them"""
    import torch
    from dcol_amd.engine import alloc_outputs
    dev = torch.device("cuda", engine.device)
    B = plan.B
    out = alloc_outputs(B, dev, True, True, want_jac=jacobian and not guard)
    SENT = -12345.678
    if guard:
        bigbuf = torch.full((144, B), SENT, dtype=torch.float64, device=dev)
        out["jac"] = bigbuf[48:96]
        assert out["jac"].is_contiguous()
    plan.run(soa(p1), soa(p2), tol=float(huge()["tol"]), grad="fd", contact=True, out=out, jacobian=jacobian)
    torch.cuda.synchronize(dev)
    if guard:
        host = bigbuf.cpu().numpy()
        assert np.all(host[:48] == SENT) and np.all(host[96:] == SENT), "a store outside the pairs' 48 B doubles"
        assert not np.any(host[48:96] == SENT), "a Jacobian entry nobody wrote"
    res = {k: (v.cpu().numpy().T if v.dim() == 2 else v.cpu().numpy()) for k, v in out.items()}
    if "jac" in res:
        res["jac"] = np.ascontiguousarray(res["jac"].reshape(B, 4, 12))
    return res


def _check_small(small, jac):
    for j, (name, i) in enumerate(small):
        J, cond, tol = jacobian_cases.restated(name, i)
        err = np.abs(jac[j] - J).max()
        print(f"{name}[{i}]: err {err:.2e} tol {tol:.2e} cond(H) {cond:.1e}")
        assert err <= tol or cond > 1e10, (name, i, err, tol, cond)


def test_gpu_one_pair_guarded(engine, ids):
    """B = 1, the 1,024-row pair: one wave, every slot full; only lane 0 stores."""
    d, ok = huge(), ok_pairs()
    i = ok[d["rows"][ok] == 1024][:1]
    plan = engine.plan(ids[0][i], ids[1][i], cache=False, jacobian="stream")
    assert plan.launch_form == "buckets" and plan.jacobian == "stream" and plan.jacobian
    (bk,) = plan.buckets()
    assert bk["kind"] == "solve" and bk["omax"] == 1024 and bk["lpp"] == 64
    res = _run_plan(engine, plan, d["pose1"][i], d["pose2"][i], True, guard=True)
    assert res["status"][0] == 0 and res["iters"][0] == d["iters"][i[0]]
    check_against_restatement(i, res["jac"])


def _three_streamed():
    """three streamed pairs of different (N, NSOC): polytope x polytope, capsule x polytope,
    polygon x cone"""
    d, ok = huge(), ok_pairs()
    t1, t2 = d["type"][d["s1"]], d["type"][d["s2"]]
    return np.array([int(ok[(t1[ok] == a) & (t2[ok] == b)][0]) for a, b in ((0, 0), (3, 0), (5, 2))])


def test_gpu_five_pairs_guarded(engine, ids):
    """B = 5: three streamed pairs of different (N, NSOC) and two pairs of at most 128 rows;
    streamed and dense JAC buckets side by side, nothing outside the window."""
    d = huge()
    big = _three_streamed()
    s1, s2, p1, p2, small = _mixed_batch(engine, ids, big, 2)
    plan = engine.plan(s1, s2, cache=False, jacobian="stream")
    assert plan.launch_form == "buckets"
    bks = [b for b in plan.buckets() if b["kind"] == "solve"]
    streamed = [b for b in bks if b["omax"] == 1024]
    dense = [b for b in bks if b["omax"] <= 128]
    assert sorted((b["N"], b["nsoc"]) for b in streamed) == [(4, 0), (5, 1), (6, 2)]
    assert all(b["lpp"] == 64 and b["pairs"] == 1 for b in streamed)
    assert dense and sum(b["pairs"] for b in dense) == 2 and len(streamed) + len(dense) == len(bks)
    res = _run_plan(engine, plan, p1, p2, True, guard=True)
    np.testing.assert_array_equal(res["status"], 0)
    np.testing.assert_array_equal(res["iters"][:3], d["iters"][big])
    check_against_restatement(big, res["jac"][:3])
    _check_small(small, res["jac"][3:])


def test_gpu_bitwise_against_plain_plan(engine, ids):
    """12 streamed and 8 register pairs.  On the streamed pairs, alpha, contact, grad, iters and
    status of the Jacobian run equal a plain plan's run, and so does the 8 | 16 plan run without
    DCOL_JACOBIAN (the plain streamed kernels); J of the register pairs equals J from an
    option-8 plan of those pairs alone."""
    big = selection()[::4]
    nb = len(big)
    s1, s2, p1, p2, small = _mixed_batch(engine, ids, big, 8)
    jplan = engine.plan(s1, s2, cache=False, jacobian="stream")
    with_j = _run_plan(engine, jplan, p1, p2, True)
    without_j = _run_plan(engine, jplan, p1, p2, False)
    plain = _run_plan(engine, engine.plan(s1[:nb], s2[:nb], cache=False), p1[:nb], p2[:nb], False)
    np.testing.assert_array_equal(plain["status"], 0)
    for k in KEYS:
        np.testing.assert_array_equal(bits(with_j[k][:nb]), bits(plain[k]), err_msg=f"Jacobian run: {k}")
        np.testing.assert_array_equal(bits(without_j[k][:nb]), bits(plain[k]), err_msg=f"run without DCOL_JACOBIAN: {k}")
        np.testing.assert_array_equal(bits(without_j[k][nb:]), bits(with_j[k][nb:]), err_msg=f"register pairs: {k}")
    dense = _run_plan(engine, engine.plan(s1[nb:], s2[nb:], cache=False, jacobian=True), p1[nb:], p2[nb:], True)
    np.testing.assert_array_equal(bits(with_j["jac"][nb:]), bits(dense["jac"]))
    assert np.all(np.isfinite(with_j["jac"][:nb]))


# ---------------------------------------------------------------- 4. failure rows
def test_gpu_failure_rows(engine, ids, full_run):
    d = huge()
    es = d["expect_status"]
    res = engine.solve_host(ids[0], ids[1], d["pose1"], d["pose2"], tol=float(d["tol"]), max_iter=3, grad=None,
                            jacobian="stream")
    np.testing.assert_array_equal(res.status, np.where(es == 0, 1, es))
    assert (res.status == TOO_LARGE).sum() == 2 and (res.status == UNSUPPORTED).sum() == 6
    assert np.all(np.isnan(res.jac)) and np.all(np.isnan(res.alpha))
    # the default run: the 1,025-row and case-4 pairs keep their status and NaN, finite J wherever status is 0
    np.testing.assert_array_equal(full_run.status, es)
    bad = full_run.status != 0
    assert bad.sum() == 8 and np.all(np.isnan(full_run.jac[bad]))
    assert np.all(np.isfinite(full_run.jac[~bad]))
    # and without the opt-in such pairs are too large for the Jacobian, as before
    i = np.flatnonzero(es == 0)[:4]
    res = engine.solve_host(ids[0][i], ids[1][i], d["pose1"][i], d["pose2"][i], grad=None, jacobian=True)
    assert np.all(res.status == TOO_LARGE) and np.all(np.isnan(res.jac))


# ---------------------------------------------------------------- 5. drop-in
def test_gpu_dropin_many_faces():
    """proximity_jacobian(big, box, stream=True) on a 200-face polytope: bitwise what
    solve_host(jacobian="stream") returns for the pair, and within the restatement rule."""
    from dcol_amd import default_engine
    from oracle import dcol_oracle as O
    from primitives.misc_primitive_constructor import PolytopeMRP, create_rect_prism
    from proximity.proximity_jacobian import proximity_jacobian
    rng = np.random.default_rng(11)
    A = np.vstack([np.eye(3), -np.eye(3), rng.normal(size=(194, 3))])
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    b = rng.uniform(0.4, 1.3, 200)
    big, box = PolytopeMRP(A, b), create_rect_prism(1.0, 0.6, 1.4)
    big.r, big.p = rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3)
    box.r, box.p = rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3)
    eng = default_engine()
    alpha, cp, J = proximity_jacobian(big, box, stream=True)
    assert isinstance(alpha, np.float64) and cp.shape == (3,) and J.shape == (4, 12)
    s1, s2 = eng.register_object(big), eng.register_object(box)
    p1, p2 = np.concatenate([big.r, big.p])[None], np.concatenate([box.r, box.p])[None]
    res = eng.solve_host([s1], [s2], p1, p2, max_iter=eng.max_iter, grad=None, jacobian="stream")
    assert res.status[0] == 0
    assert alpha.tobytes() == res.alpha[0].tobytes() and cp.tobytes() == res.contact[0].tobytes()
    assert J.tobytes() == res.jac[0].tobytes()
    sa = O.ShapeSpec(O.POLYTOPE, A=A, b=b)
    sb = O.ShapeSpec(O.POLYTOPE, A=np.asarray(box.A, float), b=np.asarray(box.b, float))
    al, _, x, s, z, it, dims = O.proximity(sa, big.r, big.p, sb, box.r, box.p, 1e-6)
    assert res.iters[0] == it and alpha_close(alpha, al)
    th = np.concatenate([p1[0], p2[0]])
    Jr, cond = contact_jacobian(O, sa, sb, x, s, z, th, dims)
    tol = tolerance(O, sa, sb, x, s, z, th, dims, Jr)
    err = np.abs(J - Jr).max()
    print(f"drop-in: err {err:.2e} tol {tol:.2e} cond(H) {cond:.1e}")
    assert err <= tol
    with pytest.raises(ValueError, match="128 with the contact-point Jacobian"):
        proximity_jacobian(big, box)


# ---------------------------------------------------------------- 6. argument errors
def test_gpu_argument_errors(engine, ids):
    import torch
    from dcol_amd import _lib
    from dcol_amd.engine import Plan, _np_ptr, alloc_outputs
    d = huge()
    i = _three_streamed()
    s1, s2 = np.ascontiguousarray(ids[0][i]), np.ascontiguousarray(ids[1][i])
    lib = _lib.load()
    h = ctypes.c_void_p()
    rc = lib.dcol_plan_create_ex(engine.table.handle, 3, _np_ptr(s1), _np_ptr(s2), _lib.PLAN_JACOBIAN_STREAM, ctypes.byref(h))
    assert rc == _lib.ERR_ARG and not h.value
    assert b"DCOL_PLAN_JACOBIAN" in lib.dcol_last_error()
    with pytest.raises(_lib.DcolLibraryError, match="DCOL_PLAN_SUSPEND"):
        Plan(engine.table, s1, s2, suspend=True, jacobian="stream")
    with pytest.raises(ValueError):
        engine.plan(s1, s2, cache=False, jacobian="streamed")
    # the plan cache tells the two kinds of Jacobian plan apart
    assert engine.plan(s1, s2, jacobian="stream") is not engine.plan(s1, s2, jacobian=True)
    assert engine.plan(s1, s2, jacobian="stream") is engine.plan(s1, s2, jacobian="stream")
    plan = engine.plan(s1, s2, cache=False, jacobian="stream")
    dev = torch.device("cuda", engine.device)
    out = alloc_outputs(3, dev, True, True)
    t1, t2 = soa(d["pose1"][i]), soa(d["pose2"][i])
    ptr = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    st = ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)
    rc = lib.dcol_plan_run_jac(plan.handle, ptr(t1), ptr(t2), 1e-6, 50, _lib.JACOBIAN | _lib.CONTACT, ptr(out["alpha"]),
                               ptr(out["contact"]), ptr(out["grad"]), None, ptr(out["iters"]), ptr(out["status"]), st)
    assert rc == _lib.ERR_ARG and b"jac" in lib.dcol_last_error()
    torch.cuda.synchronize(dev)


# ---------------------------------------------------------------- 7. capture
def test_gpu_streamed_jacobian_in_captured_graph(engine, ids):
    """One capture of Plan.run(jacobian=True) on a plan whose launches include a streamed JAC
    bucket (and a dense one): the replay writes bitwise what the plain launch wrote."""
    import torch
    from dcol_amd.engine import alloc_outputs
    big = _three_streamed()[:1]
    s1, s2, p1, p2, _ = _mixed_batch(engine, ids, big, 2)
    plan = engine.plan(s1, s2, cache=False, jacobian="stream")
    assert any(b["omax"] == 1024 for b in plan.buckets()) and plan.launch_form == "buckets"
    dev = torch.device("cuda", engine.device)
    t1, t2 = soa(p1), soa(p2)
    out = alloc_outputs(plan.B, dev, True, True, want_jac=True)
    s = torch.cuda.Stream(dev)
    s.wait_stream(torch.cuda.current_stream(dev))

    def step():
        plan.run(t1, t2, grad="fd", contact=True, out=out, stream=s, jacobian=True)
    step()
    s.synchronize()
    ref = {k: v.clone() for k, v in out.items()}
    assert np.all(ref["status"].cpu().numpy() == 0) and np.all(np.isfinite(ref["jac"].cpu().numpy()))
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        step()
    for v in out.values():
        v.fill_(-7 if v.dtype == torch.int32 else 12345.0)
    torch.cuda.synchronize(dev)
    with torch.cuda.stream(s):
        g.replay()
    s.synchronize()
    for k in out:
        np.testing.assert_array_equal(bits(out[k].cpu().numpy()), bits(ref[k].cpu().numpy()), err_msg=k)
