"""Pairs above 128 orthant rows on the GPU: the streamed-row kernel (csrc/dcol_kernels_stream.hip)
through Engine, plans, the record path, the codegen twin, the drop-in modules and a captured
graph.  Expected values: the reference's, from tests/golden/huge/huge_rows.npz (see
tests/test_stream_rows.py), at the project tolerances of DESIGN.md section 4."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import PKG, REPO, alpha_close, golden_files, grad_close, load_golden
from stream_cases import FAKE, HUGE, TOO_LARGE, UNSUPPORTED, bits, implicit_reference, register, soa

pytestmark = pytest.mark.gpu

XCHECK_LIB = os.path.join(PKG, "lib_xcheck", "libdcol.so")
KEYS = ("status", "iters", "alpha", "contact", "grad")


@pytest.fixture(scope="module")
def huge():
    return load_golden(HUGE)


@pytest.fixture(scope="module")
def fd_run(engine, huge):
    """the whole fixture through Engine.solve_host, FD gradient + contact (shared, not modified)"""
    s1, s2 = register(engine, huge)
    return engine.solve_host(s1, s2, huge["pose1"], huge["pose2"], tol=float(huge["tol"]), grad="fd")


# ---------------------------------------------------------------- 1. the fixture through Engine / a plan
def test_fixture_fd(huge, fd_run):
    d, res = huge, fd_run
    np.testing.assert_array_equal(res.status, d["expect_status"])
    assert (res.status == TOO_LARGE).sum() == 2 and (res.status == UNSUPPORTED).sum() >= 4
    ok = d["expect_status"] == 0
    np.testing.assert_array_equal(res.iters[ok], d["iters"][ok])
    assert np.all(alpha_close(res.alpha[ok], d["alpha"][ok]))
    assert np.all(np.abs(res.contact[ok] - d["contact"][ok]) <= 1e-6 * np.maximum(np.abs(d["contact"][ok]), 1.0))
    assert np.all(grad_close(res.grad[ok], d["grad"][ok]))
    assert np.all(np.isnan(res.alpha[~ok])) and np.all(np.isnan(res.grad[~ok]))


def test_fixture_envelope(engine, huge, fd_run):
    d = huge
    s1, s2 = register(engine, d)
    res = engine.solve_host(s1, s2, d["pose1"], d["pose2"], tol=float(d["tol"]), grad="envelope")
    ok = d["expect_status"] == 0
    np.testing.assert_array_equal(res.status, d["expect_status"])
    np.testing.assert_array_equal(res.iters[ok], d["iters"][ok])
    np.testing.assert_array_equal(bits(res.alpha[ok]), bits(fd_run.alpha[ok]))
    assert np.all(grad_close(res.grad[ok], d["grad"][ok]))


def test_fixture_implicit(engine, huge):
    d = huge
    s1, s2 = register(engine, d)
    idx = np.flatnonzero(d["expect_status"] == 0)
    res = engine.solve_host(s1[idx], s2[idx], d["pose1"][idx], d["pose2"][idx], tol=float(d["tol"]), grad="implicit")
    assert np.all(res.status == 0)
    for j, i in enumerate(idx):
        ref = implicit_reference(d, i)
        assert np.abs(res.grad[j] - ref).max() <= 1e-6 * max(np.abs(ref).max(), 1.0), (i, int(d["rows"][i]))


def test_fixture_max_iter(engine, huge):
    d = huge
    s1, s2 = register(engine, d)
    idx = np.flatnonzero(d["expect_status"] == 0)
    res = engine.solve_host(s1[idx], s2[idx], d["pose1"][idx], d["pose2"][idx], max_iter=3, grad="fd")
    assert np.all(res.status == 1) and np.all(res.iters == 3)
    assert np.all(np.isnan(res.alpha)) and np.all(np.isnan(res.grad))


# ---------------------------------------------------------------- 2. mixed plan
def test_mixed_plan_bitwise(engine, huge):
    """The fixture's pairs interleaved with 500 pairs of synthetic_mixed (B = 652, no multiple
    of 64): every slot written, the register buckets' pairs as in a plan of theirs alone, the
    streamed pairs as in a plan of theirs alone, bit for bit."""
    import torch
    from dcol_amd import alloc_outputs
    d = huge
    m = load_golden([p for p in golden_files() if p.endswith("synthetic_mixed.npz")][0])
    h1, h2 = register(engine, d)
    m1, m2 = register(engine, m)
    nh, nm = len(h1), 500
    B = nh + nm
    assert B % 64 != 0
    pos_h = np.round(np.linspace(0, B - 1, nh)).astype(int)      # the fixture's pairs spread through the batch
    is_h = np.zeros(B, bool)
    is_h[pos_h] = True
    s1, s2, p1, p2 = np.empty(B, np.int32), np.empty(B, np.int32), np.empty((B, 6)), np.empty((B, 6))
    s1[is_h], s2[is_h], p1[is_h], p2[is_h] = h1, h2, d["pose1"], d["pose2"]
    s1[~is_h], s2[~is_h], p1[~is_h], p2[~is_h] = m1[:nm], m2[:nm], m["pose1"][:nm], m["pose2"][:nm]

    def run(sel):
        plan = engine.plan(s1[sel], s2[sel], cache=False)
        n = int(sel.sum())
        out = alloc_outputs(n, torch.device("cuda", 0))
        for k, v in out.items():                                  # sentinels: a slot nobody writes keeps them
            v.fill_(-7 if v.dtype == torch.int32 else 12345.0)
        plan.run(soa(p1[sel]), soa(p2[sel]), grad="fd", out=out)
        torch.cuda.synchronize()
        return plan, {k: (v.cpu().numpy().T if v.dim() == 2 else v.cpu().numpy()) for k, v in out.items()}

    plan, mixed = run(np.ones(B, bool))
    assert plan.launch_form == "buckets"
    streamed = [b for b in plan.buckets() if b["kind"] == "solve" and b["omax"] == 1024]
    assert sorted((b["N"], b["nsoc"]) for b in streamed) == [(4, 0), (4, 1), (5, 1), (6, 1), (6, 2)]
    assert all(b["lpp"] == 64 for b in streamed) and sum(b["pairs"] for b in streamed) == int((d["expect_status"] == 0).sum())
    assert not np.any(mixed["status"] == -7) and not np.any(mixed["iters"] == -7)
    for k in ("alpha", "contact", "grad"):
        assert not np.any(mixed[k] == 12345.0), k
    np.testing.assert_array_equal(mixed["status"][is_h], d["expect_status"])
    np.testing.assert_array_equal(mixed["status"][~is_h], m["status"][:nm])
    _, small = run(~is_h)
    _, big = run(is_h)
    for k in KEYS:
        np.testing.assert_array_equal(bits(mixed[k][~is_h]), bits(small[k]), err_msg=f"register buckets: {k}")
        np.testing.assert_array_equal(bits(mixed[k][is_h]), bits(big[k]), err_msg=f"streamed buckets: {k}")


# ---------------------------------------------------------------- 3. record path
def test_record_path(engine, huge):
    """rec set and the SoA outputs null (dcol_prox_batch_multi_gpu in place, records only): the
    14-double records equal the SoA run's values bitwise."""
    import torch
    from dcol_amd.dist import REC, NativeComm, unpack
    d = huge
    s1, s2 = register(engine, d)
    plan = engine.plan(s1, s2, cache=False)
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


def test_record_path_world2(huge, monkeypatch):
    """The same at world 2 over the in-process collective stand-in (tests/fake_rccl; the ranks
    are host threads, as in tests/test_native_ranks.py): each rank's gathered buffer holds both
    shards' records, equal bitwise to the shards solved by themselves."""
    import threading

    import torch
    from dcol_amd import Engine, spec_from_arrays
    from dcol_amd.dist import REC, NativeComm, pack
    monkeypatch.setenv("DCOL_RCCL_LIB", FAKE)
    d = huge
    B, world = len(d["s1"]), 2
    idx = [np.arange(r, B, world) for r in range(world)]
    cap = max(len(i) for i in idx) + 1
    uid = NativeComm.unique_id()
    results, refs, errors = [None] * world, [None] * world, []
    barrier = threading.Barrier(world)

    def rank_fn(r):
        try:
            torch.cuda.set_device(0)
            eng = Engine(device=0)
            ids = np.array([eng.register(spec_from_arrays(d, k)) for k in range(len(d["type"]))], np.int32)
            mine = idx[r]
            plan = eng.plan(ids[d["s1"][mine]], ids[d["s2"][mine]])
            p1, p2 = soa(d["pose1"][mine]), soa(d["pose2"][mine])
            st = torch.cuda.Stream()
            comm = NativeComm(uid, world, r, 0)
            try:
                g = torch.full((world * cap, REC), 5.0, dtype=torch.float64, device="cuda")
                barrier.wait()
                comm.solve_gather(plan, p1, p2, cap, grad="fd", stream=st, rec_all=g, in_place=True, soa=False)
                torch.cuda.synchronize()
                ref = plan.run(p1, p2, grad="fd", contact=False, stream=st)
                st.synchronize()
            finally:
                comm.close()
            results[r] = g.cpu().numpy()
            refs[r] = pack(ref["alpha"].cpu().numpy(), ref["grad"].cpu().numpy().T, ref["status"].cpu().numpy(),
                           ref["iters"].cpu().numpy())
        except BaseException as e:   # reported by the main thread
            errors.append(f"rank {r}: {type(e).__name__}: {e}")
            barrier.abort()

    threads = [threading.Thread(target=rank_fn, args=(r,)) for r in range(world)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not any(t.is_alive() for t in threads), "a rank thread hung"
    assert not errors, errors
    expected = np.empty((world * cap, REC))
    expected.view(np.uint64)[:] = np.uint64(0xFFFFFFFFFFFFFFFF)
    for r in range(world):
        expected[r * cap:r * cap + len(idx[r])] = refs[r]
    for r in range(world):
        np.testing.assert_array_equal(results[r].view(np.uint64), expected.view(np.uint64), err_msg=f"rank {r}")


# ---------------------------------------------------------------- 4. codegen twin
_TWIN_SCRIPT = r"""
import sys, numpy as np
sys.path[:0] = [sys.argv[2], sys.argv[3]]
from dcol_amd import Engine, spec_from_arrays
d = dict(np.load(sys.argv[4]))
eng = Engine(device=0)
ids = np.array([eng.register(spec_from_arrays(d, k)) for k in range(len(d["type"]))], np.int32)
out = {}
for mode in ("fd", "envelope", "implicit"):
    r = eng.solve_host(ids[d["s1"]], ids[d["s2"]], d["pose1"], d["pose2"], tol=float(d["tol"]), grad=mode)
    out.update({f"{mode}_{k}": getattr(r, k) for k in ("status", "iters", "alpha", "contact", "grad")})
np.savez(sys.argv[1], **out)
"""


@pytest.mark.skipif(not os.path.exists(XCHECK_LIB), reason="lib_xcheck not built (make -C csrc xcheck)")
def test_codegen_twin(tmp_path, engine, huge, fd_run):
    """lib_xcheck -- the same sources under the other machine schedule -- agrees bitwise with
    the product library on the fixture, in the three gradient modes."""
    env = {k: v for k, v in os.environ.items() if k not in ("DCOL_NO_BALL", "DCOL_NO_CONE", "DCOL_LPP")}
    env["DCOL_LIB"] = XCHECK_LIB
    f = str(tmp_path / "twin.npz")
    subprocess.run([sys.executable, "-c", _TWIN_SCRIPT, f, PKG, REPO, HUGE], check=True, env=env, timeout=300)
    twin = dict(np.load(f))
    d = huge
    s1, s2 = register(engine, d)
    for mode in ("fd", "envelope", "implicit"):
        r = fd_run if mode == "fd" else engine.solve_host(s1, s2, d["pose1"], d["pose2"], tol=float(d["tol"]), grad=mode)
        for k in KEYS:
            np.testing.assert_array_equal(bits(getattr(r, k)), bits(twin[f"{mode}_{k}"]), err_msg=f"{mode} {k}")


# ---------------------------------------------------------------- 5. drop-in
def test_dropin_many_faces():
    """proximity_mrp / proximity_gradient on a 200-face PolytopeMRP against a box and against a
    sphere return the oracle's values and the reference's types, by plain one-pair launches
    (the resident pair server has no streamed case and is not started for them);
    proximity_jacobian says it stops at 128 rows."""
    from dcol_amd import default_engine
    from oracle import dcol_oracle as O
    from primitives.misc_primitive_constructor import PolytopeMRP, SphereMRP, create_rect_prism
    from proximity.proximity import proximity_mrp
    from proximity.proximity_gradient import proximity_gradient
    from proximity.proximity_jacobian import proximity_jacobian
    rng = np.random.default_rng(11)
    A = np.vstack([np.eye(3), -np.eye(3), rng.normal(size=(194, 3))])
    A /= np.linalg.norm(A, axis=1, keepdims=True)
    b = rng.uniform(0.4, 1.3, 200)
    big, box, sph = PolytopeMRP(A, b), create_rect_prism(1.0, 0.6, 1.4), SphereMRP(0.5)
    eng = default_engine()
    for o in (big, box, sph):
        eng.register_object(o)
    before = eng.pair_stats()
    calls = 0
    for other, spec in ((box, O.ShapeSpec(O.POLYTOPE, A=np.asarray(box.A, float), b=np.asarray(box.b, float))),
                        (sph, O.ShapeSpec(O.SPHERE, R=0.5))):
        for first in (True, False):
            big.r, big.p = rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3)
            other.r, other.p = rng.uniform(-3, 3, 3), rng.uniform(-1, 1, 3)
            pa, pb = (big, other) if first else (other, big)
            sa, sb = (O.ShapeSpec(O.POLYTOPE, A=A, b=b), spec) if first else (spec, O.ShapeSpec(O.POLYTOPE, A=A, b=b))
            ref_a, ref_g, x, *_ = O.proximity_gradient(sa, pa.r, pa.p, sb, pb.r, pb.p)
            alpha, cp = proximity_mrp(pa, pb)
            alpha2, g = proximity_gradient(pa, pb)
            calls += 2
            assert isinstance(alpha, np.float64) and isinstance(cp, np.ndarray) and cp.shape == (3,)
            assert isinstance(alpha2, np.float64) and isinstance(g, np.ndarray) and g.shape == (12,)
            assert alpha == alpha2 and alpha_close(alpha, ref_a)
            assert np.all(np.abs(cp - x[:3]) <= 1e-6 * np.maximum(np.abs(x[:3]), 1.0))
            assert grad_close(g, ref_g)
    after = eng.pair_stats()
    assert after["server_starts"] == before["server_starts"]
    assert after["launched"] - before["launched"] == calls and after["served"] == before["served"]
    with pytest.raises(ValueError, match="128 with the contact-point Jacobian"):
        proximity_jacobian(big, box)


# ---------------------------------------------------------------- 6. capture
def test_streamed_bucket_in_captured_graph(engine, huge):
    """A plan run whose one launch is a streamed bucket (the fixture's polytope x polytope
    pairs) captured into a graph on a side stream: the replay writes bitwise what the plain
    run wrote (dcol_plan_run allocates nothing while capturing)."""
    import torch
    from dcol_amd import alloc_outputs
    d = huge
    s1, s2 = register(engine, d)
    t1, t2 = d["type"][d["s1"]], d["type"][d["s2"]]
    sel = (d["expect_status"] == 0) & (t1 == 0) & (t2 == 0)
    plan = engine.plan(s1[sel], s2[sel], cache=False)
    assert plan.num_launches == 1 and plan.launch_form == "buckets" and plan.buckets()[0]["omax"] == 1024
    dev = torch.device("cuda", 0)
    p1, p2 = soa(d["pose1"][sel]), soa(d["pose2"][sel])
    out = alloc_outputs(plan.B, dev)
    s = torch.cuda.Stream(dev)
    step = plan.bind(p1, p2, out, grad="fd", contact=True, stream=s)
    s.wait_stream(torch.cuda.current_stream(dev))
    step()
    s.synchronize()
    ref = {k: v.clone() for k, v in out.items()}
    np.testing.assert_array_equal(ref["iters"].cpu().numpy(), d["iters"][sel])
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
