"""The drop-in Python boundary, exercised the way the reference's callers use it.

The reference's system modules bind the two proximity functions by module path at import
time (piano_mover.py:2-3, cluttered_hallway_quadrotor.py:5-6, cone_through_wall.py:4-5),
build primitives with the constructors of primitives/misc_primitive_constructor.py, and
overwrite ``.r`` / ``.p`` before every call (piano_mover.py:60-61, :84-85).  These tests do
exactly that with this repository's classes and modules, against the golden vectors the
reference produced (tests/golden/gen_golden.py):

* ``proximity_mrp(prim1, prim2, pdip_tol)`` -> (np.float64 alpha, ndarray(3) contact)
  (/root/reference/proximity/proximity.py:6, :51-54);
* ``proximity_gradient(prim1, prim2, pdip_tol)`` -> (np.float64 alpha, ndarray(12) grad)
  (/root/reference/proximity/proximity_gradient.py:91, :133-138);
* the exceptions: a bare ``Exception`` after the 50-iteration cap (pdip.py:470), ``ValueError``
  for case-4 pairs (combine_problem_matrices.py:58-70), and the unpacking ``TypeError`` of an
  unknown object (problem_matrices.py returns None, proximity.py:23);
* the pose / shape ownership contract of dcol_amd.Engine (poses read at every call, shape
  fields snapshotted until ``forget``).

GPU tests call the HIP library through the C-ABI (dcol_prox_batch_host); the TypeError test
raises before any device call and runs on the CPU.
"""
import numpy as np
import pytest

from conftest import alpha_close, golden_files, grad_close, load_golden
from dropin_objects import objects_from_golden, pose_pair

GOLDEN = {p.split("/")[-1][:-4]: p for p in golden_files()}
# per-pair calls: a spread of pairs from every family (each call is one host round trip)
PER_PAIR = 24


def spread(idx, n):
    idx = np.asarray(idx)
    return idx[np.linspace(0, idx.size - 1, min(n, idx.size)).astype(int)] if idx.size else idx


def test_unknown_object_raises_typeerror():
    """problem_matrices() returns None for an unknown class and the caller's tuple unpacking
    raises TypeError (proximity.py:23); raised before any device work."""
    from primitives.misc_primitive_constructor import SphereMRP
    from proximity.proximity import proximity_mrp
    from proximity.proximity_gradient import proximity_gradient

    class Blob:
        r = np.zeros(3)
        p = np.zeros(3)

    with pytest.raises(TypeError):
        proximity_mrp(SphereMRP(1.0), Blob())
    with pytest.raises(TypeError):
        proximity_gradient(Blob(), SphereMRP(1.0))


def test_callers_bind_by_module_path():
    """`from proximity.proximity import proximity_mrp` (the systems' import lines) resolves to
    this package's drop-in, and the constructors the systems import exist with the
    reference's signatures."""
    import inspect

    from primitives import misc_primitive_constructor as mpc
    from proximity.proximity import proximity_mrp
    from proximity.proximity_gradient import proximity_gradient
    assert list(inspect.signature(proximity_mrp).parameters) == ["prim1", "prim2", "pdip_tol", "verbose"]
    assert list(inspect.signature(proximity_gradient).parameters) == ["prim1", "prim2", "pdip_tol", "verbose"]
    assert inspect.signature(proximity_mrp).parameters["pdip_tol"].default == 1e-6
    for name in ("SphereMRP", "PolytopeMRP", "ConeMRP", "CapsuleMRP", "CylinderMRP", "PolygonMRP",
                 "create_rect_prism", "create_n_sided"):
        assert callable(getattr(mpc, name))
    assert "dcol_amd" in proximity_mrp.__module__ or proximity_mrp.__module__ == "proximity.proximity"


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_piano", "scene_quad", "scene_cone", "synthetic_mixed", "edge_cases",
                                  "large_polytopes"])
def test_per_pair_calls_match_golden(engine, name):
    """proximity_mrp and proximity_gradient, one call per pair on primitive objects, against
    the reference's golden alpha / contact / gradient; unsupported (case-4) pairs raise
    ValueError from both."""
    from proximity.proximity import proximity_mrp
    from proximity.proximity_gradient import proximity_gradient
    d = load_golden(GOLDEN[name])
    objs = objects_from_golden(d)
    tol = float(d["tol"])
    ok = np.flatnonzero(d["status"] == 0)
    for i in spread(ok, PER_PAIR):
        a, b = pose_pair(objs, d, i)
        alpha, cp = proximity_mrp(a, b, pdip_tol=tol)
        assert isinstance(alpha, np.float64)
        assert isinstance(cp, np.ndarray) and cp.shape == (3,) and cp.dtype == np.float64
        assert alpha_close(alpha, d["alpha"][i]), (i, alpha, d["alpha"][i])
        assert np.all(np.abs(cp - d["contact"][i]) <= 1e-6 * np.maximum(np.abs(d["contact"][i]), 1.0))
        alpha2, g = proximity_gradient(a, b, pdip_tol=tol)
        assert isinstance(alpha2, np.float64)
        assert isinstance(g, np.ndarray) and g.shape == (12,) and g.dtype == np.float64
        assert alpha_close(alpha2, d["alpha"][i])
        assert grad_close(g, d["grad"][i]), (i, g, d["grad"][i])
    for i in spread(np.flatnonzero(d["status"] == 2), 6):       # combine_problem_matrices.py:58-70
        a, b = pose_pair(objs, d, i)
        with pytest.raises(ValueError):
            proximity_mrp(a, b, pdip_tol=tol)
        with pytest.raises(ValueError):
            proximity_gradient(a, b, pdip_tol=tol)


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["scene_quad", "synthetic_mixed", "synthetic_polypoly"])
def test_batch_forms_match_golden(engine, name):
    """proximity_mrp_batch / proximity_gradient_batch over a whole golden set of objects."""
    import copy

    from proximity.proximity import proximity_mrp_batch
    from proximity.proximity_gradient import proximity_gradient_batch
    d = load_golden(GOLDEN[name])
    objs = objects_from_golden(d)
    p1, p2 = [], []
    for i in range(d["s1"].size):
        a, b = copy.copy(objs[int(d["s1"][i])]), copy.copy(objs[int(d["s2"][i])])   # shallow: shared shape data
        a.r, a.p = d["pose1"][i, :3], d["pose1"][i, 3:]
        b.r, b.p = d["pose2"][i, :3], d["pose2"][i, 3:]
        p1.append(a)
        p2.append(b)
    tol = float(d["tol"])
    alpha, cp, st = proximity_mrp_batch(p1, p2, pdip_tol=tol)
    np.testing.assert_array_equal(st, d["status"])
    ok = d["status"] == 0
    assert np.all(alpha_close(alpha[ok], d["alpha"][ok]))
    assert np.all(np.abs(cp[ok] - d["contact"][ok]) <= 1e-6 * np.maximum(np.abs(d["contact"][ok]), 1.0))
    assert np.all(np.isnan(alpha[~ok]))
    for mode in ("fd", "envelope"):
        alpha2, g, st2 = proximity_gradient_batch(p1, p2, pdip_tol=tol, grad=mode)
        np.testing.assert_array_equal(st2, d["status"])
        assert np.all(alpha_close(alpha2[ok], d["alpha"][ok]))
        assert np.all(grad_close(g[ok], d["grad"][ok]))


@pytest.mark.gpu
def test_iteration_cap_raises_bare_exception(engine):
    """pdip.py:470 raises a bare Exception after its iteration cap; the drop-in raises a
    subclass of Exception (PDIPFailure).  The cap is the literal 50, reached by no golden pair,
    so the default engine's cap is lowered for the call."""
    from dcol_amd import PDIPFailure, default_engine
    from proximity.proximity import proximity_mrp
    from proximity.proximity_gradient import proximity_gradient
    d = load_golden(GOLDEN["synthetic_polypoly"])
    objs = objects_from_golden(d)
    a, b = pose_pair(objs, d, 0)
    eng = default_engine()
    saved = eng.max_iter
    try:
        eng.max_iter = 2
        with pytest.raises(Exception) as ei:
            proximity_mrp(a, b)
        assert isinstance(ei.value, PDIPFailure) and not isinstance(ei.value, (ValueError, TypeError))
        with pytest.raises(PDIPFailure):
            proximity_gradient(a, b)
    finally:
        eng.max_iter = saved
    alpha, _ = proximity_mrp(a, b)
    assert alpha_close(alpha, d["alpha"][0])


@pytest.mark.gpu
def test_pose_and_shape_ownership(engine):
    """Poses are read at every call (callers overwrite .r/.p); shape fields are snapshotted
    the first time an object is seen, so an in-place shape edit needs Engine.forget()."""
    from dcol_amd import default_engine
    from primitives.misc_primitive_constructor import SphereMRP, create_rect_prism
    from proximity.proximity import proximity_mrp
    from proximity.proximity_gradient import proximity_gradient
    box = create_rect_prism(1.0, 1.0, 1.0)
    ball = SphereMRP(0.5)
    box.r, box.p = [0.0, 0.0, 0.0], [0.0, 0.0, 0.0]
    ball.r, ball.p = np.array([3.0, 0.0, 0.0]), np.zeros(3)
    a1, _ = proximity_mrp(ball, box)
    # alpha scales both primitives about their centres: touching when alpha (0.5 + 0.5) = 3
    assert abs(a1 - 3.0) < 1e-5
    ball.r = np.array([5.0, 0.0, 0.0])
    a2, g2 = proximity_gradient(ball, box)
    assert abs(a2 - 5.0) < 1e-5 and a2 > a1
    assert abs(g2[0] - 1.0) < 1e-4 and abs(g2[6] + 1.0) < 1e-4          # d alpha / d r1_x, d r2_x
    ball.R = 1.5                                                        # in-place shape edit
    a3, _ = proximity_mrp(ball, box)
    assert a3 == a2                                                     # snapshot still used
    default_engine().forget(ball)
    a4, _ = proximity_mrp(ball, box)
    assert abs(a4 - 2.5) < 1e-5                                         # 5 / (1.5 + 0.5)


def _bits(results):
    """(alpha, contact, grad, iters, status) tuples -> one uint64 array (NaN-exact)"""
    rows = []
    for a, cp, g, it, st in results:
        rows.append(np.concatenate([[a], cp if cp is not None else [], g if g is not None else [],
                                    [float(it), float(st)]]))
    return np.array(rows).view(np.uint64)


@pytest.mark.gpu
@pytest.mark.parametrize("idle_us", [1000, 20])
def test_pair_server_bitwise_launch_path(engine, monkeypatch, idle_us):
    """dcol_prox_pair's one-pair server (csrc/dcol_kernels_server.hip: one resident workgroup
    polling a device-mapped mailbox, no launch per call) returns bitwise what one launch per
    call returns (DCOL_PAIR_SERVER=0), for pairs of every golden scene / mixed / edge set,
    with proximity_mrp's flags and proximity_gradient's (fd and envelope: a flag change
    restarts the server).  idle 20 us: the server leaves between most calls, so its exit /
    restart handshake runs hundreds of times; 1000 us: it stays resident (no restarts)."""
    monkeypatch.setenv("DCOL_PAIR_SERVER_IDLE_US", str(idle_us))
    for name in ("scene_quad", "scene_cone", "scene_piano", "synthetic_mixed", "edge_cases"):
        d = load_golden(GOLDEN[name])
        objs = objects_from_golden(d)
        tol = float(d["tol"])
        idx = spread(np.arange(d["s1"].size), 60)
        for i in idx:                                 # register every shape first (table fixed below)
            engine.solve_pair(*pose_pair(objs, d, i), tol, grad=None)
        for grad in (None, "fd", "envelope"):
            res = {}
            for server in ("1", "0"):
                monkeypatch.setenv("DCOL_PAIR_SERVER", server)
                s0 = engine.pair_stats()
                res[server] = [engine.solve_pair(*pose_pair(objs, d, i), tol, grad=grad, contact=True) for i in idx]
                s1 = engine.pair_stats()
                if server == "1":    # the supported pairs went through the server
                    assert s1["served"] - s0["served"] >= int(np.sum(d["status"][idx] == 0)) // 2, (name, s0, s1)
                else:
                    assert s1["served"] == s0["served"]
            np.testing.assert_array_equal(_bits(res["1"]), _bits(res["0"]), err_msg=f"{name} grad={grad}")
            st = np.array([r[4] for r in res["1"]])
            np.testing.assert_array_equal(st, d["status"][idx])


@pytest.mark.gpu
def test_pair_server_idle_exit_and_restart(engine, monkeypatch):
    """The server leaves after its idle time (the stream drains: a device synchronise
    returns) and the next call starts a new one.  Calls alternating proximity_mrp /
    proximity_gradient flags call by call: the server keeps one kind's flags and the other
    kind takes the launch path (a restart needs two calls in a row with other flags); a run
    of one kind (an ALTRO phase) restarts it with that kind's flags.  Every answer bitwise
    equal to the first one."""
    import time

    import torch
    from primitives.misc_primitive_constructor import SphereMRP, create_rect_prism
    monkeypatch.setenv("DCOL_PAIR_SERVER", "1")
    monkeypatch.setenv("DCOL_PAIR_SERVER_IDLE_US", "200")
    box = create_rect_prism(1.0, 2.0, 0.5)
    ball = SphereMRP(0.4)
    box.r, box.p = np.zeros(3), np.array([0.1, -0.2, 0.3])
    ball.r, ball.p = np.array([2.0, 0.5, -0.3]), np.zeros(3)
    ref_m = engine.solve_pair(ball, box, grad=None)
    ref_g = engine.solve_pair(ball, box, grad="fd")
    s0 = engine.pair_stats()
    for k in range(20):
        m = engine.solve_pair(ball, box, grad=None)
        g = engine.solve_pair(ball, box, grad="fd")
        np.testing.assert_array_equal(_bits([m]), _bits([ref_m]))
        np.testing.assert_array_equal(_bits([g]), _bits([ref_g]))
        if k % 5 == 4:
            time.sleep(0.002)                         # > the idle time: the server has left
            t0 = time.perf_counter()
            torch.cuda.synchronize()
            assert time.perf_counter() - t0 < 0.5
    s1 = engine.pair_stats()
    served, launched = s1["served"] - s0["served"], s1["launched"] - s0["launched"]
    assert served + launched == 40 and served >= 20, (served, launched)
    # a phase of gradient calls: at most one launched call, then the server has their flags
    for k in range(6):
        np.testing.assert_array_equal(_bits([engine.solve_pair(ball, box, grad="fd")]), _bits([ref_g]))
    s2 = engine.pair_stats()
    assert s2["served"] - s1["served"] >= 5 and s2["launched"] - s1["launched"] <= 1, (s1, s2)


@pytest.mark.gpu
def test_pair_server_two_threads(engine):
    """Two threads calling the drop-in on one engine (the fast path takes no Python lock: the
    library serialises the calls per table): every answer bitwise equal to the same call made
    alone, and equal to the reference's golden values."""
    import copy
    import threading
    d = load_golden(GOLDEN["scene_quad"])
    ok = np.flatnonzero(d["status"] == 0)
    tol = float(d["tol"])
    sets = []
    for part in (ok[0::2][:40], ok[1::2][:40]):
        objs = objects_from_golden(d)
        sets.append([copy.deepcopy(pose_pair(objs, d, i)) + (i,) for i in part])
    ref = {}
    for s in sets:
        for a, b, i in s:
            ref[i] = engine.solve_pair(a, b, tol, grad="fd", contact=False)
    got, errors = {}, []

    def worker(s):
        try:
            for _ in range(3):
                for a, b, i in s:
                    got.setdefault(i, []).append(engine.solve_pair(a, b, tol, grad="fd", contact=False))
        except BaseException as e:   # reported by the main thread
            errors.append(repr(e))

    threads = [threading.Thread(target=worker, args=(s,)) for s in sets]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=120)
    assert not errors, errors
    for i, rs in got.items():
        for r in rs:
            np.testing.assert_array_equal(_bits([r]), _bits([ref[i]]))
        assert alpha_close(rs[0][0], d["alpha"][i]) and grad_close(rs[0][2], d["grad"][i])


def _child(mode, env_extra, timeout=240):
    import os
    import subprocess
    import sys
    import time
    here = os.path.dirname(os.path.abspath(__file__))
    env = dict(os.environ, **env_extra)
    t0 = time.monotonic()
    p = subprocess.run([sys.executable, os.path.join(here, "server_exit_child.py"), mode], capture_output=True,
                       text=True, timeout=timeout, env=env)
    return p, time.monotonic() - t0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["python", "c"])
def test_pair_server_stopped_at_process_exit(mode):
    """A process that makes drop-in calls and exits without destroying its tables while the
    one-pair server is resident (idle time 60 s): the server is stopped at exit -- by the
    binding's atexit hook (dcol_amd/_lib.py) on a normal Python exit, or, when the process
    leaves through C exit() with no Python teardown at all, by the library's own exit handler
    (dcol_shutdown, registered at the first server start) -- so the process neither tears
    its HIP context down under a polling wave nor waits out the idle time.  Then a fresh
    process opens the device, solves pairs and stops its own server."""
    env = {"DCOL_PAIR_SERVER": "1", "DCOL_PAIR_SERVER_IDLE_US": "60000000", "DCOL_DEBUG_SHUTDOWN": "1"}
    p, took = _child(mode, env)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "CHILD_OK" in p.stdout and "running=1" in p.stdout, p.stdout + p.stderr
    reports = [ln for ln in p.stderr.splitlines() if ln.startswith("dcol_shutdown:")]
    # the first dcol_shutdown of the exit found the resident server and stopped it
    assert reports and "1 pair servers running, 1 stopped, 0 did not stop" in reports[0], p.stderr
    assert len(reports) == (2 if mode == "python" else 1), reports
    assert took < 45, took       # the idle time (60 s) was not waited out
    q, _ = _child("reopen", {"DCOL_PAIR_SERVER": "1", "DCOL_DEBUG_SHUTDOWN": "1"})
    assert q.returncode == 0, q.stdout + q.stderr
    assert "CHILD_OK mode=reopen" in q.stdout and "served=" in q.stdout, q.stdout + q.stderr
    alpha = lambda out: float(out.split("alpha0=")[1].split()[0].replace("np.float64(", "").rstrip(")"))  # noqa: E731
    assert alpha(p.stdout) == alpha(q.stdout)


@pytest.mark.gpu
def test_pair_server_gives_way_to_batch_plans(engine, monkeypatch):
    """A batch plan launched while the one-pair server is resident makes it leave (a kernel
    resident beside a batch plan slowed it 1.3-2x, tools/server_tax.py): the plan (100k poly x
    poly pairs, bench configs[3]) then takes the time it takes with the server stopped, its
    results are bitwise the same, the server has left after the launch and the next drop-in
    call starts a new one and answers bitwise as before.  The drop-in's own launch path (a
    call with other flags) does not make its server leave."""
    import torch
    from bench import pairs, shape_table
    from dcol_amd import alloc_outputs, spec_from_arrays
    from primitives.misc_primitive_constructor import SphereMRP, create_rect_prism
    monkeypatch.setenv("DCOL_PAIR_SERVER", "1")
    monkeypatch.setenv("DCOL_PAIR_SERVER_IDLE_US", "30000000")
    tab = shape_table()
    ids = np.array([engine.register(spec_from_arrays(tab, k)) for k in range(len(tab["type"]))], np.int32)
    box = create_rect_prism(1.0, 2.0, 0.5)
    ball = SphereMRP(0.4)
    box.r, box.p = np.zeros(3), np.array([0.1, -0.2, 0.3])
    ball.r, ball.p = np.array([2.0, 0.5, -0.3]), np.zeros(3)
    ref_pair = engine.solve_pair(ball, box, grad=None)   # registers both: the table is final now
    B = 100_000
    s1, s2, p1, p2 = pairs(B, len(tab["type"]), seed=3)
    plan = engine.plan(ids[s1], ids[s2], cache=False)
    dev = torch.device("cuda", engine.device)
    d1 = torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev)
    d2 = torch.from_numpy(np.ascontiguousarray(p2.T)).to(dev)
    out = alloc_outputs(B, dev, want_grad=True, want_contact=False)
    stream = torch.cuda.current_stream(dev)
    run = plan.bind(d1, d2, out, grad="fd", contact=False, stream=stream)

    def timed(n=40):
        ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(n)]
        for a, b in ev:
            a.record(stream)
            run()
            b.record(stream)
        ev[-1][1].synchronize()
        return float(np.median([a.elapsed_time(b) for a, b in ev]))

    for _ in range(60):                               # clocks up
        run()
    stream.synchronize()
    ref = {k: v.clone() for k, v in out.items()}
    t = {"stopped": [], "resident": []}
    for rep in range(3):
        engine.stop_pair_server()
        assert not engine.pair_server_running()
        t["stopped"].append(timed())
        np.testing.assert_array_equal(_bits([engine.solve_pair(ball, box, grad=None)]), _bits([ref_pair]))
        assert engine.pair_server_running()           # resident (30 s idle) when the plans start
        t["resident"].append(timed())
        assert not engine.pair_server_running()       # it left at the first launch
        for k, v in out.items():
            assert torch.equal(v, ref[k]), k
    # the launch path (other flags) keeps the server
    np.testing.assert_array_equal(_bits([engine.solve_pair(ball, box, grad=None)]), _bits([ref_pair]))
    assert engine.pair_server_running()
    engine.solve_pair(ball, box, grad="envelope")     # mismatching flags: launched, server stays
    assert engine.pair_server_running()
    # a small plan (latency-bound: cannot fill the GPU) on a stream of its own leaves the
    # server resident, so a caller interleaving small batches with drop-in calls does not
    # restart it at every pair call (made, with its buffers, while no server is resident:
    # synchronous HIP calls wait for the server's blocking stream; a null-stream launch makes
    # it leave, dcol_capi.cpp plan_run_rec)
    engine.stop_pair_server()
    small = engine.plan(ids[s1[:200]], ids[s2[:200]], cache=False)
    sd1, sd2 = d1[:, :200].contiguous(), d2[:, :200].contiguous()
    sout = alloc_outputs(200, dev, want_grad=True, want_contact=False)
    side = torch.cuda.Stream(dev)
    assert small.launch_form == "buckets" and small.num_launches == 1
    np.testing.assert_array_equal(_bits([engine.solve_pair(ball, box, grad=None)]), _bits([ref_pair]))
    starts0 = engine.pair_stats()["server_starts"]
    for i in range(20):
        small.run(sd1, sd2, grad="fd", contact=False, out=sout, stream=side)
        side.synchronize()
        assert engine.pair_server_running(), i
        np.testing.assert_array_equal(_bits([engine.solve_pair(ball, box, grad=None)]), _bits([ref_pair]))
        assert engine.pair_stats()["server_starts"] == starts0, (i, engine.pair_stats())
    assert engine.pair_server_running()
    engine.stop_pair_server()
    stopped, resident = min(t["stopped"]), min(t["resident"])
    print(f"server_yield: batch ms stopped {t['stopped']} server resident at launch {t['resident']} "
          f"ratio {resident / stopped:.4f}")
    # a loose bound: the functional checks above are the test; the ratio itself (0.98 measured,
    # DESIGN.md section 1) is a performance figure that shader-clock swings move by a few %
    assert resident / stopped < 1.25, t
