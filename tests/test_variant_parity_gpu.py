"""Every compiled copy of the solver on the device against the oracle: the cases of
tests/variant_cases.py (which tests/test_variant_ledger.py shows to launch every copy of
csrc/variants.py that a plan can launch), one fresh process and one Engine per environment
group (tests/variant_child.py), 67 pairs per bucket.

Per case the parent holds the child's record to
* the layout: Plan.buckets(), launch_form and num_launches equal the x86 policy's for the
  device's SIMD count, and launch the copies the CPU ledger counts for the case;
* cases 1-3, the C oracle: status equal on every pair, Newton iteration counts equal, alpha
  within 1e-9 relative and the FD gradient within 2e-6 of max(|g|_inf, 1) (the bounds of
  tests/test_gpu_stress.py), the envelope gradient within conftest.grad_close of the oracle's FD
  gradient;
* DCOL_PLAN_CASE4 cases, the NumPy oracle's extension (recorded: variant_cases.reference) with
  conftest.alpha_close / grad_close, as tests/test_case4.py;
* Jacobian cases: the above, and J within contact_jacobian_ref.tolerance of the restatement on
  every pair, a pair above it only with cond(H) > 1e10 (the filter of
  tests/test_contact_jacobian.py; at most 10 % of a copy's pairs, held on the CPU by
  test_variant_ledger.py::test_jacobian_cases_are_well_conditioned);
* server cases: each dcol_prox_pair answer bit for bit the pair's result in the fused plan of
  the case's two pairs, every call answered by the resident server.
Each group prints, per form, the copies it launched and the worst alpha and gradient error."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import variant_cases as VC
import variant_ledger as VL
from conftest import alpha_close, gpu_available, grad_close

GROUPS = VC.env_groups()
ALPHA_RTOL, GRAD_TOL, COND_MAX = 1e-9, 2e-6, 1e10
# what a device fault looks like when the child reports it as a Python error and ends with status 1
FAULT_WORDS = ("illegal memory access", "HSA_STATUS_ERROR", "hipErrorLaunchFailure", "unspecified launch failure",
               "Memory access fault")


def run_child(env, path):
    import emul_lib
    emul_lib.load()   # built before the child needs it
    keep = {k: v for k, v in os.environ.items() if not k.startswith("DCOL_")}
    cmd = [sys.executable, os.path.join(VC.HERE, "variant_child.py"), json.dumps(env), path]
    try:
        r = subprocess.run(cmd, env={**keep, **env}, capture_output=True, text=True, timeout=600)
    except subprocess.TimeoutExpired:   # a hang: nothing more on this device
        pytest.exit(f"variant_child.py {json.dumps(env)} did not end within 600 s", returncode=3)
    # killed, or a device fault reported through Python: nothing more on this device either
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139) or any(w in r.stderr for w in FAULT_WORDS):
        pytest.exit(f"variant_child.py {json.dumps(env)} ended with {r.returncode}:\n{r.stderr[-3000:]}", returncode=3)
    assert r.returncode == 0, (r.returncode, r.stderr[-3000:])
    with np.load(path, allow_pickle=False) as z:
        return json.loads(str(z["meta"])), {k: z[k] for k in z.files if k != "meta"}


def check_jacobian(c, jac):
    """J [48, B] of a Jacobian case against the restatement on every pair"""
    from oracle import dcol_oracle as O
    from contact_jacobian_ref import contact_jacobian, tolerance
    tab = VC.table()
    s1, s2, p1, p2 = VC.pairs_of(c)
    c4 = bool(c["options"] & VC.CASE4)
    B = len(s1)
    J_dev = jac.reshape(4, 12, B).transpose(2, 0, 1)
    excused, worst = 0, 0.0
    for i in range(B):
        a, b = O.shape_from_table(tab, int(s1[i])), O.shape_from_table(tab, int(s2[i]))
        _, _, x, s, z, _, dims = O.proximity(a, p1[i, :3], p1[i, 3:], b, p2[i, :3], p2[i, 3:], 1e-6, c4)
        th = np.concatenate([p1[i], p2[i]])
        J, cond = contact_jacobian(O, a, b, x, s, z, th, dims, c4)
        tol = tolerance(O, a, b, x, s, z, th, dims, J, c4)
        err = np.abs(J_dev[i] - J).max()
        worst = max(worst, err / tol)
        if not err <= tol:
            assert cond > COND_MAX, (c["id"], i, err, tol, cond)
            excused += 1
    assert excused <= 0.1 * B, (c["id"], excused)
    return worst


@pytest.mark.gpu
@pytest.mark.parametrize("g", range(len(GROUPS)), ids=[VC.group_id(e) for e, _ in GROUPS])
def test_variant_group_matches_oracle(g, tmp_path):
    if not gpu_available():
        pytest.skip("no GPU")
    env, todo = GROUPS[g]
    meta, out = run_child(env, str(tmp_path / "out.npz"))
    stats = {}
    for c in todo:
        m = meta["cases"][str(c["id"])]
        e = m["emul"]
        # layout: the device's plan is the x86 policy's, so the CPU ledger holds here
        assert m["buckets"] == e["buckets"], (c["id"], m["buckets"], e["buckets"])
        assert m["launch_form"] == e["launch_form"] and m["num_launches"] == e["launches"], (c["id"], m, e)
        assert not e["unlaunchable"] and e["form"] == ("fused" if c["form"] == "server" else c["form"]), (c["id"], e)
        st = stats.setdefault(c["form"], {"copies": set(), "alpha": 0.0, "grad": 0.0, "env": 0.0, "jac": 0.0})
        st["copies"] |= {tuple(x) for x in e["copies"]}
        ref = VC.reference(c)
        ok = ref["status"] == 0
        assert ok.all(), c["id"]
        case4 = bool(c["options"] & VC.CASE4)
        for grad in ("fd",) if c["form"] == "server" else ("fd", "envelope"):
            al, gr = out[f"{c['id']}_{grad}_alpha"], out[f"{c['id']}_{grad}_grad"].T
            it, status = out[f"{c['id']}_{grad}_iters"], out[f"{c['id']}_{grad}_status"]
            np.testing.assert_array_equal(status, ref["status"], err_msg=f"case {c['id']} {grad}")
            ea = (np.abs(al - ref["alpha"]) / np.maximum(np.abs(ref["alpha"]), 1e-12)).max()
            eg = (np.abs(gr - ref["grad"]).max(1) / np.maximum(np.abs(ref["grad"]).max(1), 1.0)).max()
            if case4:   # as tests/test_case4.py
                assert (it == ref["iters"]).mean() >= 0.99, (c["id"], grad)
                assert alpha_close(al, ref["alpha"]).all(), (c["id"], grad, ea)
                assert grad_close(gr, ref["grad"]).all(), (c["id"], grad, eg)
                continue
            off = np.flatnonzero(it != ref["iters"])
            assert off.size == 0, (c["id"], grad, [(int(i), int(it[i]), int(ref["iters"][i]), float(al[i]),
                                                    float(ref["alpha"][i])) for i in off[:5]])
            st["alpha"] = max(st["alpha"], ea)
            assert ea <= ALPHA_RTOL, (c["id"], grad, ea)
            if grad == "fd":
                st["grad"] = max(st["grad"], eg)
                assert eg <= GRAD_TOL, (c["id"], eg)
            else:
                st["env"] = max(st["env"], eg)
                assert grad_close(gr, ref["grad"]).all(), (c["id"], eg)
        if c["form"] == "jac":
            st["jac"] = max(st["jac"], check_jacobian(c, out[f"{c['id']}_fd_jac"]))
        if c["form"] == "server":
            for i in range(2):
                sv = out[f"{c['id']}_server{i}"]
                plan = np.concatenate([[out[f"{c['id']}_fd_alpha"][i]], out[f"{c['id']}_fd_contact"][:, i],
                                       out[f"{c['id']}_fd_grad"][:, i],
                                       [out[f"{c['id']}_fd_iters"][i], out[f"{c['id']}_fd_status"][i]]])
                assert sv.tobytes() == plan.tobytes(), (c["id"], i, sv, plan)
    if meta["server_calls"]:
        assert meta["pair_stats"]["served"] == meta["server_calls"] and meta["pair_stats"]["launched"] == 0, meta["pair_stats"]
    for form, st in stats.items():
        print(f"{VC.group_id(env)} {form}: {len(st['copies'])} copies of {len(VL.compiled(form))}; worst alpha "
              f"{st['alpha']:.2e} (bound {ALPHA_RTOL:.0e}), FD gradient {st['grad']:.2e} (bound {GRAD_TOL:.0e}), envelope "
              f"gradient {st['env']:.2e}" + (f", J error / tolerance {st['jac']:.2f}" if form == "jac" else ""))
