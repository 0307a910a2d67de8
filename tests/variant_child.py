"""Child process of tests/test_variant_parity_gpu.py: `python variant_child.py ENV_JSON OUT.npz`
runs every case of one environment group (tests/variant_cases.py) on the device with one Engine
and writes what it saw (test infrastructure).  The environment is the parent's to set: DCOL_LPP,
DCOL_NO_PART, DCOL_SPLIT and DCOL_WPS are read once per process.

Per case: Plan.buckets(), launch_form and num_launches, the x86 policy's layout for the device's
SIMD count (4 per compute unit), and the outputs for grad="fd" and grad="envelope" (a Jacobian
case with jacobian=True).  A server case: its two pairs through dcol_prox_pair (FD gradient and
contact point: one set of flags, so the resident server answers every call) after all plans have
run, next to the fused plan of the two."""
import ctypes
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)

import variant_cases as VC  # noqa: E402


def main(env, out_path):
    assert all(os.environ.get(k) == v for k, v in env.items()), env
    import torch
    from dcol_amd import Engine, _lib, spec_from_arrays
    tab = VC.table()
    eng = Engine(device=0)
    ids = np.array([eng.register(spec_from_arrays(tab, k)) for k in range(len(tab["type"]))], np.int32)
    dev = torch.device("cuda", 0)
    simds = 4 * torch.cuda.get_device_properties(0).multi_processor_count
    todo = [c for c in VC.cases() if VC.env_key(c["env"]) == VC.env_key(env)]
    meta, arrays = {"simds": simds, "cases": {}}, {}
    for c in todo:
        s1, s2, p1, p2 = VC.pairs_of(c)
        jac = bool(c["options"] & VC.JACOBIAN)
        plan = eng.plan(ids[s1], ids[s2], cache=False, case4=bool(c["options"] & VC.CASE4), jacobian=jac)
        m = {"buckets": plan.buckets(), "launch_form": plan.launch_form, "num_launches": plan.num_launches,
             "emul": VC.evaluate(c, env, simds)}
        meta["cases"][str(c["id"])] = m
        d1 = torch.from_numpy(np.ascontiguousarray(p1.T)).to(dev)
        d2 = torch.from_numpy(np.ascontiguousarray(p2.T)).to(dev)
        for grad in ("fd",) if c["form"] == "server" else ("fd", "envelope"):
            o = plan.run(d1, d2, grad=grad, contact=True, jacobian=jac)
            torch.cuda.synchronize(dev)
            for k in ("alpha", "grad", "iters", "status", "contact") + (("jac",) if jac else ()):
                arrays[f"{c['id']}_{grad}_{k}"] = o[k].cpu().numpy()
        del plan
    lib = _lib.load()
    table = eng.table
    ptr = lambda x: ctypes.c_void_p(x.ctypes.data)  # noqa: E731
    calls = 0
    for c in todo:
        if c["form"] != "server":
            continue
        s1, s2, p1, p2 = VC.pairs_of(c)
        for i in range(len(s1)):
            a, ct, g = np.empty(1), np.empty(3), np.empty(12)
            it, st = ctypes.c_int32(), ctypes.c_int32()
            q1, q2 = np.ascontiguousarray(p1[i]), np.ascontiguousarray(p2[i])
            _lib.check(lib.dcol_prox_pair(table.handle, int(ids[s1[i]]), int(ids[s2[i]]), ptr(q1), ptr(q2), 1e-6, 50,
                                          _lib.GRAD_FD | _lib.CONTACT, ptr(a), ptr(ct), ptr(g), ctypes.byref(it),
                                          ctypes.byref(st)), "dcol_prox_pair")
            calls += 1
            arrays[f"{c['id']}_server{i}"] = np.concatenate([a, ct, g, [it.value, st.value]])
    meta["server_calls"] = calls
    meta["pair_stats"] = eng.pair_stats() if calls else {}
    np.savez(out_path, meta=np.array(json.dumps(meta)), **arrays)


if __name__ == "__main__":
    main(json.loads(sys.argv[1]), sys.argv[2])
