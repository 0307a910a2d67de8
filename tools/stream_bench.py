#!/usr/bin/env python3
"""Step times of streamed batches (pairs above 128 orthant rows: csrc/dcol_kernels_stream.hip),
with the (4, 0, 128) register bucket at 128 rows as the yardstick, in one session.

Batches of --pairs pairs, one shape pair each: polytope x polytope at 128 (register bucket),
129, 256, 512 and 1,024 rows; polygon x polytope and polytope x cone at 256 rows.  Random
k-face polytopes as tools/large_bench.py, poses as bench.py configs[3], FD gradients.  A
step is one dcol_plan_run; step time = device events around --steps back-to-back steps,
minimum and median over --rounds rounds that alternate the batches.  Per batch one JSON
line: ms per step, pair-solves/s, mean iterations, ns per pair x row x iteration.  The first
64 pairs of each batch are checked against the NumPy oracle (status, iteration counts, alpha
1e-6 relative).
--jacobian: instead, the cost of the contact-point Jacobian on streamed pairs
(csrc/dcol_kernels_stream_jac.hip): batches at 129, 256 and 1,024 rows for (4, 0) and at 256
rows for (6, 1), each in ONE plan made with jacobian="stream"; per round the FD-only run (the
plain streamed kernels) and the run with the Jacobian (their JAC copies, FD gradient too)
alternate.  Per batch one JSON line: ms per step of both and their ratio (of the minima).
--case4: instead, the case-4 streamed kernels (csrc/dcol_kernels_stream_c4.hip; plans made with
case4="stream"): polygon x polygon (8, 2) and cylinder x polygon (7, 2) batches at 40, 129, 512
and 1,024 rows, and beside each the existing streamed (6, 2) instance (polygon x sphere) at the
same row count -- the nearest kernel of cases 1-3 -- in the same session.
Usage: python3 tools/stream_bench.py [--pairs 4096] [--steps 30] [--rounds 4] [--jacobian | --case4]
"""
import argparse
import json
import os
import sys

import numpy as np

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "dcol-trajectory-optimization_amd"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=4096)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--check", type=int, default=64)
    ap.add_argument("--jacobian", action="store_true")
    ap.add_argument("--case4", action="store_true")
    args = ap.parse_args()
    import torch
    from dcol_amd import Engine, ShapeSpec, alloc_outputs
    from oracle import dcol_oracle as O
    rng = np.random.default_rng(5)

    # a shape: (the engine's spec, the oracle's spec, orthant rows)
    def poly(k):
        A = np.vstack([np.eye(3), -np.eye(3), rng.normal(size=(k - 6, 3))])
        A /= np.linalg.norm(A, axis=1, keepdims=True)
        b = rng.uniform(0.4, 1.3, k)
        return ShapeSpec(0, A=tuple(A.reshape(-1)), b=tuple(b)), O.ShapeSpec(O.POLYTOPE, A=A, b=b), k

    def gon(k):
        t = np.linspace(0, 2 * np.pi, k, endpoint=False)
        A, b = np.stack([np.cos(t), np.sin(t)], 1), np.full(k, 0.6)
        return ShapeSpec(5, A=tuple(A.reshape(-1)), b=tuple(b), R=0.2), O.ShapeSpec(O.POLYGON, A=A, b=b, R=0.2), k

    cone = (ShapeSpec(2, H=1.2, beta=0.4), O.ShapeSpec(O.CONE, H=1.2, beta=0.4), 1)
    sph = (ShapeSpec(1, R=0.5), O.ShapeSpec(O.SPHERE, R=0.5), 0)
    cyl = (ShapeSpec(4, R=0.3, L=1.0), O.ShapeSpec(O.CYLINDER, R=0.3, L=1.0), 4)

    cases = [("poly x poly 128 (register bucket)", poly(64), poly(64)), ("poly x poly 129", poly(65), poly(64)),
             ("poly x poly 256", poly(128), poly(128)), ("poly x poly 512", poly(256), poly(256)),
             ("poly x poly 1024", poly(512), poly(512)), ("polygon x poly 256", gon(128), poly(128)),
             ("poly x cone 256", poly(255), cone)]
    case4 = "stream" if args.case4 else False
    if args.case4:
        cases = []
        for r in (40, 129, 512, 1024):
            cases += [(f"polygon x polygon {r}", gon(r // 2), gon(r - r // 2)), (f"cylinder x polygon {r}", cyl, gon(r - 4)),
                      (f"polygon x sphere {r} (streamed (6, 2))", gon(r), sph)]
    eng = Engine(device=0)
    dev = torch.device("cuda", 0)
    B = args.pairs
    if args.jacobian:
        jacobian_bench(args, eng, dev, rng, [("poly x poly 129", poly(65), poly(64)), ("poly x poly 256", poly(128), poly(128)),
                                             ("poly x poly 1024", poly(512), poly(512)),
                                             ("polygon x poly 256", gon(128), poly(128))])
        return
    runs = []
    for name, a, b in cases:
        ia, ib = eng.register(a[0]), eng.register(b[0])
        p1 = np.hstack([rng.uniform(-3, 3, (B, 3)), rng.uniform(-1, 1, (B, 3))])
        p2 = np.hstack([rng.uniform(-3, 3, (B, 3)), rng.uniform(-1, 1, (B, 3))])
        runs.append(dict(name=name, a=a, b=b, ia=ia, ib=ib, p1=p1, p2=p2))
    for r in runs:   # (plans after every shape is registered: one table)
        plan = eng.plan(np.full(B, r["ia"], np.int32), np.full(B, r["ib"], np.int32), case4=case4)
        d1 = torch.from_numpy(np.ascontiguousarray(r["p1"].T)).to(dev)
        d2 = torch.from_numpy(np.ascontiguousarray(r["p2"].T)).to(dev)
        out = alloc_outputs(B, dev, want_grad=True, want_contact=False)
        step = plan.bind(d1, d2, out, grad="fd", contact=False)
        for _ in range(3):
            step()
        torch.cuda.synchronize()
        it = out["iters"].cpu().numpy()
        st = out["status"].cpu().numpy()
        al = out["alpha"].cpu().numpy()
        n = min(args.check, B)
        for i in range(n):
            ra = O.proximity(r["a"][1], r["p1"][i, :3], r["p1"][i, 3:], r["b"][1], r["p2"][i, :3], r["p2"][i, 3:],
                             case4=bool(case4))
            assert st[i] == 0 and it[i] == ra[5] and abs(al[i] - ra[0]) <= 1e-6 * abs(ra[0]), (r["name"], i)
        r.update(plan=plan, step=step, keep=(d1, d2, out), iters=float(it[st == 0].mean()), ok=int((st == 0).sum()),
                 bucket=plan.buckets()[0], ms=[])
    for _ in range(args.rounds):
        for r in runs:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(args.steps):
                r["step"]()
            e1.record()
            torch.cuda.synchronize()
            r["ms"].append(e0.elapsed_time(e1) / args.steps)
    for r in runs:
        bk = r["bucket"]
        rows = r["a"][2] + r["b"][2]
        mn, med = float(np.min(r["ms"])), float(np.median(r["ms"]))
        print(json.dumps({"batch": r["name"], "pairs": B, "rows": rows, "bucket": [bk["N"], bk["nsoc"], bk["omax"], bk["lpp"]],
                          "ok": r["ok"], "mean_iters": round(r["iters"], 2), "ms_min": round(mn, 4), "ms_median": round(med, 4),
                          "pair_solves_per_s": round(B / (mn * 1e-3)),
                          "ns_per_pair_row_iter": round(mn * 1e6 / (B * rows * r["iters"]), 4)}), flush=True)


def jacobian_bench(args, eng, dev, rng, cases):
    import torch
    from dcol_amd import alloc_outputs
    B = args.pairs
    runs = []
    for name, a, b in cases:
        ia, ib = eng.register(a[0]), eng.register(b[0])
        p1 = np.hstack([rng.uniform(-3, 3, (B, 3)), rng.uniform(-1, 1, (B, 3))])
        p2 = np.hstack([rng.uniform(-3, 3, (B, 3)), rng.uniform(-1, 1, (B, 3))])
        runs.append(dict(name=name, rows=a[2] + b[2], ia=ia, ib=ib, p1=p1, p2=p2))
    for r in runs:
        plan = eng.plan(np.full(B, r["ia"], np.int32), np.full(B, r["ib"], np.int32), jacobian="stream")
        d1 = torch.from_numpy(np.ascontiguousarray(r["p1"].T)).to(dev)
        d2 = torch.from_numpy(np.ascontiguousarray(r["p2"].T)).to(dev)
        out = alloc_outputs(B, dev, want_grad=True, want_contact=False, want_jac=True)
        steps = {m: (lambda m=m, plan=plan, d1=d1, d2=d2, out=out: plan.run(d1, d2, grad="fd", contact=False, out=out,
                                                                          jacobian=m == "jac")) for m in ("fd", "jac")}
        for m in ("fd", "jac"):
            for _ in range(3):
                steps[m]()
        torch.cuda.synchronize()
        it, st = out["iters"].cpu().numpy(), out["status"].cpu().numpy()
        fin = bool(np.isfinite(out["jac"].cpu().numpy()[:, st == 0]).all())
        r.update(plan=plan, steps=steps, iters=float(it[st == 0].mean()), ok=int((st == 0).sum()), finite=fin,
                 bucket=plan.buckets()[0], ms={"fd": [], "jac": []})
    for _ in range(args.rounds):
        for r in runs:
            for m in ("fd", "jac"):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                for _ in range(args.steps):
                    r["steps"][m]()
                e1.record()
                torch.cuda.synchronize()
                r["ms"][m].append(e0.elapsed_time(e1) / args.steps)
    for r in runs:
        bk = r["bucket"]
        fd, jac = float(np.min(r["ms"]["fd"])), float(np.min(r["ms"]["jac"]))
        print(json.dumps({"batch": r["name"], "pairs": B, "rows": r["rows"], "bucket": [bk["N"], bk["nsoc"], bk["omax"], bk["lpp"]],
                          "ok": r["ok"], "jac_finite": r["finite"], "mean_iters": round(r["iters"], 2),
                          "ms_fd_min": round(fd, 4), "ms_fd_median": round(float(np.median(r["ms"]["fd"])), 4),
                          "ms_jac_min": round(jac, 4), "ms_jac_median": round(float(np.median(r["ms"]["jac"])), 4),
                          "jac_over_fd": round(jac / fd, 3)}), flush=True)


if __name__ == "__main__":
    main()
