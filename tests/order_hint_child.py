"""Child process of tests/test_order_hint.py: the order-hint scenarios on the GPU, every
output of every run saved to one .npz.  The test runs it twice -- with the hint (the
default) and under DCOL_NO_ORDER_HINT=1, which the library reads once per process -- and
compares the two files bitwise.

Usage: python order_hint_child.py OUT.npz
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (os.path.join(REPO, "dcol-trajectory-optimization_amd"), REPO):
    if p not in sys.path:
        sys.path.insert(0, p)

SENT_F = -12345.678   # prefill of the float outputs (no solve returns it)
SENT_I = -77          # prefill of iters / status
POLY_B = (1, 31, 256, 257, 1000)   # one pair; a partly filled wave; whole windows; whole windows
                                   # and one pair; 1000: a ragged last window ending in an 8-pair wave
MIXED_TILE = 2        # synthetic_mixed.npz (1500 pairs) tiled: several variants and lane counts
RUNS = 4


def golden(name):
    return dict(np.load(os.path.join(HERE, "golden", name), allow_pickle=False))


def poses(d, B, r):
    """Poses of run r of a B-pair case: the golden poses in runs 0 and 3 (so the first and the
    last run compare with the golden status and iterations), perturbed ones in between (the
    iteration counts, and with them the order, change from run to run)."""
    K = -(-B // len(d["s1"]))
    p1, p2 = np.tile(d["pose1"], (K, 1))[:B].copy(), np.tile(d["pose2"], (K, 1))[:B].copy()
    if r in (1, 2):
        rng = np.random.default_rng(100 * r + B % 97)
        p1 += 0.05 * rng.standard_normal(p1.shape)
        p2 += 0.05 * rng.standard_normal(p2.shape)
    return p1, p2


def main(out_path):
    import torch
    from dcol_amd import Engine, spec_from_arrays
    from dcol_amd.engine import alloc_outputs

    eng = Engine(device=0)
    dev = torch.device("cuda", 0)
    res = {}

    def register(d):
        ids = np.array([eng.register(spec_from_arrays(d, k)) for k in range(len(d["type"]))], np.int32)
        return ids[d["s1"]], ids[d["s2"]]

    def soa(p):
        return torch.from_numpy(np.ascontiguousarray(p.T)).to(dev)

    def fresh(B):
        o = alloc_outputs(B, dev, True, True)
        for k, t in o.items():
            t.fill_(SENT_I if t.dtype == torch.int32 else SENT_F)
        return o

    def keep(tag, o):
        for k, t in o.items():
            res[f"{tag}.{k}"] = t.cpu().numpy()

    dp, dm = golden("synthetic_polypoly.npz"), golden("synthetic_mixed.npz")
    sp = register(dp)
    sm = register(dm)
    cases = [(f"poly{B}", dp, sp[0][:B], sp[1][:B], B) for B in POLY_B]
    Bm = MIXED_TILE * len(dm["s1"])
    cases.append(("mixed", dm, np.tile(sm[0], MIXED_TILE), np.tile(sm[1], MIXED_TILE), Bm))
    forms, lanes = [], set()
    for tag, d, s1, s2, B in cases:
        plan = eng.plan(s1, s2, cache=False, fuse=False)
        forms.append(plan.launch_form)
        lanes |= {b["lpp"] for b in plan.buckets() if b["kind"] == "solve"}
        for r in range(RUNS):   # consecutive runs of ONE plan on ONE stream: run r + 1 uses run r's counts
            p1, p2 = poses(d, B, r)
            o = fresh(B)
            plan.run(soa(p1), soa(p2), grad="fd", contact=True, out=o)
            torch.cuda.synchronize()
            keep(f"{tag}.run{r}", o)
    res["forms"] = np.array(forms)
    res["lanes"] = np.array(sorted(lanes), np.int32)

    # max_iter = 3: every hint byte is 3, outputs NaN; then an uncapped run on that hint
    B = 1000
    plan = eng.plan(sp[0][:B], sp[1][:B], cache=False, fuse=False)
    p1, p2 = (soa(p) for p in poses(dp, B, 0))
    plan.run(p1, p2, grad="fd", contact=True, out=fresh(B))   # (counts to forget)
    for tag, cap in (("cap3", 3), ("aftercap", 50)):
        o = fresh(B)
        plan.run(p1, p2, max_iter=cap, grad="fd", contact=True, out=o)
        torch.cuda.synchronize()
        keep(tag, o)

    # two streams: the same plan concurrently on two streams at different poses, three rounds
    plan = eng.plan(sp[0][:B], sp[1][:B], cache=False, fuse=False)
    st = [torch.cuda.Stream(dev), torch.cuda.Stream(dev)]
    ps = [tuple(soa(p) for p in poses(dp, B, r)) for r in (0, 1)]
    torch.cuda.synchronize()
    for rnd in range(3):
        os_ = [fresh(B), fresh(B)]
        torch.cuda.synchronize()
        for j in (0, 1):
            plan.run(ps[j][0], ps[j][1], grad="fd", contact=True, out=os_[j], stream=st[j])
        torch.cuda.synchronize()
        for j in (0, 1):
            keep(f"two.round{rnd}.stream{j}", os_[j])
    np.savez(out_path, **res)


if __name__ == "__main__":
    main(sys.argv[1])
