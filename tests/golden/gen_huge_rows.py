#!/usr/bin/env python3
"""Generate tests/golden/huge/huge_rows.npz by running the REFERENCE implementation on pairs
of 129 to 1,025 orthant rows (the streamed-row kernel's range, and one row past its cap).

Runs only where the reference is mounted (see gen_golden.py, whose helpers drive it).  Data
only: the shape table, the pairs and poses, and the reference's alpha, contact point, FD
gradient, iteration count and status.  The fixture sits in a directory of its own because the
parity tests written for the <= 128-row fixtures collect every tests/golden/*.npz -- among
them the C oracle's, whose restatement is capped at 136 rows.

The generator asserts, and writes nothing if one fails:
  * every supported pair converges in the reference;
  * the NumPy oracle's iteration count for it is unchanged under two draws of 1e-13 relative
    pose perturbation (a pair that flips is replaced by another draw of poses);
  * at most 5 % of the draws were replaced (the number is stored as `replaced`).

`expect_status` is what the engine reports: the reference's status, except DCOL_TOO_LARGE (5)
for the pairs of more than 1,024 rows, which the reference solves.

Usage:  python tests/golden/gen_huge_rows.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

import gen_golden as G  # noqa: E402  (puts the reference on sys.path)
from gen_golden import mpc  # noqa: E402
from oracle import dcol_oracle as O  # noqa: E402

MAX_ROWS = 1024
ST_TOO_LARGE = 5
DRAWS = 3          # pose draws per ordered pair
TOL = 1e-6


def offset_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, v = q[0], q[1:]
    vx = np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]])
    return np.eye(3) + 2 * w * vx + 2 * vx @ vx


def build_table(rng):
    tab = G.Table()
    k = {}
    for name, faces in (("p123", 123), ("p127", 127), ("p186", 186), ("p187", 187), ("p250", 250), ("p251", 251),
                        ("p506a", 506), ("p506b", 506), ("p512a", 512), ("p512b", 512), ("p513", 513)):
        obj = G.rand_polytope(rng, faces)
        if name == "p250":       # a non-identity r_offset / Q_offset
            obj.r_offset = rng.uniform(-0.5, 0.5, 3)
            obj.Q_offset = offset_rotation(rng)
        k[name] = tab.add(obj)
    for name, edges in (("g125", 125), ("g300", 300)):
        poly = mpc.create_n_sided(edges, 0.6)
        k[name] = tab.add(mpc.PolygonMRP(poly["A"], poly["b"], 0.2))
    k["sph"] = tab.add(mpc.SphereMRP(0.5))
    k["cone"] = tab.add(mpc.ConeMRP(1.2, np.deg2rad(25.0)))
    k["cap"] = tab.add(mpc.CapsuleMRP(0.3, 1.0))
    k["cyl"] = tab.add(mpc.CylinderMRP(0.3, 1.0))
    k["box"] = tab.add(mpc.create_rect_prism(1.0, 0.6, 1.4))
    return tab, k


# unordered combinations; every one runs in both orders.  Orthant-row totals: 129 (a last
# slot of one row), 192 / 193 and 256 / 257 (full slots, one row over), 1,012, 1,024 (the cap),
# 1,025 (past it); every streamed (N, NSOC): polytope x polytope (4, 0), polytope x sphere /
# cone (4, 1), capsule / cylinder x polytope (5, 1), polygon x polytope (6, 1), polygon x
# sphere / cone (6, 2)
COMBOS = [("p123", "box"), ("p127", "cap"), ("p186", "box"), ("p187", "box"), ("p250", "box"), ("p251", "box"),
          ("p506a", "p506b"), ("p512a", "p512b"), ("p123", "p127"), ("p186", "p187"), ("p251", "p513"),
          ("p186", "sph"), ("p250", "cone"), ("p512a", "sph"), ("p513", "cone"),
          ("cyl", "p187"), ("cyl", "p506a"), ("cap", "p512b"),
          ("g125", "p123"), ("g300", "p250"), ("g300", "box"), ("g125", "box"), ("g300", "sph"), ("g300", "cone")]
TOO_LARGE = [("p512a", "p513")]
CASE4 = [("g300", "cap"), ("cyl", "g125"), ("cap", "cyl")]


def oracle_iters(tab_arrays, k1, k2, q1, q2):
    out = O.run_batch(tab_arrays, np.array([k1]), np.array([k2]), np.array([q1]), np.array([q2]), TOL, False)
    return int(out["status"][0]), int(out["iters"][0])


def stable(tab_arrays, k1, k2, q1, q2, rng):
    st, it = oracle_iters(tab_arrays, k1, k2, q1, q2)
    if st != 0:
        return False
    for _ in range(2):
        e1 = 1.0 + 1e-13 * rng.uniform(-1, 1, 6)
        e2 = 1.0 + 1e-13 * rng.uniform(-1, 1, 6)
        if oracle_iters(tab_arrays, k1, k2, np.array(q1) * e1, np.array(q2) * e2) != (0, it):
            return False
    return True


def main():
    rng = np.random.default_rng(20261019)
    tab, k = build_table(rng)
    arrays = tab.arrays()
    rows = {i: (int(arrays["nh"][i]) if arrays["type"][i] in (G.POLYTOPE, G.POLYGON)
                else {G.SPHERE: 0, G.CONE: 1, G.CAPSULE: 2, G.CYLINDER: 4}[int(arrays["type"][i])])
            for i in range(len(tab.objs))}
    pairs, expect, draws, replaced = [], [], 0, 0
    for a, b in COMBOS + TOO_LARGE:
        for k1, k2 in ((k[a], k[b]), (k[b], k[a])):
            for _ in range(DRAWS if (a, b) in COMBOS else 1):
                while True:
                    draws += 1
                    q1, q2 = G.rand_pose(rng), G.rand_pose(rng)
                    if stable(arrays, k1, k2, q1, q2, rng):
                        break
                    replaced += 1
                pairs.append((k1, k2, q1, q2))
                expect.append(ST_TOO_LARGE if rows[k1] + rows[k2] > MAX_ROWS else 0)
    for a, b in CASE4:
        for k1, k2 in ((k[a], k[b]), (k[b], k[a])):
            pairs.append((k1, k2, G.rand_pose(rng), G.rand_pose(rng)))
            expect.append(G.ST_UNSUPPORTED)
    assert replaced <= 0.05 * draws, f"{replaced} of {draws} draws replaced"

    B = len(pairs)
    out = dict(alpha=np.full(B, np.nan), contact=np.full((B, 3), np.nan), grad=np.full((B, 12), np.nan),
               iters=np.full(B, -1, np.int32), status=np.zeros(B, np.int32))
    for i, (k1, k2, q1, q2) in enumerate(pairs):
        o1, o2 = tab.objs[k1], tab.objs[k2]
        o1.r, o1.p = np.array(q1[:3], float), np.array(q1[3:], float)
        o2.r, o2.p = np.array(q2[:3], float), np.array(q2[3:], float)
        try:
            x, s, z, it = G.ref_solve(o1, o2, TOL)
        except G.Unsupported:
            out["status"][i] = G.ST_UNSUPPORTED
            continue
        a_mrp, cp = G.proximity_mrp(o1, o2, pdip_tol=TOL)
        a_g, g = G.proximity_gradient(o1, o2, pdip_tol=TOL)
        assert a_mrp == x[3] and a_g == x[3] and np.array_equal(cp, x[:3])
        out["alpha"][i], out["contact"][i], out["grad"][i], out["iters"][i] = x[3], x[:3], g, it
    expect = np.array(expect, np.int32)
    supported = expect != G.ST_UNSUPPORTED
    assert np.all(out["status"][supported] == 0), "a supported pair did not converge in the reference"
    assert np.all(out["status"][~supported] == G.ST_UNSUPPORTED)

    arrays.update(s1=np.array([p[0] for p in pairs], np.int32), s2=np.array([p[1] for p in pairs], np.int32),
                  pose1=np.array([p[2] for p in pairs], float).reshape(-1, 6),
                  pose2=np.array([p[3] for p in pairs], float).reshape(-1, 6), tol=np.float64(TOL),
                  expect_status=expect, rows=np.array([rows[p[0]] + rows[p[1]] for p in pairs], np.int32),
                  replaced=np.int32(replaced), draws=np.int32(draws))
    arrays.update(out)
    os.makedirs(os.path.join(HERE, "huge"), exist_ok=True)
    path = os.path.join(HERE, "huge", "huge_rows.npz")
    np.savez_compressed(path, **arrays)
    print(f"{B} pairs, {replaced} of {draws} draws replaced, iters {out['iters'][expect == 0].min()}.."
          f"{out['iters'][expect == 0].max()} -> {path} ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
