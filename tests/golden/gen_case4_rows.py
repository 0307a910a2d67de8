#!/usr/bin/env python3
"""Generate tests/golden/case4_huge/case4_rows.npz: case-4 pairs (polygon x capsule / cylinder /
polygon) of 32 to 1,027 orthant rows -- the range of the case-4 streamed kernels
(DCOL_PLAN_CASE4_STREAM), the last register bucket below it and the first counts past its cap.

The reference raises ValueError for case-4 pairs, so -- as for tests/golden/variants/
case4_ref.npz -- the recorded values are the NumPy oracle's own, oracle.dcol_oracle.run_batch(...,
case4=True); tests/test_case4_stream.py pins that oracle to brute-force geometry.  Data only: the
shape table, the pairs and poses, and the oracle's alpha, contact point, FD gradient, iteration
count and status.  Nothing outside the repository is read.

Shapes: a capsule, a cylinder and irregular polygons (sorted random edge angles with no gap of
2.5 rad or more, edge offsets U(0.5, 0.9), R = 0.2); every fourth shape has a body offset.  A
capsule brings 2 orthant rows, a cylinder 4, an n-gon n (csrc/dcol_host.hpp digest_shape).  PAIRS
lists the ordered pairs; both orders occur, since primitive 2's extra columns start at column
4 + 2 behind a polygon and at 4 + 1 behind a capsule or cylinder.  Six poses per pair, drawn as
tests/test_case4.py draws them, at tol = 1e-6.

The generator asserts, and writes nothing if one fails:
  * the oracle alone gives status 0 on every pair (it has no row limit);
  * no pose is kept whose exit-test quantity mu = s'z / deg at the oracle's last or second-last
    iteration lies within a relative 1e-6 of tol: such a pose is redrawn, so that rounding does
    not decide an iteration count (solve_lp_pdip's trace argument gives the mu sequence);
  * at most 5 % of the draws were redrawn (the number is stored as `replaced`).

`expect_status` is what the engine reports under DCOL_PLAN_CASE4 | DCOL_PLAN_CASE4_STREAM: 0, or
DCOL_TOO_LARGE (5) for the pairs of more than 1,024 rows.

Usage:  python tests/golden/gen_case4_rows.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from geometry_bruteforce import CAPSULE, CYLINDER, POLYGON, _dcm  # noqa: E402
from oracle import dcol_oracle as O  # noqa: E402

MAX_ROWS = 1024
ST_TOO_LARGE = 5
DRAWS = 6
TOL = 1e-6
GONS = (16, 17, 28, 29, 30, 31, 33, 62, 63, 64, 65, 200, 511, 512, 513, 1020, 1021, 1022, 1023)
# ordered pairs by row count (a number names the polygon of that many edges)
PAIRS = [(28, "cyl"), (30, "cap"), (16, 16),                                              # 32: the last register bucket
         (16, 17), (17, 16), (29, "cyl"), ("cyl", 29), (31, "cap"), ("cap", 31),          # 33: first streamed
         (30, "cyl"), (31, "cyl"), ("cyl", 31), (33, "cap"), ("cap", 33),                 # 34, 35
         (62, "cap"), (63, "cap"), (64, "cap"), (65, "cap"),                              # 64, 65 (slot edge), 66, 67
         (64, 64), (64, 65), (200, 200),                                                  # 128, 129, 400
         (1021, "cap"),                                                                   # 1,023: odd tail
         (512, 512), (511, 513), (1020, "cyl"), ("cyl", 1020), (1022, "cap"),             # 1,024: the cap
         (512, 513), (1023, "cap"), (1022, "cyl"), ("cyl", 1022), (1023, "cyl")]          # 1,025 .. 1,027: too large


def polygon(rng, n):
    while True:
        t = np.sort(rng.uniform(0, 2 * np.pi, n))
        if np.diff(np.append(t, t[0] + 2 * np.pi)).max() < 2.5:   # bounded, with margin
            return np.stack([np.cos(t), np.sin(t)], 1), rng.uniform(0.5, 0.9, n)


def build_table(rng):
    tab = {k: [] for k in ("type", "nh", "A_off", "params", "r_offset", "Q_offset")}
    A_rows, b_rows, ids = [], [], {}
    for k, name in enumerate(("cap", "cyl") + GONS):
        ids[name] = k
        tab["A_off"].append(len(b_rows))
        if isinstance(name, int):
            A, b = polygon(rng, name)
            tab["type"].append(POLYGON)
            tab["nh"].append(name)
            A_rows += [list(a) + [0.0] for a in A]
            b_rows += list(b)
            tab["params"].append((0.2, 0, 0, 0))
        else:
            tab["type"].append(CAPSULE if name == "cap" else CYLINDER)
            tab["nh"].append(0)
            tab["params"].append((0.3, 1.0, 0, 0))
        off = k % 4 == 3
        tab["r_offset"].append(rng.uniform(-0.3, 0.3, 3) if off else np.zeros(3))
        tab["Q_offset"].append(_dcm(rng.uniform(-0.5, 0.5, 3)) if off else np.eye(3))
    out = {k: np.array(v) for k, v in tab.items()}
    for k in ("type", "nh", "A_off"):
        out[k] = out[k].astype(np.int32)
    out["A_pool"] = np.array(A_rows, dtype=np.float64).reshape(-1, 3)
    out["b_pool"] = np.array(b_rows, dtype=np.float64)
    return out, ids


def near_exit(tab, k1, k2, q1, q2):
    """the oracle's mu at its last or second-last iteration within a relative 1e-6 of tol"""
    a, b = O.shape_from_table(tab, k1), O.shape_from_table(tab, k2)
    c, G, h, no, n1, n2 = O._assemble(a, q1[:3], q1[3:], b, q2[:3], q2[3:], True)
    trace = []
    O.solve_lp_pdip(c, G, h, no, n1, n2, TOL, trace)
    return any(abs(t["mu"] - TOL) <= 1e-6 * TOL for t in trace[-2:])


def main():
    rng = np.random.default_rng(20261021)
    tab, ids = build_table(rng)
    rows_of = {k: {CAPSULE: 2, CYLINDER: 4}.get(int(tab["type"][k]), int(tab["nh"][k])) for k in range(len(tab["type"]))}
    s1, s2, p1, p2, draws, replaced = [], [], [], [], 0, 0
    for a, b in PAIRS:
        for _ in range(DRAWS):
            while True:
                draws += 1
                q1 = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-1, 1, 3)])
                q2 = np.concatenate([rng.uniform(-1.5, 1.5, 3), rng.uniform(-1, 1, 3)])
                if not near_exit(tab, ids[a], ids[b], q1, q2):
                    break
                replaced += 1
            s1.append(ids[a]); s2.append(ids[b]); p1.append(q1); p2.append(q2)
    assert replaced <= 0.05 * draws, f"{replaced} of {draws} draws replaced"
    s1, s2 = np.array(s1, np.int32), np.array(s2, np.int32)
    p1, p2 = np.array(p1), np.array(p2)
    out = O.run_batch(tab, s1, s2, p1, p2, TOL, True, case4=True)
    assert np.all(out["status"] == 0), "the oracle did not converge on every pair"
    rows = np.array([rows_of[int(a)] + rows_of[int(b)] for a, b in zip(s1, s2)], np.int32)
    tab.update(s1=s1, s2=s2, pose1=p1, pose2=p2, tol=np.float64(TOL), rows=rows,
               expect_status=np.where(rows > MAX_ROWS, ST_TOO_LARGE, 0).astype(np.int32),
               replaced=np.int32(replaced), draws=np.int32(draws))
    for k in ("alpha", "contact", "grad", "iters", "status"):
        tab[k] = out[k]
    os.makedirs(os.path.join(HERE, "case4_huge"), exist_ok=True)
    path = os.path.join(HERE, "case4_huge", "case4_rows.npz")
    np.savez_compressed(path, **tab)
    ok = rows <= MAX_ROWS
    print(f"{len(s1)} pairs, {replaced} of {draws} draws redrawn, iters {out['iters'][ok].min()}..{out['iters'][ok].max()}"
          f" -> {path} ({os.path.getsize(path) / 1024:.0f} KB)")


if __name__ == "__main__":
    main()
