"""The shape table of the case-4 tests (tests/test_case4.py, the case-4 pair of
tests/test_contact_jacobian.py): capsules, cylinders and polygons (test infrastructure)."""
import numpy as np

from geometry_bruteforce import CAPSULE, CYLINDER, POLYGON, _dcm

KINDS = (CAPSULE, CYLINDER, POLYGON)


def ngon(n, d):
    t = np.linspace(0, 2 * np.pi, n, endpoint=False)
    return np.stack([np.cos(t), np.sin(t)], 1), np.full(n, d)


def case4_table(rng, n_shapes=9):
    """Shape table (tests/golden layout) of capsules, cylinders and polygons, some with
    non-trivial body offsets."""
    tab = {k: [] for k in ("type", "nh", "A_off", "params", "r_offset", "Q_offset")}
    A_rows, b_rows = [], []
    for k in range(n_shapes):
        t = KINDS[k % 3]
        R, L = rng.uniform(0.15, 0.6), rng.uniform(0.4, 2.0)
        tab["type"].append(t)
        tab["A_off"].append(len(b_rows))
        if t == POLYGON:
            A, b = ngon(int(rng.integers(3, 8)), rng.uniform(0.3, 1.0))
            tab["nh"].append(len(b))
            A_rows += [list(a) + [0.0] for a in A]
            b_rows += list(b)
            tab["params"].append((R * 0.5, 0, 0, 0))
        else:
            tab["nh"].append(0)
            tab["params"].append((R, L, 0, 0))
        off = k % 4 == 3
        tab["r_offset"].append(rng.uniform(-0.3, 0.3, 3) if off else np.zeros(3))
        tab["Q_offset"].append(_dcm(rng.uniform(-0.5, 0.5, 3)) if off else np.eye(3))
    out = {k: np.array(v) for k, v in tab.items()}
    out["type"] = out["type"].astype(np.int32)
    out["nh"] = out["nh"].astype(np.int32)
    out["A_off"] = out["A_off"].astype(np.int32)
    out["A_pool"] = np.array(A_rows, dtype=np.float64).reshape(-1, 3)
    out["b_pool"] = np.array(b_rows, dtype=np.float64)
    return out
