"""Primitive objects of a golden shape table for calls through the drop-in modules
(tests/test_dropin.py, tests/test_contact_jacobian.py; test infrastructure)."""
import numpy as np


def objects_from_golden(d):
    """One primitive object per shape of a golden shape table, built with the drop-in
    constructors (misc_primitive_constructor.py:4-88) and the table's offsets."""
    from primitives.misc_primitive_constructor import (CapsuleMRP, ConeMRP, CylinderMRP, PolygonMRP, PolytopeMRP,
                                                       SphereMRP)
    objs = []
    for k in range(len(d["type"])):
        t, nh, off = int(d["type"][k]), int(d["nh"][k]), int(d["A_off"][k])
        R, L, H, beta = (float(v) for v in d["params"][k])
        A = d["A_pool"][off:off + nh]
        b = d["b_pool"][off:off + nh]
        o = {0: lambda: PolytopeMRP(A[:, :3].copy(), b.copy()), 1: lambda: SphereMRP(R), 2: lambda: ConeMRP(H, beta),
             3: lambda: CapsuleMRP(R, L), 4: lambda: CylinderMRP(R, L),
             5: lambda: PolygonMRP(A[:, :2].copy(), b.copy(), R)}[t]()
        o.r_offset = np.array(d["r_offset"][k], dtype=np.float64)
        o.Q_offset = np.array(d["Q_offset"][k], dtype=np.float64).reshape(3, 3)
        objs.append(o)
    return objs


def pose_pair(objs, d, i):
    """Set the two primitives of golden pair i to its poses (callers overwrite .r/.p) and
    return them.  A pair may name the same shape twice: then two objects are needed."""
    a, b = objs[int(d["s1"][i])], objs[int(d["s2"][i])]
    if a is b:
        import copy
        b = copy.deepcopy(a)
    a.r, a.p = list(d["pose1"][i, :3]), d["pose1"][i, 3:].copy()     # lists too (piano_mover.py:176)
    b.r, b.p = d["pose2"][i, :3].copy(), d["pose2"][i, 3:].copy()
    return a, b
