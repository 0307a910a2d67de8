"""proximity_jacobian — the contact-point Jacobian of two primitives at their current poses
(no counterpart in the reference's proximity package; the upstream method's
DifferentiableCollisions.jl proximity_jacobian returns the same derivative).

alpha, the contact point x[0:3] and J = d[x0, x1, x2, alpha] / d[r1, p1, r2, p2] (4 x 12,
columns ordered as proximity_gradient's): the KKT conditions of the conic program
differentiated at the iterate the PDIP returns, solved on the GPU next to the solve
(include/dcol.h dcol_plan_run_jac).  One host call with a batch of one per call: per-call
latency is not what this entry point is for -- batches go through
Engine.solve_host(jacobian=True) or Plan.run(jacobian=True).
"""
import numpy as np

from dcol_amd.engine import DEFAULT_TOL, default_engine, raise_for_status
from dcol_amd.shapes import pose_of


def proximity_jacobian(prim1, prim2, pdip_tol=DEFAULT_TOL, verbose=False, stream=False):
    """-> (alpha: float64, contact_point: ndarray(3), J: ndarray(4, 12)).  Raises like
    proximity_mrp / proximity_gradient.  J is NaN where the linearised KKT system at the
    iterate is singular (the pair's status stays OK: alpha and the contact point are valid).
    stream=True: a pair of 129 to 1,024 orthant rows (a many-faced polytope) gets its Jacobian
    from the streamed-row kernels (Engine.solve_host(jacobian="stream")) instead of the
    ValueError the default raises for it."""
    eng = default_engine()
    with eng._lock:
        s1 = eng.register_object(prim1)
        s2 = eng.register_object(prim2)
    p1 = np.reshape(pose_of(prim1), (1, 6))
    p2 = np.reshape(pose_of(prim2), (1, 6))
    res = eng.solve_host([s1], [s2], p1, p2, tol=pdip_tol, max_iter=eng.max_iter, grad=None, contact=True,
                         jacobian="stream" if stream else True)
    raise_for_status(int(res.status[0]))
    return res.alpha[0], res.contact[0].copy(), res.jac[0].copy()
