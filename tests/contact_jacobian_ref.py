"""NumPy restatement of the contact-point Jacobian d[x0..2, alpha]/d[r1, p1, r2, p2] on the
oracle's own pieces (test infrastructure of tests/test_contact_jacobian.py; DESIGN.md
"gradient modes").

At the returned iterate (x, s, z) the KKT conditions G'z + c = 0, G x + s = h, s o z = const
are differentiated in a pose coordinate with the residuals held fixed:
    G'dz = -dG'z,   G dx + ds = dh - dG x,   L(z) ds + L(s) dz = 0,
L(v) = diag(v) on orthant rows and the arrow matrix on each SOC block.  With
D = L(s)^-1 L(z):  H dx = -dG'z - G'D (dG x - dh),  H = G'D G  (non-symmetric), and in
adjoint form, v_k = H^-T e_k, a_k = -D'G v_k:
    J[k][j] = a_k.(dG_j x - dh_j) - z.(dG_j v_k),   k = 0..3 (x, y, z of the contact, alpha).
dG_j, dh_j by central differences of the assembled problem (step 1e-6), as the oracle's
implicit_gradient takes them.
"""
import numpy as np


def arrow(v):
    """L(v) of one SOC block: [[v0, vbar'], [vbar, v0 I]]."""
    L = v[0] * np.eye(v.size)
    L[0, 1:] = v[1:]
    L[1:, 0] = v[1:]
    return L


def cone_matrix(v, dims):
    """L(v) over [orthant | soc1 | soc2] (block diagonal)."""
    no, n1, n2 = dims
    L = np.diag(np.asarray(v, float).copy())
    for lo, n in ((no, n1), (no + n1, n2)):
        if n > 0:
            L[lo:lo + n, lo:lo + n] = arrow(v[lo:lo + n])
    return L


def contact_jacobian(O, a, b, x, s, z, theta, dims, case4=False, step=1e-6, nt=False):
    """-> (J (4, 12), cond(H)).  nt=True: the NT-scaled form D = W^-2 of the engine's
    DCOL_GRAD_IMPLICIT mode extended to the contact rows (recorded, never asserted)."""
    th = np.asarray(theta, float)
    _, G, h, _, _, _ = O._assemble(a, th[0:3], th[3:6], b, th[6:9], th[9:12], case4)
    if nt:
        W = O._NT(s, z, O._Cones(*dims))
        Wi = W.solve_mat(np.eye(s.size))
        D = Wi.T @ Wi
    else:
        D = np.linalg.solve(cone_matrix(s, dims), cone_matrix(z, dims))
    H = G.T @ D @ G
    V = np.linalg.solve(H.T, np.eye(G.shape[1])[:, :4])     # columns v_k = H^-T e_k
    Aw = -D.T @ (G @ V)                                       # columns a_k
    J = np.empty((4, 12))
    for j in range(12):
        tp, tm = th.copy(), th.copy()
        tp[j] += step
        tm[j] -= step
        _, Gp, hp, _, _, _ = O._assemble(a, tp[0:3], tp[3:6], b, tp[6:9], tp[9:12], case4)
        _, Gm, hm, _, _, _ = O._assemble(a, tm[0:3], tm[3:6], b, tm[6:9], tm[9:12], case4)
        dG, dh = (Gp - Gm) / (2 * step), (hp - hm) / (2 * step)
        J[:, j] = Aw.T @ (dG @ x - dh) - (dG @ V).T @ z
    return J, np.linalg.cond(H)


def sensitivity(O, a, b, x, s, z, theta, dims, J, case4=False, seed=0):
    """Largest change of J over three seeded re-evaluations with x, s, z each perturbed by
    1e-13 relative: how far two evaluations of the same formula at iterates that agree to
    rounding may differ (the per-pair tolerance of the kernel comparisons comes from it)."""
    rng = np.random.default_rng(seed)
    worst = 0.0
    for _ in range(3):
        xp, sp, zp = (v * (1.0 + 1e-13 * rng.standard_normal(v.size)) for v in (x, s, z))
        Jp, _ = contact_jacobian(O, a, b, xp, sp, zp, theta, dims, case4)
        worst = max(worst, float(np.abs(Jp - J).max()))
    return worst


def tolerance(O, a, b, x, s, z, theta, dims, J, case4=False):
    """max(1e-7, 100 sens) sc, never above 1e-3 sc; sc = max(|J|_inf, 1)."""
    sc = max(float(np.abs(J).max()), 1.0)
    sens = sensitivity(O, a, b, x, s, z, theta, dims, J, case4) / sc
    return min(max(1e-7, 100.0 * sens), 1e-3) * sc
