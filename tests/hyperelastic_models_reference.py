"""numpy restatement of the St Venant-Kirchhoff, Mooney-Rivlin and Yeoh energies of NonlinearElasticitySolver (no counterpart
upstream): psi(F), the first Piola-Kirchhoff stress P(F) and the fourth-order tangent A(F) = dP/dF in plain tensor form (S, E, F^-T
and their derivatives - not the invariant-derivative contraction of fs_hyper_models.hip), then the P1 element, the global assembly
and a host Newton on the pattern of hyperelastic_reference.py.  tests/test_hyperelastic_models_host.py holds this file to itself
(complex-step derivatives, symmetry, objectivity, small-strain limit) before any kernel is held to it.

Parameter row p[4]:  st_venant_kirchhoff (mu, lambda, 0, 0);  mooney_rivlin (c10, c01, kappa, 0);  yeoh (c10, c20, c30, kappa).
2-D is true plane strain: F is embedded in 3 x 3 with F33 = 1, the invariants are the 3-D ones, psi(I) = 0."""
import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

MODELS = ("st_venant_kirchhoff", "mooney_rivlin", "yeoh")
I3 = np.eye(3)


def embed(F):
    """d x d -> 3 x 3 (plane strain: F33 = 1); keeps a complex dtype"""
    F = np.asarray(F)
    if F.shape == (3, 3):
        return F
    G = np.eye(3, dtype=F.dtype)
    G[:2, :2] = F
    return G


def row(model, **kw):
    """the parameter row p[4] of a model from its named coefficients"""
    if model in ("st_venant_kirchhoff", "neo_hookean"):
        return np.array([kw["mu"], kw["lmbda"], 0.0, 0.0])
    if model == "mooney_rivlin":
        return np.array([kw["c10"], kw["c01"], kw["kappa"], 0.0])
    if model == "yeoh":
        return np.array([kw["c10"], kw["c20"], kw["c30"], kw["kappa"]])
    raise ValueError(model)


def small_strain_moduli(model, p):
    """(mu0, lambda0) of the linearisation at F = I; lambda0 = kappa - 2 mu0 / 3 for the two rubber models"""
    if model in ("st_venant_kirchhoff", "neo_hookean"):
        return p[0], p[1]
    if model == "mooney_rivlin":
        mu0, kappa = 2.0 * (p[0] + p[1]), p[2]
    else:
        mu0, kappa = 2.0 * p[0], p[3]
    return mu0, kappa - 2.0 * mu0 / 3.0


def isotropic_tensor(mu, lmbda, d=3):
    """lambda d_iJ d_kL + mu (d_ik d_JL + d_iL d_Jk) on the leading d x d x d x d block"""
    A = lmbda * np.einsum("iJ,kL->iJkL", I3, I3) + mu * (np.einsum("ik,JL->iJkL", I3, I3) + np.einsum("iL,Jk->iJkL", I3, I3))
    return A[:d, :d, :d, :d]


def _yeoh_f(p, x):
    return (p[0] * x + p[1] * x ** 2 + p[2] * x ** 3, p[0] + 2.0 * p[1] * x + 3.0 * p[2] * x ** 2, 2.0 * p[1] + 6.0 * p[2] * x)


def psi(model, p, F):
    F = embed(F)
    C = F.T @ F
    J = np.linalg.det(F)
    if model == "st_venant_kirchhoff":
        E = 0.5 * (C - I3)
        return 0.5 * p[1] * np.trace(E) ** 2 + p[0] * np.sum(E * E)
    if model == "neo_hookean":
        lj = np.log(J)
        return 0.5 * p[0] * (np.trace(C) - 3.0) - p[0] * lj + 0.5 * p[1] * lj * lj
    I1 = np.trace(C)
    I1b = J ** (-2.0 / 3.0) * I1
    if model == "mooney_rivlin":
        I2b = J ** (-4.0 / 3.0) * 0.5 * (I1 * I1 - np.trace(C @ C))
        return p[0] * (I1b - 3.0) + p[1] * (I2b - 3.0) + 0.5 * p[2] * (J - 1.0) ** 2
    return _yeoh_f(p, I1b - 3.0)[0] + 0.5 * p[3] * (J - 1.0) ** 2


def _iso_parts(F):
    """what the two rubber models share: J, F^-T, the derivative D1 of Ibar1 and D2 of Ibar2 with respect to F"""
    J = np.linalg.det(F)
    Fit = np.linalg.inv(F).T
    C = F.T @ F
    I1 = np.trace(C)
    I2 = 0.5 * (I1 * I1 - np.trace(C @ C))
    a, b = J ** (-2.0 / 3.0), J ** (-4.0 / 3.0)
    G2 = 2.0 * (I1 * F - F @ C)
    D1 = a * (2.0 * F - (2.0 / 3.0) * I1 * Fit)
    D2 = b * (G2 - (4.0 / 3.0) * I2 * Fit)
    return J, Fit, C, I1, I2, a, b, G2, D1, D2


def first_pk(model, p, F):
    """P = d psi / dF, 3 x 3 or (plane strain) its in-plane 2 x 2 block"""
    d = np.asarray(F).shape[0]
    F = embed(F)
    if model == "st_venant_kirchhoff":
        E = 0.5 * (F.T @ F - I3)
        P = F @ (p[1] * np.trace(E) * I3 + 2.0 * p[0] * E)
    elif model == "neo_hookean":
        Fit = np.linalg.inv(F).T
        P = p[0] * (F - Fit) + p[1] * np.log(np.linalg.det(F)) * Fit
    else:
        J, Fit, C, I1, I2, a, b, G2, D1, D2 = _iso_parts(F)
        if model == "mooney_rivlin":
            P = p[0] * D1 + p[1] * D2 + p[2] * (J - 1.0) * J * Fit
        else:
            P = _yeoh_f(p, a * I1 - 3.0)[1] * D1 + p[3] * (J - 1.0) * J * Fit
    return P[:d, :d]


def tangent(model, p, F):
    """A[i, J, k, L] = dP_iJ / dF_kL"""
    d = np.asarray(F).shape[0]
    F = embed(np.asarray(F, dtype=np.float64))
    B = F @ F.T
    dd = np.einsum("ik,JL->iJkL", I3, I3)
    if model == "st_venant_kirchhoff":
        E = 0.5 * (F.T @ F - I3)
        S = p[1] * np.trace(E) * I3 + 2.0 * p[0] * E
        A = (np.einsum("ik,LJ->iJkL", I3, S) + p[1] * np.einsum("iJ,kL->iJkL", F, F)
             + p[0] * (np.einsum("iL,kJ->iJkL", F, F) + np.einsum("ik,JL->iJkL", B, I3)))
        return A[:d, :d, :d, :d]
    J, Fit, C, I1, I2, a, b, G2, D1, D2 = _iso_parts(F)
    dFit = -np.einsum("kJ,iL->iJkL", Fit, Fit)                      # d (F^-T)_iJ / dF_kL
    H1 = (-(2.0 / 3.0) * np.einsum("kL,iJ->iJkL", Fit, D1)
          + a * (2.0 * dd - (4.0 / 3.0) * np.einsum("kL,iJ->iJkL", F, Fit) - (2.0 / 3.0) * I1 * dFit))
    vol = (2.0 * J - 1.0) * J * np.einsum("iJ,kL->iJkL", Fit, Fit) + (J - 1.0) * J * dFit
    if model == "mooney_rivlin":
        dG2 = (4.0 * np.einsum("iJ,kL->iJkL", F, F) + 2.0 * I1 * dd
               - 2.0 * (np.einsum("ik,LJ->iJkL", I3, C) + np.einsum("iL,kJ->iJkL", F, F) + np.einsum("ik,JL->iJkL", B, I3)))
        H2 = (-(4.0 / 3.0) * np.einsum("kL,iJ->iJkL", Fit, D2)
              + b * (dG2 - (4.0 / 3.0) * np.einsum("kL,iJ->iJkL", G2, Fit) - (4.0 / 3.0) * I2 * dFit))
        A = p[0] * H1 + p[1] * H2 + p[2] * vol
    else:
        _, f1, f2 = _yeoh_f(p, a * I1 - 3.0)
        A = f2 * np.einsum("iJ,kL->iJkL", D1, D1) + f1 * H1 + p[3] * vol
    return A[:d, :d, :d, :d]


def cauchy(model, p, F):
    """sigma = P F^T / J in the tensor storage (xx, yy, zz, xy, xz, yz), plane strain (xx, yy, zz, xy); model may be 'neo_hookean'"""
    d = np.asarray(F).shape[0]
    F3 = embed(F)
    s = first_pk(model, p, F3) @ F3.T / np.linalg.det(F3)
    return np.array([s[0, 0], s[1, 1], s[2, 2], s[0, 1]] + ([s[0, 2], s[1, 2]] if d == 3 else []))


def von_mises(sig):
    """sqrt(3/2 dev : dev) of stresses [.., 6 or 4] in the tensor storage"""
    sig = np.asarray(sig)
    m = sig[..., :3].mean(axis=-1, keepdims=True)
    return np.sqrt(1.5 * (((sig[..., :3] - m) ** 2).sum(axis=-1) + 2.0 * (sig[..., 3:] ** 2).sum(axis=-1)))


def gradients(X):
    """(g [d+1, d], volume) of the simplex with vertex coordinates X [d+1, d]"""
    d = X.shape[1]
    E = (X[1:] - X[0]).T
    Ei = np.linalg.inv(E)
    g = np.zeros((d + 1, d))
    g[1:] = Ei
    g[0] = -Ei.sum(axis=0)
    return g, abs(np.linalg.det(E)) / (6.0 if d == 3 else 2.0)


def element(X, U, model, p):
    """X [d+1, d], U [d+1, d] -> (V psi, f [d+1, d], K [d+1, d, d+1, d], J, sigma [6 or 4])"""
    d = X.shape[1]
    g, V = gradients(X)
    F = np.eye(d) + U.T @ g
    J = np.linalg.det(F)
    P = first_pk(model, p, F)
    A = tangent(model, p, F)
    f = V * g @ P.T
    K = V * np.einsum("iJkL,aJ,bL->aibk", A, g, g)
    return V * psi(model, p, F), f, K, J, cauchy(model, p, F)


def assemble(coords, cells, u, model, params):
    """(energy, f_int [n_dofs], K CSR, J [n_cells], sigma [n_cells, 6 or 4]); params: one row p[4] or [n_cells, 4]"""
    cells = np.asarray(cells, dtype=np.int64)
    nc, nv = cells.shape
    d = nv - 1
    coords = np.asarray(coords, dtype=np.float64)[:, :d]
    U = np.asarray(u, dtype=np.float64).reshape(-1, d)
    params = np.broadcast_to(np.asarray(params, dtype=np.float64), (nc, 4))
    n = coords.shape[0] * d
    f = np.zeros(n)
    energy = 0.0
    Js = np.empty(nc)
    sig = np.empty((nc, 6 if d == 3 else 4))
    rows, cols, vals = [], [], []
    for c in range(nc):
        vt = cells[c]
        e, fe, Ke, Js[c], sig[c] = element(coords[vt], U[vt], model, params[c])
        energy += e
        dofs = (vt[:, None] * d + np.arange(d)[None, :]).ravel()
        np.add.at(f, dofs, fe.ravel())
        rows.append(np.repeat(dofs, len(dofs)))
        cols.append(np.tile(dofs, len(dofs)))
        vals.append(Ke.reshape(len(dofs), len(dofs)).ravel())
    K = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return energy, f, K, Js, sig


def newton(coords, cells, model, params, f_ext, dofs, vals, u0=None, rtol=1e-12, atol=1e-13, max_it=50, cut_back=False):
    """Host Newton (DOLFIN's stopping test) on f_int(u) = f_ext with u[dofs] = vals.  Full steps; with cut_back a step that inverts a
    cell is halved, as the device loop does.  Returns (u, residual norms, step lengths)."""
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    n = np.asarray(coords).shape[0] * d
    u = np.zeros(n) if u0 is None else np.array(u0, dtype=np.float64)
    dofs = np.asarray(dofs, dtype=np.int64)
    u[dofs] = vals
    free = np.ones(n, dtype=bool)
    free[dofs] = False
    hist, steps = [], []
    for _ in range(max_it + 1):
        _, fi, K, J, _ = assemble(coords, cells, u, model, params)
        if not np.all(J > 0):
            raise ValueError("inverted cell in the host Newton iterate")
        r = fi - f_ext
        r[~free] = 0.0
        hist.append(np.linalg.norm(r))
        if hist[-1] < atol or hist[-1] / hist[0] < rtol:
            return u, hist, steps
        du = np.zeros(n)
        du[free] = -spla.spsolve(K[free][:, free].tocsc(), r[free])
        step = 1.0
        if cut_back:
            while not _all_positive(coords, cells, u + step * du, d):
                step *= 0.5
        steps.append(step)
        u = u + step * du
    raise RuntimeError("host Newton did not converge")


def _all_positive(coords, cells, u, d):
    X = np.asarray(coords, dtype=np.float64)[:, :d][cells]
    U = u.reshape(-1, d)[cells]
    E0 = np.swapaxes(X[:, 1:] - X[:, :1], 1, 2)
    E1 = E0 + np.swapaxes(U[:, 1:] - U[:, :1], 1, 2)
    J = np.linalg.det(E1) / np.linalg.det(E0)
    return bool(np.all(J > 0) and np.all(np.isfinite(J)))


def exact_stretch_t(model, p, s, d=3):
    """Lateral stretch t of F = diag(s, t[, t]) with free lateral faces: P_22(s, t) = 0 by a scalar Newton on this file's own P
    (derivative from its own A: dP_22/dt = A_2222 [+ A_2233])."""
    t = 1.0
    for _ in range(100):
        F = np.diag([s] + [t] * (d - 1))
        g = first_pk(model, p, F)[1, 1]
        A = tangent(model, p, F)
        dg = A[1, 1, 1, 1] + (A[1, 1, 2, 2] if d == 3 else 0.0)
        dt = -g / dg
        t += dt
        if abs(dt) < 1e-15:
            break
    else:
        raise RuntimeError("lateral stretch: no convergence")
    return t


def first_pk_11(model, p, s, t, d=3):
    return first_pk(model, p, np.diag([s] + [t] * (d - 1)))[0, 0]
