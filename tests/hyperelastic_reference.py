"""numpy restatement of the compressible neo-Hookean P1 element (NonlinearElasticitySolver.py:41-98): energy V psi, internal
force f_a = V P g_a and tangent K_ab, global assembly into scipy CSR and a host Newton with spsolve.  The independent check of
the device kernels (fs_hyper.hip)."""
import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla


def element(X, U, mu, lmbda):
    """X [d+1, d] vertex coordinates, U [d+1, d] displacements -> (V psi, f [d+1, d], K [d+1, d, d+1, d], J)."""
    d = X.shape[1]
    E = (X[1:] - X[0]).T                       # columns: edge vectors
    Ei = np.linalg.inv(E)
    g = np.zeros((d + 1, d))
    g[1:] = Ei
    g[0] = -Ei.sum(axis=0)
    V = abs(np.linalg.det(E)) / (6.0 if d == 3 else 2.0)
    H = U.T @ g                                 # H[i, j] = sum_a U[a, i] g[a, j]
    F = np.eye(d) + H
    J = np.linalg.det(F)
    FiT = np.linalg.inv(F).T
    lj = np.log(J)
    ic3 = 2.0 * np.trace(H) + np.sum(H * H) + (d - 3.0)     # tr C - 3 (2-D: the reference's Identity(2) with 3)
    energy = V * (0.5 * mu * ic3 - mu * lj + 0.5 * lmbda * lj * lj)
    P = mu * (F - FiT) + lmbda * lj * FiT
    f = V * g @ P.T                              # f[a, i] = V sum_j P[i, j] g[a, j]
    G = g @ FiT.T                                # G[a, i] = (F^-T g_a)_i
    gg = g @ g.T
    K = V * (lmbda * np.einsum("ai,bk->aibk", G, G) + (mu - lmbda * lj) * np.einsum("ak,bi->aibk", G, G)
             + mu * np.einsum("ab,ik->aibk", gg, np.eye(d)))
    return energy, f, K, J


def assemble(coords, cells, u, mu, lmbda):
    """(energy, f_int [n_dofs], K CSR, J per cell) of the whole mesh; mu / lmbda numbers or arrays [n_cells]."""
    coords = np.asarray(coords, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    nc, nv = cells.shape
    d = nv - 1
    coords = coords[:, :d]
    U = np.asarray(u, dtype=np.float64).reshape(-1, d)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (nc,))
    lmbda = np.broadcast_to(np.asarray(lmbda, dtype=np.float64), (nc,))
    n = coords.shape[0] * d
    f = np.zeros(n)
    energy = 0.0
    Js = np.empty(nc)
    rows, cols, vals = [], [], []
    for c in range(nc):
        vt = cells[c]
        e, fe, Ke, Js[c] = element(coords[vt], U[vt], mu[c], lmbda[c])
        energy += e
        dofs = (vt[:, None] * d + np.arange(d)[None, :]).ravel()
        np.add.at(f, dofs, fe.ravel())
        rows.append(np.repeat(dofs, len(dofs)))
        cols.append(np.tile(dofs, len(dofs)))
        vals.append(Ke.reshape(len(dofs), len(dofs)).ravel())
    K = sps.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    return energy, f, K, Js


def newton(coords, cells, mu, lmbda, f_ext, dofs, vals, u0=None, rtol=1e-12, atol=1e-13, max_it=50):
    """Host Newton (DOLFIN's stopping test) on f_int(u) = f_ext with u[dofs] = vals; full steps.  Returns (u, residual norms)."""
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    n = np.asarray(coords).shape[0] * d
    u = np.zeros(n) if u0 is None else np.array(u0, dtype=np.float64)
    dofs = np.asarray(dofs, dtype=np.int64)
    u[dofs] = vals
    free = np.ones(n, dtype=bool)
    free[dofs] = False
    hist = []
    for _ in range(max_it + 1):
        _, fi, K, J = assemble(coords, cells, u, mu, lmbda)
        if not np.all(J > 0):
            raise ValueError("inverted cell in the host Newton iterate")
        r = fi - f_ext
        r[~free] = 0.0
        hist.append(np.linalg.norm(r))
        if hist[-1] < atol or hist[-1] / hist[0] < rtol:
            return u, hist
        Kf = K[free][:, free]
        u[free] -= spla.spsolve(Kf.tocsc(), r[free])
    raise RuntimeError("host Newton did not converge")


def exact_stretch_t(s, mu, lmbda, d=3):
    """Lateral stretch t of the homogeneous uniaxial state F = diag(s, t[, t]) with free lateral faces:
    mu (t^2 - 1) + lambda ln(s t^(d-1)) = 0 (Newton from t = 1)."""
    t = 1.0
    for _ in range(100):
        g = mu * (t * t - 1.0) + lmbda * np.log(s * t ** (d - 1))
        dg = 2.0 * mu * t + lmbda * (d - 1) / t
        dt = -g / dg
        t += dt
        if abs(dt) < 1e-16:
            break
    return t


def first_pk_11(s, t, mu, lmbda, d=3):
    """P_11 of F = diag(s, t[, t]): mu (s - 1/s) + lambda ln J / s."""
    J = s * t ** (d - 1)
    return mu * (s - 1.0 / s) + lmbda * np.log(J) / s
