"""numpy / scipy fp64 restatement of small-strain linear viscoelasticity (generalized Maxwell solid, Prony series) on P1 cells
(ViscoelasticitySolver): the one-step recursion, the per-cell update, the history load, the effective moduli, a host time-marcher
with a sparse direct solve per step and the closed forms the tests use.  The independent check of the device kernels
(fs_viscoelasticity.hip); the reference project has no viscoelastic code.

Tensors are full 3 x 3 arrays here (plane strain: the in-plane block of the strain, zeros elsewhere; the deviator then has a zz
entry); `pack` / `unpack` of plasticity_reference convert to the device's storage.  g, tau: [n_terms] (one material) or
[n_cells, n_terms]."""
import numpy as np
import scipy.sparse.linalg as spla

import plasticity_reference as pr
from plasticity_reference import pack, unpack, gradients, strains, von_mises, I3  # noqa: F401  (re-exported)

SERIES_X = 1e-5         # below this dt / tau the series of b replaces -expm1(-x) / x


def ab(x):
    """(a, b) of h_new = a h_old + b (e_new - e_old) for x = dt / tau"""
    x = np.asarray(x, dtype=np.float64)
    small = x < SERIES_X
    xs = np.where(small, 1.0, x)
    b = np.where(small, 1.0 - x / 2.0 + x ** 2 / 6.0 - x ** 3 / 24.0, -np.expm1(-xs) / xs)
    return np.exp(-x), b


def _terms(g, tau, n):
    g = np.asarray(g, dtype=np.float64)
    tau = np.asarray(tau, dtype=np.float64)
    nt = g.shape[-1] if g.ndim else 0
    return np.broadcast_to(g, (n, nt)), np.broadcast_to(tau, (n, nt))


def effective_moduli(mu0, lm0, g, tau, dt):
    """(mu_eff, lambda_eff) [n] of the step operator; dt None: the long-term moduli"""
    mu0 = np.atleast_1d(np.asarray(mu0, dtype=np.float64))
    n = max(mu0.size, np.size(lm0), np.asarray(g).shape[0] if np.ndim(g) == 2 else 1)
    g, tau = _terms(g, tau, n)
    f = 1.0 - g.sum(axis=1)
    if dt is not None:
        f = f + (g * ab(dt / tau)[1]).sum(axis=1)
    mu = mu0 * f
    K = np.asarray(lm0, dtype=np.float64) + 2.0 * mu0 / 3.0
    return mu, K - 2.0 * mu / 3.0


def dev(eps):
    return eps - np.trace(eps, axis1=1, axis2=2)[:, None, None] * I3 / 3.0


def update(eps, e_old, h_old, mu0, lm0, g, tau, dt):
    """eps, e_old [n,3,3], h_old [n,nt,3,3] -> (e_new, h_new, sigma)"""
    n = eps.shape[0]
    g, tau = _terms(g, tau, n)
    mu0, lm0 = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (mu0, lm0))
    a, b = ab(dt / tau)
    e = dev(eps)
    h = a[:, :, None, None] * h_old + b[:, :, None, None] * (e - e_old)[:, None]
    ginf = 1.0 - g.sum(axis=1)
    K = lm0 + 2.0 * mu0 / 3.0
    tr = np.trace(eps, axis1=1, axis2=2)
    sig = (K * tr)[:, None, None] * I3 + 2.0 * mu0[:, None, None] * (ginf[:, None, None] * e + (g[:, :, None, None] * h).sum(axis=1))
    return e, h, sig


def s_hist(e_old, h_old, mu0, g, tau, dt):
    n = e_old.shape[0]
    g, tau = _terms(g, tau, n)
    mu0 = np.broadcast_to(np.asarray(mu0, dtype=np.float64), (n,))
    a, b = ab(dt / tau)
    return 2.0 * mu0[:, None, None] * (g[:, :, None, None] * (a[:, :, None, None] * h_old - b[:, :, None, None] * e_old[:, None])).sum(axis=1)


def internal_force(coords, cells, sig):
    """int B^T sigma dx [n_dofs] for a per-cell stress [nc,3,3]"""
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    g, V = gradients(coords, cells)
    fe = V[:, None, None] * np.einsum("nij,naj->nai", sig[:, :d, :d], g)
    dofs = cells[:, :, None] * d + np.arange(d)[None, None, :]
    return np.bincount(dofs.ravel(), weights=fe.ravel(), minlength=np.asarray(coords).shape[0] * d)


def history_load(coords, cells, e_old, h_old, mu0, g, tau, dt):
    return -internal_force(coords, cells, s_hist(e_old, h_old, mu0, g, tau, dt))


def stiffness(coords, cells, mu, lm):
    """the linear elasticity operator (CSR) of per-cell or constant (mu, lambda): the elastic branch of the plasticity reference"""
    cells = np.asarray(cells, dtype=np.int64)
    nc, d = len(cells), cells.shape[1] - 1
    z = np.zeros(np.asarray(coords).shape[0] * d)
    return pr.assemble(coords, cells, z, np.zeros((nc, 3, 3)), np.zeros(nc), mu, lm, 1e300, 0.0)["K"]


def elastic_solve(coords, cells, mu, lm, f, dofs, vals):
    K = stiffness(coords, cells, mu, lm)
    u = np.zeros(f.size)
    dofs = np.asarray(dofs, dtype=np.int64)
    u[dofs] = vals
    free = np.ones(f.size, dtype=bool)
    free[dofs] = False
    rhs = (f - K @ u)[free]
    u[free] = spla.spsolve(K[free][:, free].tocsc(), rhs)
    return u


def march(coords, cells, mat, steps):
    """mat = (mu0, lambda0, g, tau); steps: per step (dt, f_ext, dofs, vals).  From the zero state.  Returns per step a dict: u, e, h,
    sigma (after the step), f_hist (the history load the step used)."""
    cells = np.asarray(cells, dtype=np.int64)
    nc, d = len(cells), cells.shape[1] - 1
    mu0, lm0, g, tau = mat
    g, tau = _terms(g, tau, nc)
    e, h = np.zeros((nc, 3, 3)), np.zeros((nc, g.shape[1], 3, 3))
    out = []
    cache = {}
    for dt, f_ext, dofs, vals in steps:
        if dt not in cache:
            cache[dt] = effective_moduli(mu0, lm0, g, tau, dt)
        mu_e, lm_e = cache[dt]
        fh = history_load(coords, cells, e, h, mu0, g, tau, dt)
        u = elastic_solve(coords, cells, mu_e, lm_e, f_ext + fh, dofs, vals)
        e, h, sig = update(strains(coords, cells, u)[0], e, h, mu0, lm0, g, tau, dt)
        out.append({"u": u, "e": e, "h": h, "sigma": sig, "f_hist": fh})
    return out


def relaxation_modulus(G0, g, tau, t):
    g, tau = np.asarray(g, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    return G0 * (1.0 - g.sum() + (g * np.exp(-t / tau)).sum())


def shear_ramp(G0, gamma0, g, tau, t1, t):
    """sigma_xy(t), 0 <= t <= t1, during the linear ramp gamma = gamma0 t / t1: G0 (gamma0/t1) [g_inf t + sum g_k tau_k (1 - exp(-t/tau_k))]"""
    g, tau = np.asarray(g, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    return G0 * (gamma0 / t1) * ((1.0 - g.sum()) * t + (g * tau * (-np.expm1(-t / tau))).sum())


def shear_ramp_hold(G0, gamma0, g, tau, t1, t):
    """sigma_xy(t), t >= t1, for simple shear u = gamma(t) y e_x with gamma ramped linearly to gamma0 over [0, t1] and held:
    eps_xy = gamma/2, so sigma_xy = 2 G0 [g_inf gamma0/2 + sum g_k h_k,xy], h_k(t) = (gamma0/2)(tau_k/t1)(1 - exp(-t1/tau_k))
    exp(-(t - t1)/tau_k)."""
    g, tau = np.asarray(g, dtype=np.float64), np.asarray(tau, dtype=np.float64)
    return G0 * gamma0 * (1.0 - g.sum() + (g * (tau / t1) * (-np.expm1(-t1 / tau)) * np.exp(-(t - t1) / tau)).sum())
