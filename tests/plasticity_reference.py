"""numpy / scipy fp64 restatement of small-strain J2 plasticity with linear isotropic hardening on P1 cells (PlasticitySolver): the
radial return with its consistent tangent, the element, global assembly into scipy CSR and a host Newton with a sparse direct
solve.  The independent check of the device kernels (fs_plasticity.hip); the reference project has no plasticity code.

Tensors are full 3 x 3 arrays here (plane strain: the in-plane block of the strain, zeros elsewhere); `pack` / `unpack` convert
to the device's storage (xx, yy, zz, xy, xz, yz) in 3-D and (xx, yy, zz, xy) in plane strain."""
import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla

I3 = np.eye(3)
R32 = np.sqrt(1.5)
_IDX = {3: ((0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)), 2: ((0, 0), (1, 1), (2, 2), (0, 1))}


def pack(T, d):
    """[n, 3, 3] symmetric tensors -> [n, 6] (3-D) or [n, 4] (plane strain)"""
    return np.stack([T[:, i, j] for i, j in _IDX[d]], axis=1)


def unpack(a, d):
    a = np.asarray(a, dtype=np.float64)
    T = np.zeros((a.shape[0], 3, 3))
    for k, (i, j) in enumerate(_IDX[d]):
        T[:, i, j] = a[:, k]
        T[:, j, i] = a[:, k]
    return T


def return_map(eps, ep, p, mu, lmbda, sy, H, tangent=True):
    """eps, ep [n, 3, 3], p [n]; material numbers or [n].  Returns (sigma [n,3,3], ep_new, p_new, f [n], D [n,3,3,3,3] or None)."""
    n = eps.shape[0]
    mu, lmbda, sy, H = (np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in (mu, lmbda, sy, H))
    e = eps - ep
    tr = np.trace(e, axis1=1, axis2=2)
    K = lmbda + 2.0 * mu / 3.0
    s = 2.0 * mu[:, None, None] * (e - tr[:, None, None] * I3 / 3.0)
    sn = np.sqrt(np.einsum("nij,nij->n", s, s))
    q = R32 * sn
    f = q - (sy + H * p)
    sig = K[:, None, None] * tr[:, None, None] * I3 + s
    y = f > 0.0
    dp = np.where(y, f / (3.0 * mu + H), 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        N = np.where(y[:, None, None], s / sn[:, None, None], 0.0)
        beta = np.where(y, 3.0 * mu * dp / q, 0.0)
    sig = sig - (2.0 * mu * dp * R32)[:, None, None] * N
    ep_new = ep + (R32 * dp)[:, None, None] * N
    p_new = p + dp
    if not tangent:
        return sig, ep_new, p_new, f, None
    Isym = 0.5 * (np.einsum("ik,jl->ijkl", I3, I3) + np.einsum("il,jk->ijkl", I3, I3))
    II = np.einsum("ij,kl->ijkl", I3, I3)
    Idev = Isym - II / 3.0
    C = lmbda[:, None, None, None, None] * II + 2.0 * mu[:, None, None, None, None] * Isym
    cN = np.where(y, 2.0 * mu * (3.0 * mu / (3.0 * mu + H) - beta), 0.0)
    D = C - (2.0 * mu * beta)[:, None, None, None, None] * Idev - cN[:, None, None, None, None] * np.einsum("nij,nkl->nijkl", N, N)
    return sig, ep_new, p_new, f, D


def gradients(coords, cells):
    """(g [nc, d+1, d] barycentric gradients, V [nc] volumes / areas)"""
    coords = np.asarray(coords, dtype=np.float64)
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    X = coords[:, :d][cells]
    E = np.transpose(X[:, 1:] - X[:, :1], (0, 2, 1))            # columns: edge vectors
    Ei = np.linalg.inv(E)
    g = np.zeros((len(cells), d + 1, d))
    g[:, 1:] = Ei
    g[:, 0] = -Ei.sum(axis=1)
    V = np.abs(np.linalg.det(E)) / (6.0 if d == 3 else 2.0)
    return g, V


def strains(coords, cells, u):
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    g, V = gradients(coords, cells)
    U = np.asarray(u, dtype=np.float64).reshape(-1, d)[cells]
    Hm = np.einsum("nai,naj->nij", U, g)
    eps = np.zeros((len(cells), 3, 3))
    eps[:, :d, :d] = 0.5 * (Hm + np.transpose(Hm, (0, 2, 1)))
    return eps, g, V


def assemble(coords, cells, u, ep, p, mu, lmbda, sy, H, tangent=True):
    """State at the displacement u from the committed history (ep [nc,3,3], p [nc]).  Returns a dict: f (internal force), K (CSR or
    None), sigma, ep (trial), p (trial), fy (the yield function of the trial state per cell)."""
    cells = np.asarray(cells, dtype=np.int64)
    nc, nv = cells.shape
    d = nv - 1
    eps, g, V = strains(coords, cells, u)
    sig, ep1, p1, fy, D = return_map(eps, ep, p, mu, lmbda, sy, H, tangent)
    n = np.asarray(coords).shape[0] * d
    fe = V[:, None, None] * np.einsum("nij,naj->nai", sig[:, :d, :d], g)
    dofs = cells[:, :, None] * d + np.arange(d)[None, None, :]
    f = np.bincount(dofs.ravel(), weights=fe.ravel(), minlength=n)
    K = None
    if tangent:
        Ke = V[:, None, None, None, None] * np.einsum("naj,nijkl,nbl->naibk", g, D[:, :d, :d, :d, :d], g)
        nd = nv * d
        dd = dofs.reshape(nc, nd)
        rows = np.repeat(dd, nd, axis=1).ravel()
        cols = np.tile(dd, (1, nd)).ravel()
        K = sps.csr_matrix((Ke.reshape(nc, nd * nd).ravel(), (rows, cols)), shape=(n, n))
    return {"f": f, "K": K, "sigma": sig, "ep": ep1, "p": p1, "fy": fy}


def newton_step(coords, cells, mat, f_ext, dofs, vals, u0, ep, p, rtol=1e-9, atol=1e-10, max_it=50):
    """One load step: Newton (DOLFIN's stopping test, full steps) on f_int(u; ep, p) = f_ext with u[dofs] = vals, starting from u0.
    Returns (u, state of the converged iterate, residual norms)."""
    cells = np.asarray(cells, dtype=np.int64)
    u = np.array(u0, dtype=np.float64)
    dofs = np.asarray(dofs, dtype=np.int64)
    u[dofs] = vals
    free = np.ones(u.size, dtype=bool)
    free[dofs] = False
    hist = []
    for _ in range(max_it + 1):
        st = assemble(coords, cells, u, ep, p, *mat)
        r = st["f"] - f_ext
        r[~free] = 0.0
        hist.append(np.linalg.norm(r))
        if hist[-1] < atol or (hist[0] > 0 and hist[-1] / hist[0] < rtol):
            return u, st, hist
        Kf = st["K"][free][:, free]
        u[free] -= spla.spsolve(Kf.tocsc(), r[free])
    raise RuntimeError("host Newton did not converge")


def solve_steps(coords, cells, mat, loads, rtol=1e-9, atol=1e-10):
    """loads: per step (f_ext, dofs, vals).  Returns per step a dict: u, p, ep, sigma, fy (at the converged iterate, from the history
    the step started with), iterations."""
    cells = np.asarray(cells, dtype=np.int64)
    nc, d = len(cells), cells.shape[1] - 1
    u = np.zeros(np.asarray(coords).shape[0] * d)
    ep, p = np.zeros((nc, 3, 3)), np.zeros(nc)
    out = []
    for f_ext, dofs, vals in loads:
        u, st, hist = newton_step(coords, cells, mat, f_ext, dofs, vals, u, ep, p, rtol, atol)
        ep, p = st["ep"], st["p"]
        out.append({"u": u.copy(), "p": p.copy(), "ep": ep.copy(), "sigma": st["sigma"], "fy": st["fy"], "iterations": len(hist) - 1,
                    "history": hist})
    return out


def von_mises(sig):
    s = sig - np.trace(sig, axis1=1, axis2=2)[:, None, None] * I3 / 3.0
    return R32 * np.sqrt(np.einsum("nij,nij->n", s, s))


def uniaxial(eps_hist, E, nu, sy, H):
    """Closed form of the uniaxial stress path for a strain history eps_xx (monotone pieces): per step (sigma_xx, p, lateral strain).
    1-D return mapping with the tangent modulus E_t = E H / (E + H)."""
    out = []
    p = 0.0
    for e in eps_hist:
        s_tr = E * (e - _ep(out))
        f = abs(s_tr) - (sy + H * p)
        if f > 0:
            dp = f / (E + H)
            p += dp
            epx = _ep(out) + dp * np.sign(s_tr)
            s = s_tr - E * dp * np.sign(s_tr)
        else:
            epx = _ep(out)
            s = s_tr
        out.append((s, p, -nu * s / E - epx / 2.0, epx))
    return [(s, p, lat) for s, p, lat, _ in out]


def _ep(out):
    return out[-1][3] if out else 0.0
