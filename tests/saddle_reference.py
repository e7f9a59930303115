"""Host replay of the two block preconditioners of fs_saddle_solve (fs_saddle_solve.inc: sd_precond and sd_precond_ld, step for step), of
its eigenvalue estimate, of the small dense algebra behind its Arnoldi state and of the iteration itself (host_fgmres, plain
float64), with a componentwise forward-error bound carried next to every vector of the preconditioners.  Shared by test_saddle_reference_host.py (the replays against explicit dense extended-precision operators on
the CPU) and test_gpu_saddle_replay.py (the device against the replays).  Plain numpy / scipy, no GPU.

The bounds follow the rules at the top of amg_reference.py: a product y = Op x leaves with |Op| e_x + t_row eps (|Op| |x|)_row, an
element-wise update with the bounds of its inputs times the magnitudes of their coefficients + 2 eps (the sum of the magnitudes of
its terms); the V-cycle in the middle carries the bound that its right-hand side arrives with through the moduli of its maps
(vcycle_replay(..., e_r=...)).  The Chebyshev polynomials here are short (at most five steps on the mass matrix, velocity_sweeps on
the velocity block), so their bounds are chained operation by operation: about a factor of 3.5 per step on the Jacobi-scaled P1
mass matrix, 2e2 eps in all, which stays four orders inside the tightness condition.  The constants of the polynomials (theta,
delta, sigma, rho) are the same IEEE double operations in the same order as in the library and carry no bound of their own, and so
do the inverse diagonals: 1 / J_ii (0 where the diagonal is zero, as k_sd_diag forms it) and 1 / Mp_ii (1 where it is zero,
k_sd_scalar_dinv).

Layout of the block vectors: four unknowns per node (u_x, u_y, u_z, p), the nv vertex nodes first; the pressure slot of an edge node
of a Taylor-Hood space is a dummy unknown."""
import numpy as np
import scipy.sparse as sp

from amg_reference import LD, TIGHT, _add, _product, _round, _sub, vcycle_replay  # noqa: F401
from spmv_reference import EPS, _host_product


def jacobi_dinv(J):
    """k_sd_diag: 1 / diagonal, 0 where the diagonal is zero."""
    d = sp.csr_matrix(J).diagonal()
    return np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 0.0)


def scalar_dinv(M):
    """k_sd_scalar_dinv: 1 / diagonal, 1 where the diagonal is zero."""
    d = sp.csr_matrix(M).diagonal()
    return np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)


def chebyshev_constants(lo, up, steps):
    """(c1 of the first step, [(c1, c2) of the later steps]) of d = c2 d + c1 dinv (b - A x): sd_precond's operations, in its order."""
    theta, delta = 0.5 * (up + lo), 0.5 * (up - lo)
    sigma = theta / delta
    rho_c = 1.0 / sigma
    later = []
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho_c)
        later.append((2.0 * rho_new / delta, rho_new * rho_c))
        rho_c = rho_new
    return 1.0 / theta, later


def _chebyshev(A, absA, dinv, b, eb, lo, up, steps, keep=None):
    """k_sd_cheb / k_sd_vel_cheb: x after `steps` steps from a zero guess and its bound.  keep: the components the polynomial acts
    on (None = all); the others of x and d are 0, exactly."""
    first, later = chebyshev_constants(lo, up, steps)
    mask = np.ones(len(b)) if keep is None else keep.astype(np.float64)
    d = _round(LD(first) * dinv.astype(LD) * b.astype(LD)) * mask
    ed = (np.abs(first * dinv) * eb + 2.0 * EPS * np.abs(d)) * mask
    x, ex = d.copy(), ed.copy()
    for c1, c2 in later:
        t, et = _product(A, absA, x, ex)
        t1 = LD(c2) * d.astype(LD)
        t2 = LD(c1) * dinv.astype(LD) * (b.astype(LD) - t.astype(LD))
        ed = (abs(c2) * ed + np.abs(c1 * dinv) * (eb + et)
              + 2.0 * EPS * (np.abs(_round(t1)) + np.abs(c1 * dinv) * (np.abs(b) + np.abs(t)))) * mask
        d = _round(t1 + t2) * mask
        x, ex = _add(x, ex, d, ed)
        x, ex = x * mask, ex * mask
    return x, ex


def mass_chebyshev(Mp, rp, erp):
    """The five Chebyshev steps on the Jacobi-scaled P1 mass matrix over [1/2, 5/2] (Wathen) that stand in for Mp^-1."""
    Mp = sp.csr_matrix(Mp)
    return _chebyshev(Mp, abs(Mp), scalar_dinv(Mp), rp, erp, 0.5, 2.5, 5)


def identity_pressure_rows(J, nv):
    """k_sd_ident_p: the vertex rows whose (3, 3) diagonal entry is not zero (a Dirichlet pressure)."""
    return sp.csr_matrix(J).diagonal()[3:4 * nv:4] != 0.0


def identity_pressure_rows_ld(J, nv):
    """k_ld_ident_p: the pressure rows that hold a unit (3, 3) diagonal and nothing else."""
    J = sp.csr_matrix(J)
    rows = J[3:4 * nv:4]
    one = sp.csr_matrix((np.ones(nv), (np.arange(nv), 4 * np.arange(nv) + 3)), shape=rows.shape)
    diff = abs(rows - one)
    return np.asarray(diff.max(axis=1).todense()).ravel() == 0.0


def cahouet_chabard_replay(J, Mp, levels, opts, r):
    """z = P^-1 r of sd_precond and the bound e_z of |z_device - z|.  J, Mp: scipy CSR copies of the device matrices (to_csr);
    levels: the hierarchy of Kp for amg_reference.vcycle_replay (list of level dicts or the output of prepare()), None without the
    term Kp^-1 (steady); opts: {"nu", "rho", "inv_dt", "velocity_sweeps", "vel_lmax" (with more than one sweep), "nv",
    "smoother_steps" (2), "coarse" (the dense inverse of the coarsest level or None)}."""
    J = sp.csr_matrix(J)
    n, nv = J.shape[0], int(opts["nv"])
    r = np.asarray(r, dtype=np.float64)
    vel = (np.arange(n) & 3) != 3
    dinv = jacobi_dinv(J)
    sweeps = max(int(opts.get("velocity_sweeps", 1)), 1)
    zero = np.zeros(n)
    if sweeps == 1:
        zu = _round(dinv.astype(LD) * r.astype(LD)) * vel
        ezu = 2.0 * EPS * np.abs(zu)
    else:
        lmax = float(opts["vel_lmax"])
        zu, ezu = _chebyshev(J, abs(J), dinv, r, zero, lmax / 8.0, 1.1 * lmax, sweeps, keep=vel)
    # rp = r_p - (D z_u): planes (3, 0..2) of the vertex rows
    prow = 4 * np.arange(nv) + 3
    D = sp.csr_matrix(J[prow] @ sp.diags(vel.astype(np.float64)))
    D.eliminate_zeros()
    t, et = _product(D, abs(D), zu, ezu)
    rp, erp = _sub(r[prow], np.zeros(nv), t, et + 2.0 * EPS * (abs(D) @ np.abs(zu)))       # (the four partial sums of a row)
    transient = float(opts.get("inv_dt", 0.0)) > 0.0 and levels is not None
    if transient:
        p1, ep1 = vcycle_replay(levels, rp, int(opts.get("smoother_steps", 2)), opts.get("coarse"), e_r=erp)
    p2, ep2 = mass_chebyshev(Mp, rp, erp)
    r2 = float(opts["rho"]) * float(opts["rho"])
    c1, c2 = r2 * float(opts.get("inv_dt", 0.0)), r2 * float(opts["nu"])
    zp = LD(c2) * p2.astype(LD)
    ezp = abs(c2) * ep2 + 2.0 * EPS * np.abs(c2 * p2)
    if transient:
        zp = zp + LD(c1) * p1.astype(LD)
        ezp = ezp + abs(c1) * ep1 + 2.0 * EPS * np.abs(c1 * p1) + 2.0 * EPS * np.abs(_round(zp))
    ident = identity_pressure_rows(J, nv)
    z, ez = zu.copy(), ezu.copy()
    z[3::4], ez[3::4] = r[3::4], 0.0                       # dummy pressure slots of the edge nodes: z = r
    z[prow] = np.where(ident, r[prow], _round(zp))
    ez[prow] = np.where(ident, 0.0, ezp)
    return z, ez


def block_upper_replay(J, Mp, levels, opts, r):
    """z = [A J_vp; 0 S]^-1 r of sd_precond_ld and its bound.  J: the reduced large-deformation operator (CG1, four unknowns per
    vertex); levels: the hierarchy of a0; opts: {"schur_scale", "tdim", "smoother_steps" (2), "coarse"}.  levels = None (no
    hierarchy: the library runs an inner CG on a0, which is no fixed operator): the tdim velocity components of z come back as NaN
    with an infinite bound, the pressure rows and the 2-D dummy slot, which do not depend on the velocity solve, as always."""
    J = sp.csr_matrix(J)
    n = J.shape[0]
    nv, d = n // 4, int(opts["tdim"])
    r = np.asarray(r, dtype=np.float64)
    prow = 4 * np.arange(nv) + 3
    p2, ep2 = mass_chebyshev(Mp, r[prow], np.zeros(nv))
    c = 1.0 / float(opts["schur_scale"])
    ident = identity_pressure_rows_ld(J, nv)
    y, ey = np.zeros(n), np.zeros(n)
    y[prow] = np.where(ident, r[prow], _round(LD(c) * p2.astype(LD)))
    ey[prow] = np.where(ident, 0.0, abs(c) * ep2 + 2.0 * EPS * np.abs(c * p2))
    jy, ejy = _product(J, abs(J), y, ey)
    vrow = (4 * np.arange(nv)[:, None] + np.arange(d)).ravel()
    t, et = _sub(r[vrow], np.zeros(len(vrow)), jy[vrow], ejy[vrow])
    if levels is None:
        zv, ezv = np.full(len(vrow), np.nan), np.full(len(vrow), np.inf)
    else:
        zv, ezv = vcycle_replay(levels, t, int(opts.get("smoother_steps", 2)), opts.get("coarse"), e_r=et)
    z, ez = np.zeros(n), np.zeros(n)
    z[vrow], ez[vrow] = zv, ezv
    if d == 2:
        z[2::4] = r[2::4]
    z[prow], ez[prow] = y[prow], ey[prow]
    return z, ez


def check_inside(z, z_ref, e_z, what, rows=None):
    """|z - z_ref| <= e_z in every component (of `rows`, if given); returns (largest err / e_z, max(e_z) / max|z_ref|)."""
    if rows is not None:
        z, z_ref, e_z = z[rows], z_ref[rows], e_z[rows]
    assert np.all(np.isfinite(z)), (what, "non-finite entries")
    err = np.abs(z - z_ref)
    ratio = float((err / np.maximum(e_z, 1e-300))[(err > 0) | (e_z > 0)].max(initial=0.0))
    bad = err > e_z
    assert not bad.any(), (what, "outside the bound", int(bad.sum()), np.flatnonzero(bad)[:8], ratio)
    return ratio, float(e_z.max() / np.abs(z_ref).max())


# ---- the eigenvalue estimate of the velocity block ------------------------------------------------------------------------------
def hashed_seed(n):
    """k_sd_seed: a hashed start vector in [-1, 1), 0 on the pressure components."""
    i = np.arange(n, dtype=np.uint64)
    m = np.uint64(0xffffffff)
    x = (i * np.uint64(2654435761) + np.uint64(12345)) & m
    x ^= x >> np.uint64(16)
    x = (x * np.uint64(0x7feb352d)) & m
    x ^= x >> np.uint64(15)
    x = (x * np.uint64(0x846ca68b)) & m
    x ^= x >> np.uint64(16)
    v = (x & np.uint64(0xffffff)).astype(np.float64) / 8388608.0 - 1.0
    v[3::4] = 0.0
    return v


def power_lmax(J, dinv=None, extended=True):
    """The 12 power iterations on D^-1 J, velocity components only, from the hashed seed: vel_lmax of fs_saddle_solve.  extended:
    products and norms in extended precision rounded once; else plain float64 in scipy's order of summation."""
    J = sp.csr_matrix(J)
    n = J.shape[0]
    dinv = jacobi_dinv(J) if dinv is None else dinv
    vel = (np.arange(n) & 3) != 3
    w = hashed_seed(n)
    lam = 1.0
    for it in range(12):
        nn = float(np.sqrt(np.sum(w.astype(LD) ** 2))) if extended else float(np.sqrt(w @ w))
        if not nn > 0.0:
            break
        if it > 0:
            lam = nn
        z = (1.0 / nn) * w
        t = _host_product(J, z)[0] if extended else J @ z
        w = np.where(vel, dinv * t, 0.0)
    return lam


def velocity_lambda_true(J):
    """The largest eigenvalue of D^-1 A on the velocity block (dense; the block need not be symmetric: largest real part)."""
    J = sp.csr_matrix(J)
    vel = np.flatnonzero((np.arange(J.shape[0]) & 3) != 3)
    A = J[vel][:, vel].toarray()
    d = np.diag(A)
    keep = d != 0.0
    A = A[keep][:, keep] / d[keep][:, None]
    if len(A) > 1200:
        from scipy.sparse.linalg import eigs
        return float(eigs(sp.csr_matrix(A), k=1, which="LR", tol=1e-12, v0=np.ones(len(A)))[0].real[0])
    return float(np.linalg.eigvals(A).real.max())


# ---- the small dense algebra of the Arnoldi state -------------------------------------------------------------------------------
def hessenberg_from_rotations(R, cs, sn, k):
    """Hbar [k + 1, k] = Q^T [R; 0]: the Hessenberg matrix before the Givens rotations (cs_i, sn_i) on rows i, i + 1 turned its first
    k columns into the upper triangular R (k_sd_givens: a' = cs a + sn c, c' = -sn a + cs c, column j by rotations 0 .. j)."""
    H = np.zeros((k + 1, k), dtype=LD)
    H[:k, :] = np.triu(np.asarray(R, dtype=LD)[:k, :k])
    for j in range(k):
        for i in range(j, -1, -1):
            a, c = H[i, j], H[i + 1, j]
            H[i, j] = LD(cs[i]) * a - LD(sn[i]) * c
            H[i + 1, j] = LD(sn[i]) * a + LD(cs[i]) * c
    return H.astype(np.float64)


def least_squares(Hbar, beta):
    """(y, ||beta e1 - Hbar y||) of the small least-squares problem of a GMRES cycle."""
    rhs = np.zeros(Hbar.shape[0])
    rhs[0] = beta
    y = np.linalg.lstsq(Hbar, rhs, rcond=None)[0]
    return y, float(np.linalg.norm(rhs - Hbar @ y))


def two_pass_arnoldi(JZ, v0):
    """The reference of the orthogonality check: the columns of JZ orthogonalised against v0 and each other by two full
    Gram-Schmidt passes in float64.  Returns V [k + 1, n]."""
    V = [v0 / np.linalg.norm(v0)]
    for w in JZ:
        w = w.copy()
        for _ in range(2):
            B = np.array(V)
            w = w - B.T @ (B @ w)
        V.append(w / np.linalg.norm(w))
    return np.array(V)


def orthogonality_loss(V):
    V = np.asarray(V)
    return float(np.abs(V @ V.T - np.eye(len(V))).max())


# ---- the iteration itself, restated -----------------------------------------------------------------------------------------------
GATE = 0.5                    # k_sd_hess_pass: a second Gram-Schmidt pass unless hh^2 > GATE ||w||^2


def host_fgmres(J, precond, b, x0=None, restart=60, max_iter=600, rtol=0.0, atol=0.0, gate=GATE):
    """fs_saddle_solve's iteration in float64: restarted FGMRES, classical Gram-Schmidt with a gated second pass, the new norm by
    Pythagoras, Givens rotations, the true residual at every restart.  precond(r) -> z.  Returns a dict: x, iterations, converged,
    history (the recurrence residual after every iteration), ratios (hh^2 / ||w||^2 of the first pass per iteration),
    second_passes, loss (largest |V^T V - I| per cycle), true (the true residual at every restart), cycle (the state of the last cycle
    in the form of backend.saddle_last_cycle())."""
    J = sp.csr_matrix(J)
    n = J.shape[0]
    x = np.zeros(n) if x0 is None else np.array(x0, dtype=np.float64)
    thr = max(rtol * float(np.linalg.norm(b)), atol)
    out = {"history": [], "ratios": [], "second_passes": 0, "loss": [], "true": []}
    it, conv = 0, 0
    while True:
        r = b - J @ x
        res = float(np.linalg.norm(r))
        out["true"].append(res)
        if res <= thr:
            conv = 1
            break
        if it >= max_iter:
            break
        m = restart
        V, Z = [r / res], []
        H = np.zeros((m + 1, m))
        cs, sn, gam = np.zeros(m), np.zeros(m), np.zeros(m + 1)
        gam[0] = res
        k, stop, passes = 0, False, 0
        while k < m and it + k < max_iter and not stop:
            z = precond(V[k])
            Z.append(z)
            w = J @ z
            B = np.array(V)
            before = float(w @ w)
            h = B @ w
            H[:k + 1, k] = h
            hh2 = before - float(h @ h)
            w = w - B.T @ h
            out["ratios"].append(hh2 / before if before > 0 else 0.0)
            if not hh2 > gate * before:
                out["second_passes"] += 1
                passes += 1
                before = float(w @ w)
                h = B @ w
                H[:k + 1, k] += h
                hh2 = before - float(h @ h)
                w = w - B.T @ h
            hh = np.sqrt(hh2) if hh2 > 0 else 0.0
            H[k + 1, k] = hh
            for j in range(k):
                a, c = H[j, k], H[j + 1, k]
                H[j, k], H[j + 1, k] = cs[j] * a + sn[j] * c, -sn[j] * a + cs[j] * c
            a, c = H[k, k], H[k + 1, k]
            d = np.sqrt(a * a + c * c)
            cs[k], sn[k] = (a / d, c / d) if d > 0 else (1.0, 0.0)
            H[k, k], H[k + 1, k] = d, 0.0
            gam[k + 1] = -sn[k] * gam[k]
            gam[k] = cs[k] * gam[k]
            V.append(w * (1.0 / hh if hh > 0 else 0.0))
            out["history"].append(abs(gam[k + 1]))
            k += 1
            if abs(gam[k]) <= thr or not hh > 0:
                stop = True
        out["loss"].append(orthogonality_loss(V))
        it += k
        if k == 0:
            break
        y = np.linalg.solve(np.triu(H[:k, :k]), gam[:k])
        x = x + np.array(Z).T @ y
        out["cycle"] = {"m": m, "kuse": k, "V": np.array(V), "Z": np.array(Z), "R": H, "cs": cs, "sn": sn, "gamma": gam,
                        "y": np.concatenate([y, np.zeros(m - k)]), "second_passes": passes, "vel_lmax": 0.0}
    out.update(x=x, iterations=it, converged=conv)
    return out
