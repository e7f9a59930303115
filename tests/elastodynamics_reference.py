"""numpy / scipy restatement of the generalized-alpha marcher of ElastodynamicsSolver, written from the balance equation

    M a_{n+1-am} + C v_{n+1-af} + K u_{n+1-af} = s_f(t_n + (1 - af) dt) F,      C = eta_M M + eta_K K,

in the ACCELERATION form (the device solves for the displacement): with the Newmark predictors u~ = u_n + dt v_n + dt^2 (1/2 - beta) a_n,
v~ = v_n + dt (1 - gamma) a_n and u_{n+1} = u~ + beta dt^2 a_{n+1}, v_{n+1} = v~ + gamma dt a_{n+1} the unknown a_{n+1} solves

    [(1 - am) M + (1 - af) gamma dt C + (1 - af) beta dt^2 K] a_{n+1} = s_f F - am M a_n - C ((1 - af) v~ + af v_n) - K ((1 - af) u~ + af u_n).

Dirichlet dofs are partitioned off: there u_{n+1} = g s_g(t_{n+1}) is known, hence a_{n+1} = (u_{n+1} - u~) / (beta dt^2) and v_{n+1} from
the same update; the free block is solved by a sparse direct factorisation (one per step length).  The march starts from
M a_0 = s_f(t_0) F - C v_0 - K u_0 on the free dofs and a_0 = 0 on the Dirichlet dofs."""
import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla


def parameters(rho_inf):
    """(alpha_m, alpha_f, beta, gamma) from the high-frequency spectral radius"""
    am = (2.0 * rho_inf - 1.0) / (rho_inf + 1.0)
    af = rho_inf / (rho_inf + 1.0)
    return am, af, 0.25 * (1.0 - am + af) ** 2, 0.5 - am + af


def march(K, M, F, u0, v0, dts, par, eta_m=0.0, eta_k=0.0, sf=None, sf0=1.0, dofs=(), g=(), sg=None):
    """One dict {'u', 'v', 'a'} per time point (the start included).  K, M: dense or sparse, WITHOUT eliminated rows; par = (alpha_m,
    alpha_f, beta, gamma); sf[n]: the load factor of step n (at t_n + (1 - af) dt_n), sf0: the one at t_0; dofs, g: the Dirichlet dofs
    and values (a dof named twice takes the last value), sg[k]: their factor at time point k."""
    am, af, beta, gamma = par
    K, M = sp.csr_matrix(K), sp.csr_matrix(M)
    n = K.shape[0]
    C = eta_m * M + eta_k * K
    F = np.zeros(n) if F is None else np.asarray(F, dtype=np.float64)
    N = len(dts)
    sf = np.ones(N) if sf is None else np.asarray(sf, dtype=np.float64)
    sg = np.ones(N + 1) if sg is None else np.asarray(sg, dtype=np.float64)
    gfull = np.zeros(n)
    fixed = np.zeros(n, dtype=bool)
    for i, val in zip(np.asarray(dofs, dtype=np.int64), np.asarray(g, dtype=np.float64)):
        gfull[i] = val
        fixed[i] = True
    fr, fx = np.nonzero(~fixed)[0], np.nonzero(fixed)[0]
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    u[fx] = gfull[fx] * sg[0]
    a = np.zeros(n)
    r0 = sf0 * F - C @ v - K @ u
    if len(fr) and np.any(r0[fr]):
        a[fr] = spla.splu(sp.csc_matrix(M[fr][:, fr])).solve(r0[fr])
    out = [{'u': u.copy(), 'v': v.copy(), 'a': a.copy()}]
    factor = {}
    for k in range(N):
        dt = float(dts[k])
        if dt not in factor:
            A = (1.0 - am) * M + ((1.0 - af) * gamma * dt) * C + ((1.0 - af) * beta * dt * dt) * K
            factor[dt] = (A, spla.splu(sp.csc_matrix(A[fr][:, fr])) if len(fr) else None)
        A, lu = factor[dt]
        ut = u + dt * v + dt * dt * (0.5 - beta) * a
        vt = v + dt * (1.0 - gamma) * a
        r = sf[k] * F - am * (M @ a) - C @ ((1.0 - af) * vt + af * v) - K @ ((1.0 - af) * ut + af * u)
        an = np.zeros(n)
        an[fx] = (gfull[fx] * sg[k + 1] - ut[fx]) / (beta * dt * dt)
        if len(fr):
            an[fr] = lu.solve(r[fr] - (A[fr][:, fx] @ an[fx] if len(fx) else 0.0))
        u = ut + beta * dt * dt * an
        u[fx] = gfull[fx] * sg[k + 1]
        v = vt + gamma * dt * an
        a = an
        out.append({'u': u.copy(), 'v': v.copy(), 'a': a.copy()})
    return out


def energy(K, M, u, v):
    """(1/2 v^T M v, 1/2 u^T K u)"""
    return 0.5 * float(v @ (M @ v)), 0.5 * float(u @ (K @ u))


def discrete_frequency(omega, dt):
    """the frequency at which the trapezoidal rule (rho_inf = 1) marches an undamped mode of frequency omega"""
    return (2.0 / dt) * np.arctan(0.5 * omega * dt)
