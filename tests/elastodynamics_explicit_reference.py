"""numpy restatement of the explicit (central-difference, lumped-mass) marcher of ElastodynamicsSolver, written in the Newmark
(u, v, a) form with beta = 0 and gamma = 1/2 - algebraically the march of the device's leapfrog (u_n, w_n = v_{n-1/2}), not its code:

    u_{n+1} = u_n + dt v_n + dt^2/2 a_n,
    a_{n+1} = (s_f[n+1] F - K u_{n+1} - eta_M m (v_n + dt/2 a_n)) / (m (1 + eta_M dt/2)),
    v_{n+1} = v_n + dt/2 (a_n + a_{n+1}),

with the lumped mass m (a vector), C = eta_M diag(m) and a_0 = (s_f[0] F - K u_0) / m - eta_M v_0.  The two forms meet in
w_{n+1/2} = v_n + dt/2 a_n.  Dirichlet rows follow the rule of the scheme: u_{n+1} = g s_g[n+1]; the half-step velocity of such a
row is (u_{n+1} - u_n) / dt, its full-step velocity is the half-step velocity BEHIND it, v_{n+1} = (u_{n+1} - u_n) / dt, and its
acceleration is 0 (at the start such a row keeps the v_0 it was given and a_0 = 0).

march_leapfrog is the same march in the device's own variables; the host tests hold the two together."""
import numpy as np
import scipy.sparse as sp


def _dirichlet(n, dofs, g):
    gfull, fixed = np.zeros(n), np.zeros(n, dtype=bool)
    for i, val in zip(np.asarray(dofs, dtype=np.int64), np.asarray(g, dtype=np.float64)):
        gfull[i], fixed[i] = val, True             # a dof named twice takes the last value
    return gfull, fixed


def march(K, m, F, u0, v0, dt, steps, eta_m=0.0, sf=None, dofs=(), g=(), sg=None):
    """One dict {'u', 'v', 'a'} per time point (the start included).  K: dense or sparse, WITHOUT eliminated rows; m: the lumped mass;
    sf[k], sg[k]: the load and Dirichlet factors at time point k (steps + 1 values each)."""
    K = sp.csr_matrix(K)
    n = K.shape[0]
    m = np.asarray(m, dtype=np.float64)
    F = np.zeros(n) if F is None else np.asarray(F, dtype=np.float64)
    sf = np.ones(steps + 1) if sf is None else np.asarray(sf, dtype=np.float64)
    sg = np.ones(steps + 1) if sg is None else np.asarray(sg, dtype=np.float64)
    gfull, fixed = _dirichlet(n, dofs, g)
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    u[fixed] = gfull[fixed] * sg[0]
    a = (sf[0] * F - K @ u) / m - eta_m * v
    a[fixed] = 0.0
    out = [{'u': u.copy(), 'v': v.copy(), 'a': a.copy()}]
    for k in range(steps):
        un = u + dt * v + (0.5 * dt * dt) * a
        un[fixed] = gfull[fixed] * sg[k + 1]
        an = (sf[k + 1] * F - K @ un - eta_m * m * (v + (0.5 * dt) * a)) / (m * (1.0 + 0.5 * eta_m * dt))
        vn = v + (0.5 * dt) * (a + an)
        vn[fixed] = (un[fixed] - u[fixed]) / dt
        an[fixed] = 0.0
        u, v, a = un, vn, an
        out.append({'u': u.copy(), 'v': v.copy(), 'a': a.copy()})
    return out


def march_leapfrog(K, m, F, u0, v0, dt, steps, eta_m=0.0, sf=None, dofs=(), g=(), sg=None):
    """The same march in the variables of the device: one dict {'u': u_n, 'w': w_n = v_{n-1/2}, 'y': K u_{n-1}} per time point n >= 1,
    and at index 0 {'u': u_0, 'w': None, 'y': None}."""
    K = sp.csr_matrix(K)
    n = K.shape[0]
    m = np.asarray(m, dtype=np.float64)
    F = np.zeros(n) if F is None else np.asarray(F, dtype=np.float64)
    sf = np.ones(steps + 1) if sf is None else np.asarray(sf, dtype=np.float64)
    sg = np.ones(steps + 1) if sg is None else np.asarray(sg, dtype=np.float64)
    gfull, fixed = _dirichlet(n, dofs, g)
    alpha = 0.5 * eta_m * dt
    u = np.array(u0, dtype=np.float64)
    u[fixed] = gfull[fixed] * sg[0]
    out = [{'u': u.copy(), 'w': None, 'y': None}]
    w = None
    for k in range(steps):
        y = K @ u
        if k == 0:
            v0 = np.asarray(v0, dtype=np.float64)
            wn = v0 + (0.5 * dt) * ((sf[0] * F - y) / m - eta_m * v0)
        else:
            wn = ((1.0 - alpha) * w + dt * (sf[k] * F - y) / m) / (1.0 + alpha)
        un = u + dt * wn
        un[fixed] = gfull[fixed] * sg[k + 1]
        wn[fixed] = (un[fixed] - u[fixed]) / dt
        u, w = un, wn
        out.append({'u': u.copy(), 'w': w.copy(), 'y': y})
    return out


def full_step(K, m, F, u, w, dt, eta_m, sf_n, fixed=None):
    """(v_n, a_n) of the leapfrog state (u_n, w_n = v_{n-1/2}): w+ is the recurrence's w_{n+1/2}; Dirichlet rows: v = w, a = 0"""
    alpha = 0.5 * eta_m * dt
    F = np.zeros(len(u)) if F is None else F
    wp = ((1.0 - alpha) * w + dt * (sf_n * F - sp.csr_matrix(K) @ u) / m) / (1.0 + alpha)
    v, a = 0.5 * (w + wp), (wp - w) / dt
    if fixed is not None:
        v[fixed], a[fixed] = w[fixed], 0.0
    return v, a


def step_energy(m, w_half, u_next, y):
    """(E_kin, E_pot) of the step n -> n+1: 1/2 sum m w_{n+1/2}^2, 1/2 u_{n+1}^T K u_n with y = K u_n"""
    return 0.5 * float(np.sum(m * w_half * w_half)), 0.5 * float(u_next @ y)


def discrete_frequency(omega, dt):
    """the frequency at which central differences march an undamped mode of frequency omega: sin(omega_h dt / 2) = omega dt / 2"""
    return (2.0 / dt) * np.arcsin(0.5 * omega * dt)
