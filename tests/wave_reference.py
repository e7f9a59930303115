"""numpy / scipy restatement of the explicit scalar wave model of WaveSolver (include/fenicssolver_amd.h, the fs_wave_* block): assembly
of K, m, d and F on a given simplex mesh, the start, the marcher, the discrete energy and the Gershgorin step bound.  It shares no
code with the package: meshes come in as plain arrays.

Model: u_tt = div(c^2 grad u) + f on scalar P1.  K the stiffness with c^2 per cell, m_i = int phi_i dx, d_i = sum over the absorbing
facets F around i of c(cell of F) |F| / dim, F the load (body source + flux facets + point loads), f^n = s_f[n] F, Dirichlet dofs take
g s_g[n].  Step n -> n+1 (n >= 1), y = K u^n:
    (m/dt^2 + d/(2 dt)) u^{n+1} = s_f[n] F - y + (2 m/dt^2) u^n - (m/dt^2 - d/(2 dt)) u^{n-1},
start a^0 = (s_f[0] F - K u^0 - d v^0) / m, u^1 = u^0 + dt v^0 + dt^2/2 a^0; Dirichlet dofs overwritten after either.
Energy of step n -> n+1: (1/2 sum m ((u^{n+1} - u^n)/dt)^2, 1/2 (u^{n+1})^T y).
"""
import math

import numpy as np
import scipy.sparse as sp


# ---------------------------------------------------------------------------------------------------------------- geometry
def _gradients(coords, cells):
    """(grad lambda_a [nc, d+1, d], cell measure [nc])"""
    X = coords[cells]
    d = coords.shape[1]
    J = np.stack([X[:, k + 1] - X[:, 0] for k in range(d)], axis=2)
    Ji = np.linalg.inv(J)
    g = np.concatenate([-Ji.sum(axis=1, keepdims=True), Ji], axis=1)
    return g, np.abs(np.linalg.det(J)) / math.factorial(d)


def facet_measure(coords, facets):
    X = coords[facets]
    if coords.shape[1] == 2:
        return np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
    return 0.5 * np.linalg.norm(np.cross(X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]), axis=1)


def boundary_facets(cells):
    """(facets [nf, d] sorted vertex tuples, cell of each) of the facets that belong to one cell only"""
    nl = cells.shape[1]
    fl, cl = [], []
    for k in range(nl):
        fl.append(np.sort(np.delete(cells, k, axis=1), axis=1))
        cl.append(np.arange(len(cells)))
    f, c = np.concatenate(fl), np.concatenate(cl)
    uniq, inv, cnt = np.unique(f, axis=0, return_inverse=True, return_counts=True)
    keep = cnt[inv.ravel()] == 1
    return f[keep], c[keep]


# ---------------------------------------------------------------------------------------------------------------- assembly
def stiffness(coords, cells, c_cell):
    """K_ij = sum_cells c^2 |cell| grad lambda_i . grad lambda_j (csr)"""
    g, vol = _gradients(coords, cells)
    c2 = np.broadcast_to(np.asarray(c_cell, dtype=np.float64), (len(cells),)) ** 2
    ke = (c2 * vol)[:, None, None] * np.einsum("cad,cbd->cab", g, g)
    nl = cells.shape[1]
    rows, cols = np.repeat(cells, nl, axis=1).ravel(), np.tile(cells, (1, nl)).ravel()
    n = coords.shape[0]
    return sp.coo_matrix((ke.ravel(), (rows, cols)), shape=(n, n)).tocsr()


def lumped_mass(coords, cells):
    _, vol = _gradients(coords, cells)
    m = np.zeros(coords.shape[0])
    np.add.at(m, cells.ravel(), np.repeat(vol / cells.shape[1], cells.shape[1]))
    return m


def facet_vector(coords, facets, g):
    """b_i = int g phi_i ds over the facets, g one number per facet (or one number)"""
    d = coords.shape[1]
    w = facet_measure(coords, facets) * np.broadcast_to(np.asarray(g, dtype=np.float64), (len(facets),)) / d
    b = np.zeros(coords.shape[0])
    np.add.at(b, facets.ravel(), np.repeat(w, facets.shape[1]))
    return b


def damping(coords, facets, facet_cells, c_cell):
    """d_i = sum_F c(cell of F) |F| / dim over the absorbing facets"""
    c = np.broadcast_to(np.asarray(c_cell, dtype=np.float64), (int(np.max(facet_cells)) + 1 if np.ndim(c_cell) == 0 else len(c_cell),))
    return facet_vector(coords, facets, c[facet_cells])


def body_load(coords, cells, f):
    """int f phi_i dx: f a number, or nodal values (its P1 interpolant, integrated exactly)"""
    if np.ndim(f) == 0:
        return float(f) * lumped_mass(coords, cells)
    _, vol = _gradients(coords, cells)
    nl = cells.shape[1]
    me = (np.ones((nl, nl)) + np.eye(nl)) / (nl * (nl + 1.0))          # consistent P1 mass of a cell of unit measure
    b = np.zeros(coords.shape[0])
    np.add.at(b, cells.ravel(), (vol[:, None] * (np.asarray(f, dtype=np.float64)[cells] @ me)).ravel())
    return b


def point_load(coords, cells, point, magnitude):
    """magnitude * phi_i(point) on the cell that holds the point: (dofs, weights)"""
    d = coords.shape[1]
    X = coords[cells]
    T = np.stack([X[:, k + 1] - X[:, 0] for k in range(d)], axis=2)
    lam = np.linalg.solve(T, (np.asarray(point, dtype=np.float64)[:d] - X[:, 0])[:, :, None])[:, :, 0]
    bary = np.concatenate([1.0 - lam.sum(axis=1, keepdims=True), lam], axis=1)
    i = int(np.argmax(bary.min(axis=1)))
    return cells[i], magnitude * bary[i]


def gershgorin(K, m):
    """lambda_G = max_i sum_j |K_ij| / m_i >= lambda_max(M_L^-1 K)"""
    return float(np.max(np.asarray(abs(K).sum(axis=1)).ravel() / m))


def critical_time_step(K, m):
    return 2.0 / math.sqrt(gershgorin(K, m))


def lambda_max(K, m):
    """the true largest eigenvalue of M_L^-1 K (dense: small meshes only)"""
    s = 1.0 / np.sqrt(m)
    return float(np.linalg.eigvalsh(s[:, None] * K.toarray() * s[None, :])[-1])


# ---------------------------------------------------------------------------------------------------------------- the marcher
def ricker(t, frequency, delay):
    a = (math.pi * frequency * (np.asarray(t, dtype=np.float64) - delay)) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def start(K, m, d, F, dt, u0, v0, sf0, sg1, bc_dofs=None, bc_vals=None):
    a0 = (sf0 * F - K @ u0 - d * v0) / m
    u1 = u0 + dt * v0 + 0.5 * dt * dt * a0
    if bc_dofs is not None and len(bc_dofs):
        u1[bc_dofs] = np.asarray(bc_vals) * sg1
    return u1


def step(K, m, d, F, dt, up, u, sf, sg, bc_dofs=None, bc_vals=None):
    """(u^{n+1}, (E_kin, E_pot)) from (u^{n-1}, u^n) with s_f[n] and s_g[n+1]"""
    y = K @ u
    a, b = m / dt ** 2, d / (2.0 * dt)
    un = (sf * F - y + 2.0 * a * u - (a - b) * up) / (a + b)
    if bc_dofs is not None and len(bc_dofs):
        un[bc_dofs] = np.asarray(bc_vals) * sg
    return un, energy(K, m, dt, u, un, y)


def energy(K, m, dt, u, un, y=None):
    y = K @ u if y is None else y
    return 0.5 * float(np.sum(m * ((un - u) / dt) ** 2)), 0.5 * float(un @ y)


def march(K, m, d, F, dt, u0, v0, n_steps, sf=None, sg=None, bc_dofs=None, bc_vals=None, receivers=None):
    """n_steps steps from (u^0, v^0): the start, then n_steps - 1 updates.  sf[n], n < n_steps, and sg[n], n <= n_steps (None: 1).
    Returns {'u': u^N, 'u_prev': u^{N-1}, 'traces' [n_steps + 1, n_receivers], 'energy' [n_steps, 2]} (energy[n]: step n -> n+1)."""
    sf = np.ones(n_steps) if sf is None else np.asarray(sf, dtype=np.float64)
    sg = np.ones(n_steps + 1) if sg is None else np.asarray(sg, dtype=np.float64)
    rec = np.zeros(0, dtype=np.int64) if receivers is None else np.asarray(receivers, dtype=np.int64)
    tr, en = np.zeros((n_steps + 1, len(rec))), np.zeros((n_steps, 2))
    up = np.array(u0, dtype=np.float64)
    tr[0] = up[rec]
    u = start(K, m, d, F, dt, up, np.asarray(v0, dtype=np.float64), sf[0], sg[1], bc_dofs, bc_vals)
    en[0] = energy(K, m, dt, up, u)
    tr[1] = u[rec]
    for n in range(1, n_steps):
        un, en[n] = step(K, m, d, F, dt, up, u, sf[n], sg[n + 1], bc_dofs, bc_vals)
        up, u = u, un
        tr[n + 1] = u[rec]
    return {"u": u, "u_prev": up, "traces": tr, "energy": en}


# ---------------------------------------------------------------------------------------------------------------- the standing wave
def unit_square(n):
    """right-diagonal triangles of the unit square, vertices x fastest: (coords, cells)"""
    x = np.arange(n + 1) / float(n)
    coords = np.stack([np.tile(x, n + 1), np.repeat(x, n + 1)], axis=1)
    ix, iy = np.meshgrid(np.arange(n), np.arange(n), indexing="xy")
    v0 = (iy * (n + 1) + ix).ravel()
    v1, v2 = v0 + 1, v0 + n + 1
    v3 = v2 + 1
    cells = np.stack([np.stack([v0, v1, v3], axis=1), np.stack([v0, v2, v3], axis=1)], axis=1).reshape(-1, 3)
    return coords, cells


def standing_wave(n, safety=0.5, T=1.0):
    """sin(pi x) sin(pi y) cos(sqrt 2 pi t) on the unit square, homogeneous Dirichlet, to t = T at `safety` times the Gershgorin step
    rounded down so that T is a whole number of steps.  Returns (max error at T, energy [N, 2], dt, N, lambda_G, u^N)."""
    coords, cells = unit_square(n)
    K, m = stiffness(coords, cells, 1.0), lumped_mass(coords, cells)
    lam = gershgorin(K, m)
    N = int(math.ceil(T / (safety * 2.0 / math.sqrt(lam))))
    dt = T / N
    x, y = coords[:, 0], coords[:, 1]
    on = (x == 0) | (x == 1) | (y == 0) | (y == 1)
    bc = np.nonzero(on)[0]
    u0 = np.sin(math.pi * x) * np.sin(math.pi * y)
    u0[bc] = 0.0
    z = np.zeros_like(u0)
    r = march(K, m, z, z, dt, u0, z, N, bc_dofs=bc, bc_vals=np.zeros(len(bc)))
    exact = np.sin(math.pi * x) * np.sin(math.pi * y) * math.cos(math.sqrt(2.0) * math.pi * T)
    return float(np.abs(r["u"] - exact).max()), r["energy"], dt, N, lam, r["u"]
