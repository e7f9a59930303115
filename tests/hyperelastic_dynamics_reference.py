"""numpy fp64 restatement of the explicit finite-strain marcher of HyperelasticDynamicsSolver: central differences with a lumped mass
and the internal force of a hyperelastic energy, written in the Newmark (u, v, a) form with beta = 0 and gamma = 1/2 -
algebraically the march of the device's leapfrog (u_n, w_n = v_{n-1/2}), not its code:

    u_{n+1} = u_n + dt v_n + dt^2/2 a_n,
    a_{n+1} = (s_f[n+1] F - f_int(u_{n+1}) - eta_M m (v_n + dt/2 a_n)) / (m (1 + eta_M dt/2)),
    v_{n+1} = v_n + dt/2 (a_n + a_{n+1}),

with a_0 = (s_f[0] F - f_int(u_0)) / m - eta_M v_0; the two forms meet in w_{n+1/2} = v_n + dt/2 a_n.  Dirichlet rows as in
elastodynamics_explicit_reference.py: u_{n+1} = g s_g[n+1], v_{n+1} = (u_{n+1} - u_n) / dt, a = 0.

Forces and energy are those of hyperelastic_models_reference.py (first_pk, psi; 'neo_hookean' included, with F embedded in 3 x 3 in
plane strain so that psi = 0 at rest): f_a = V P g_a summed over the cells, Pi = sum V psi.  `Body.force_energy` evaluates them for all
cells at once with the same tensor formulas (S, E, F^-T - not the invariant-derivative contraction of the device);
`Body.force_energy_by_cell` is the cell-by-cell sum through first_pk and psi themselves, and tests/test_hyperelastic_dynamics_host.py
holds the two together.  The lumped mass is the row sum of the P1 mass: rho V / (d + 1) per cell and vertex."""
import numpy as np

import hyperelastic_models_reference as mr

MODELS = ("neo_hookean",) + mr.MODELS


class Body:
    """a P1 mesh with one parameter row per cell: coords [n_nodes, >= d], cells [n_cells, d + 1], params one row p[4] or [n_cells, 4]"""

    def __init__(self, coords, cells, model, params):
        self.cells = np.asarray(cells, dtype=np.int64)
        nc, nv = self.cells.shape
        self.d = d = nv - 1
        self.X = np.asarray(coords, dtype=np.float64)[:, :d]
        self.n = self.X.shape[0] * d
        self.model = model
        self.p = np.broadcast_to(np.asarray(params, dtype=np.float64), (nc, 4))
        Xc = self.X[self.cells]
        E = np.swapaxes(Xc[:, 1:] - Xc[:, :1], 1, 2)                       # columns: edge vectors
        Ei = np.linalg.inv(E)
        self.g = np.concatenate([-Ei.sum(axis=1, keepdims=True), Ei], axis=1)      # [nc, d + 1, d]
        self.vol = np.abs(np.linalg.det(E)) / (6.0 if d == 3 else 2.0)
        self.dofs = (self.cells[:, :, None] * d + np.arange(d)[None, None, :]).reshape(nc, -1)

    def lumped_mass(self, rho):
        rho = np.broadcast_to(np.asarray(rho, dtype=np.float64), self.vol.shape)
        share = np.repeat((rho * self.vol / (self.d + 1))[:, None], (self.d + 1) * self.d, axis=1)
        return np.bincount(self.dofs.ravel(), weights=share.ravel(), minlength=self.n)

    def deformation_gradients(self, u):
        U = np.asarray(u, dtype=np.float64).reshape(-1, self.d)[self.cells]          # [nc, d + 1, d]
        return np.eye(self.d)[None] + np.einsum("cai,caj->cij", U, self.g)

    def force_energy(self, u):
        """(f_int [n], Pi, J [n_cells]) with every cell at once"""
        d, p, model = self.d, self.p, self.model
        Fd = self.deformation_gradients(u)
        nc = len(Fd)
        F = np.zeros((nc, 3, 3))
        F[:, :d, :d] = Fd
        if d == 2:
            F[:, 2, 2] = 1.0
        I3 = np.eye(3)[None]
        with np.errstate(all="ignore"):                                    # (a march that blows up is marched to its end)
            J = np.linalg.det(F)
            C = np.einsum("cki,ckj->cij", F, F)
            I1 = np.trace(C, axis1=1, axis2=2)
            cof = np.stack([np.cross(F[:, 1], F[:, 2]), np.cross(F[:, 2], F[:, 0]), np.cross(F[:, 0], F[:, 1])], axis=1)
            Fit = cof / J[:, None, None]                                   # F^-T (no exception on an inverted or non-finite cell)
            c0, c1, c2, c3 = (p[:, k] for k in range(4))
            if model == "st_venant_kirchhoff":
                E = 0.5 * (C - I3)
                trE = np.trace(E, axis1=1, axis2=2)
                P = F @ (c1[:, None, None] * trE[:, None, None] * I3 + 2.0 * c0[:, None, None] * E)
                psi = 0.5 * c1 * trE ** 2 + c0 * np.sum(E * E, axis=(1, 2))
            elif model == "neo_hookean":
                lj = np.log(J)
                P = c0[:, None, None] * (F - Fit) + (c1 * lj)[:, None, None] * Fit
                psi = 0.5 * c0 * (I1 - 3.0) - c0 * lj + 0.5 * c1 * lj * lj
            else:
                a, b = np.cbrt(J) ** -2, np.cbrt(J) ** -4
                I2 = 0.5 * (I1 * I1 - np.trace(C @ C, axis1=1, axis2=2))
                D1 = a[:, None, None] * (2.0 * F - (2.0 / 3.0) * I1[:, None, None] * Fit)
                volP = ((J - 1.0) * J)[:, None, None] * Fit
                if model == "mooney_rivlin":
                    G2 = 2.0 * (I1[:, None, None] * F - F @ C)
                    D2 = b[:, None, None] * (G2 - (4.0 / 3.0) * I2[:, None, None] * Fit)
                    P = c0[:, None, None] * D1 + c1[:, None, None] * D2 + c2[:, None, None] * volP
                    psi = c0 * (a * I1 - 3.0) + c1 * (b * I2 - 3.0) + 0.5 * c2 * (J - 1.0) ** 2
                elif model == "yeoh":
                    x = a * I1 - 3.0
                    P = (c0 + 2.0 * c1 * x + 3.0 * c2 * x ** 2)[:, None, None] * D1 + c3[:, None, None] * volP
                    psi = c0 * x + c1 * x ** 2 + c2 * x ** 3 + 0.5 * c3 * (J - 1.0) ** 2
                else:
                    raise ValueError(model)
        fe = self.vol[:, None, None] * np.einsum("caj,cij->cai", self.g, P[:, :d, :d])
        f = np.bincount(self.dofs.ravel(), weights=fe.reshape(nc, -1).ravel(), minlength=self.n)
        return f, float(np.sum(self.vol * psi)), J

    def force_energy_by_cell(self, u):
        """the same through first_pk and psi of hyperelastic_models_reference.py, one cell at a time"""
        Fd = self.deformation_gradients(u)
        f, energy = np.zeros(self.n), 0.0
        for c in range(len(Fd)):
            P = mr.first_pk(self.model, self.p[c], Fd[c])
            np.add.at(f, self.dofs[c], (self.vol[c] * self.g[c] @ P.T).ravel())
            energy += self.vol[c] * mr.psi(self.model, self.p[c], Fd[c])
        return f, float(energy), np.linalg.det(Fd)


def _dirichlet(n, dofs, g):
    gfull, fixed = np.zeros(n), np.zeros(n, dtype=bool)
    for i, val in zip(np.asarray(dofs, dtype=np.int64), np.asarray(g, dtype=np.float64)):
        gfull[i], fixed[i] = val, True             # a dof named twice takes the last value
    return gfull, fixed


def march(body, m, F, u0, v0, dt, steps, eta_m=0.0, sf=None, dofs=(), g=(), sg=None):
    """One dict per time point n = 0 .. steps: 'u', 'v', 'a' (full-step values), 'pi' = Pi(u_n), 'min_J', and 'w' = w_{n-1/2}, the
    half-step velocity behind the point (None at n = 0).  m: the lumped mass; sf[k], sg[k]: the load and Dirichlet factors at time
    point k (steps + 1 values each).  A point with min_J <= 0 holds an inverted cell: the device reports the step that starts there."""
    n = body.n
    m = np.asarray(m, dtype=np.float64)
    F = np.zeros(n) if F is None else np.asarray(F, dtype=np.float64)
    sf = np.ones(steps + 1) if sf is None else np.asarray(sf, dtype=np.float64)
    sg = np.ones(steps + 1) if sg is None else np.asarray(sg, dtype=np.float64)
    gfull, fixed = _dirichlet(n, dofs, g)
    u, v = np.array(u0, dtype=np.float64), np.array(v0, dtype=np.float64)
    u[fixed] = gfull[fixed] * sg[0]
    fi, pi, J = body.force_energy(u)
    a = (sf[0] * F - fi) / m - eta_m * v
    a[fixed] = 0.0
    out = [{'u': u.copy(), 'v': v.copy(), 'a': a.copy(), 'w': None, 'pi': pi, 'min_J': float(J.min())}]
    for k in range(steps):
        wh = v + (0.5 * dt) * a
        un = u + dt * v + (0.5 * dt * dt) * a
        un[fixed] = gfull[fixed] * sg[k + 1]
        wh[fixed] = (un[fixed] - u[fixed]) / dt
        fi, pi, J = body.force_energy(un)
        with np.errstate(all="ignore"):
            an = (sf[k + 1] * F - fi - eta_m * m * (v + (0.5 * dt) * a)) / (m * (1.0 + 0.5 * eta_m * dt))
            vn = v + (0.5 * dt) * (a + an)
        vn[fixed] = wh[fixed]
        an[fixed] = 0.0
        u, v, a = un, vn, an
        out.append({'u': u.copy(), 'v': v.copy(), 'a': a.copy(), 'w': wh, 'pi': pi, 'min_J': float(J.min())})
    return out


def step_energies(m, ref):
    """[steps, 2]: (E_kin(w_{n+1/2}), Pi(u_n)) of the step n -> n+1, n = 0 .. steps - 1, as the device reports them"""
    return np.array([[0.5 * float(np.sum(m * ref[k + 1]['w'] ** 2)), ref[k]['pi']] for k in range(len(ref) - 1)])


def half_step_energy(en, pi_last=None):
    """E_{n+1/2} = E_kin(w_{n+1/2}) + (Pi(u_n) + Pi(u_{n+1})) / 2 from rows (E_kin, Pi(u_n)) of consecutive steps: one value fewer
    than rows, unless pi_last = Pi of the point behind the last step closes the last one"""
    en = np.asarray(en, dtype=np.float64)
    pi = en[:, 1] if pi_last is None else np.append(en[:, 1], pi_last)
    k = len(pi) - 1
    return en[:k, 0] + 0.5 * (pi[:k] + pi[1:k + 1])


def first_inverted_step(ref):
    """the n of the first time point whose state holds an inverted (or non-finite) cell; None: none"""
    for k, s in enumerate(ref):
        if not (s['min_J'] > 0.0 and np.isfinite(s['min_J'])):
            return k
    return None


def rigid_motion(X, axis, angle, shift):
    """u = (R - I) X + c for the rotation about `axis` (3-D; 2-D: about z) by `angle`"""
    d = X.shape[1]
    if d == 2:
        R = np.array([[np.cos(angle), -np.sin(angle)], [np.sin(angle), np.cos(angle)]])
    else:
        k = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
        Kx = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
        R = np.eye(3) + np.sin(angle) * Kx + (1.0 - np.cos(angle)) * Kx @ Kx
    return (X @ (R - np.eye(d)).T + np.asarray(shift, dtype=np.float64)[None, :d]).ravel()
