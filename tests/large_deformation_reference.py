"""Host restatement of LargeDeformationSolver's forms (FenicsSolver/LargeDeformationSolver.py:80-135) on P1 cells, in numpy.

Unknowns per vertex: (u, v, p) - 2d + 1 values, dof = vertex * (2d + 1) + component.  With F = I + grad u, J = det F,
S = J (-p I + mu (F F^T - I)) F^-T and pp = p / lambda + J^2 - 1:
    R_u = (1/dt) <u - u0, _u> - q <v, _u> - (1-q) <v0, _u>
    R_v = (1/dt) <v - v0, _v> + q <S, grad _v> + (1-q) <S0, grad _v> + <J F^-T g, _v>_ds + <f, _v>
    R_p = q <pp, _p> + (1-q) <pp0, _p>
Every integrand is a polynomial of degree <= 2 on a P1 cell, integrated here in closed form (the reference's degree-4 rule is
exact for them).  The Jacobian is the analytic derivative; tests compare it with central differences of the residual.
``newton`` is the monolithic Newton of solve(F == 0, w, bcs, J) with scipy's spsolve standing in for MUMPS and the stopping test
of DOLFIN's NewtonSolver (||R|| with Dirichlet rows zeroed, absolute 1e-9 / relative 1e-7, 50 iterations).
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sps
import scipy.sparse.linalg as spla


def geometry(co, cells):
    """(g [nc, d+1, d] gradients of the barycentric functions, vol [nc])."""
    X = co[cells]
    d = co.shape[1]
    E = X[:, 1:, :] - X[:, :1, :]                      # rows = edge vectors
    Ginv = np.linalg.inv(E)                            # grad lambda_i = column i of E^-1
    g = np.empty((len(cells), d + 1, d))
    g[:, 1:, :] = np.transpose(Ginv, (0, 2, 1))
    g[:, 0, :] = -g[:, 1:, :].sum(axis=1)
    vol = np.abs(np.linalg.det(E)) / (2.0 if d == 2 else 6.0)
    return g, vol


def kinematics(u, cells, g):
    """F, F^-T, J per cell for the nodal displacement u [nv, d]."""
    d = g.shape[2]
    F = np.eye(d)[None] + np.einsum('cai,caj->cij', u[cells], g)
    J = np.linalg.det(F)
    FiT = np.transpose(np.linalg.inv(F), (0, 2, 1))
    return F, FiT, J


class Problem:
    def __init__(self, co, cells, dt, q, mu, lmbda, body=None, facets=()):
        """facets: iterable of (cell, local vertex opposite the facet, g[d])."""
        self.co = np.asarray(co, dtype=np.float64)
        self.cells = np.asarray(cells, dtype=np.int64)
        self.d = self.co.shape[1]
        self.nv = len(self.co)
        self.nb = 2 * self.d + 1
        self.dt, self.q, self.mu, self.lmbda = float(dt), float(q), float(mu), float(lmbda)
        self.body = np.zeros(self.d) if body is None else np.asarray(body, dtype=np.float64)
        self.g, self.vol = geometry(self.co, self.cells)
        fl = list(facets)
        self.fcell = np.array([f[0] for f in fl], dtype=np.int64)
        self.fopp = np.array([f[1] for f in fl], dtype=np.int64)
        self.fg = np.array([np.asarray(f[2], dtype=np.float64) for f in fl]).reshape(len(fl), self.d)
        if len(fl):
            keep = np.ones((len(fl), self.d + 1), dtype=bool)
            keep[np.arange(len(fl)), self.fopp] = False
            self.flocal = np.nonzero(keep)[1].reshape(len(fl), self.d)          # facet vertices, ascending local index
            P = self.co[self.cells[self.fcell[:, None], self.flocal]]
            if self.d == 2:
                self.farea = np.linalg.norm(P[:, 1] - P[:, 0], axis=1)
            else:
                self.farea = 0.5 * np.linalg.norm(np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0]), axis=1)

    # ---- layout
    def split(self, x):
        a = np.asarray(x).reshape(self.nv, self.nb)
        return a[:, :self.d], a[:, self.d:2 * self.d], a[:, 2 * self.d]

    def join(self, u, v, p):
        return np.concatenate([u, v, p[:, None]], axis=1).reshape(-1)

    def dof(self, node, field, comp=0):
        off = {'u': 0, 'v': self.d, 'p': 2 * self.d}[field]
        return np.asarray(node) * self.nb + off + comp

    # ---- residual
    def _mass(self):
        d = self.d
        return self.vol[:, None, None] * (1.0 + np.eye(d + 1))[None] / ((d + 1) * (d + 2))

    def residual(self, x, x0):
        d, q, dt, mu = self.d, self.q, self.dt, self.mu
        u, v, p = self.split(x)
        u0, v0, p0 = self.split(x0)
        cells, g, vol = self.cells, self.g, self.vol
        M = self._mass()
        R = np.zeros((self.nv, self.nb))
        ru = (u - u0) / dt - q * v - (1.0 - q) * v0
        np.add.at(R[:, :d], cells, np.einsum('cab,cbi->cai', M, ru[cells]))
        np.add.at(R[:, d:2 * d], cells, np.einsum('cab,cbi->cai', M, (v - v0)[cells] / dt))
        pq = (q * p + (1.0 - q) * p0) / self.lmbda
        np.add.at(R[:, 2 * d], cells, np.einsum('cab,cb->ca', M, pq[cells]))
        for w, uu, pp in ((q, u, p), (1.0 - q, u0, p0)):
            F, FiT, J = kinematics(uu, cells, g)
            pm = pp[cells].mean(axis=1)
            S = mu * J[:, None, None] * F - ((pm + mu) * J)[:, None, None] * FiT
            f = vol[:, None, None] * np.einsum('cij,caj->cai', S, g)
            np.add.at(R[:, d:2 * d], cells, w * f)
            np.add.at(R[:, 2 * d], cells, np.repeat((w * vol * (J * J - 1.0) / (d + 1))[:, None], d + 1, axis=1))
        np.add.at(R[:, d:2 * d], cells, np.broadcast_to((vol / (d + 1))[:, None, None] * self.body[None, None, :], (len(cells), d + 1, d)))
        if len(self.fcell):
            F, FiT, J = kinematics(u, cells[self.fcell], g[self.fcell])
            h = (self.farea / d * J)[:, None] * np.einsum('fij,fj->fi', FiT, self.fg)
            nodes = cells[self.fcell[:, None], self.flocal]
            np.add.at(R[:, d:2 * d], nodes, np.repeat(h[:, None, :], d, axis=1))
        return R.reshape(-1)

    # ---- Jacobian
    def jacobian(self, x):
        d, q, dt, mu = self.d, self.q, self.dt, self.mu
        nb = self.nb
        u, v, p = self.split(x)
        cells, g, vol = self.cells, self.g, self.vol
        nc = len(cells)
        M = self._mass()
        F, FiT, J = kinematics(u, cells, g)
        pm = p[cells].mean(axis=1)
        G = np.einsum('cij,caj->cai', FiT, g)               # G_a = F^-T g_a
        Fg = np.einsum('cij,caj->cai', F, g)
        gg = np.einsum('cai,cbi->cab', g, g)
        I = np.eye(d)
        # Kt[c, a, b, i, k] = d (V S g_a)_i / d u_bk
        Kt = vol[:, None, None, None, None] * (
            mu * J[:, None, None, None, None] * (np.einsum('cbk,cai->cabik', G, Fg) + gg[:, :, :, None, None] * I[None, None, None])
            - ((pm + mu) * J)[:, None, None, None, None] * (np.einsum('cbk,cai->cabik', G, G) - np.einsum('cbi,cak->cabik', G, G)))
        E = np.zeros((nc, d + 1, nb, d + 1, nb))
        eye = np.eye(d)
        ui, vi, pi = slice(0, d), slice(d, 2 * d), 2 * d
        E[:, :, ui, :, ui] = (M / dt)[:, :, None, :, None] * eye[None, None, :, None, :]
        E[:, :, ui, :, vi] = (-q * M)[:, :, None, :, None] * eye[None, None, :, None, :]
        E[:, :, vi, :, vi] = (M / dt)[:, :, None, :, None] * eye[None, None, :, None, :]
        E[:, :, vi, :, ui] = q * np.transpose(Kt, (0, 1, 3, 2, 4))
        ic = vol / (d + 1)
        # J_vp[a, b][i] = -q J G_a[i] V/(d+1)   (S linear in p; int phi_b = V/(d+1))
        E[:, :, vi, :, pi] = (-q * (J * ic)[:, None, None] * G)[:, :, :, None]
        # J_pu[a, (b, k)] = q 2 J^2 G_b[k] V/(d+1)
        E[:, :, pi, :, ui] = np.broadcast_to((2.0 * q * (J * J * ic)[:, None, None] * G)[:, None, :, :], (nc, d + 1, d + 1, d))
        E[:, :, pi, :, pi] = q / self.lmbda * M
        rows = (cells[:, :, None] * nb + np.arange(nb)[None, None, :])           # [nc, d+1, nb]
        R_ = np.broadcast_to(rows[:, :, :, None, None], E.shape)
        C_ = np.broadcast_to(rows[:, None, None, :, :], E.shape)
        A = sps.coo_matrix((E.ravel(), (R_.ravel(), C_.ravel())), shape=(self.nv * nb,) * 2)
        if len(self.fcell):
            Ff, FiTf, Jf = kinematics(u, cells[self.fcell], g[self.fcell])
            h = np.einsum('fij,fj->fi', FiTf, self.fg)
            Gf = np.einsum('fij,fbj->fbi', FiTf, g[self.fcell])
            w = self.farea / d * Jf
            # d (w J F^-T g)_i / d u_bk = w J (G_b[k] h_i - G_b[i] h_k)
            K = w[:, None, None, None] * (np.einsum('fbk,fi->fbik', Gf, h) - np.einsum('fbi,fk->fbik', Gf, h))
            nf = len(self.fcell)
            anodes = cells[self.fcell[:, None], self.flocal]                    # [nf, d]
            bnodes = cells[self.fcell]                                           # [nf, d+1]
            r = np.broadcast_to((anodes[:, :, None, None, None] * nb + d + np.arange(d)[None, None, None, :, None]), (nf, d, d + 1, d, d))
            c = np.broadcast_to((bnodes[:, None, :, None, None] * nb + np.arange(d)[None, None, None, None, :]), (nf, d, d + 1, d, d))
            vals = np.broadcast_to(K[:, None], (nf, d, d + 1, d, d))
            A = A + sps.coo_matrix((vals.ravel(), (r.ravel(), c.ravel())), shape=A.shape)
        return A.tocsr()

    # ---- Dirichlet rows and Newton
    @staticmethod
    def with_dirichlet(A, dofs):
        """DirichletBC.apply(A): the rows become identity rows."""
        A = A.tolil(copy=True)
        for i in dofs:
            A.rows[i] = [int(i)]
            A.data[i] = [1.0]
        return A.tocsr()

    def newton_step(self, x, x0, dofs):
        R = self.residual(x, x0)
        R[dofs] = 0.0
        A = self.with_dirichlet(self.jacobian(x), dofs)
        return spla.spsolve(A.tocsc(), -R)

    def reduced_step(self, x, x0, dofs):
        """The Newton correction through the reduced (v, p) system: du = dt (q dv - r_u) on free displacement dofs, 0 on Dirichlet
        ones, the (v, p) system solved for (dv, dp)."""
        d, nb, q, dt = self.d, self.nb, self.q, self.dt
        n = self.nv * nb
        Ared, b, vp, ru, isd, allu = self.reduced_system(x, x0, dofs)
        y = spla.spsolve(Ared.tocsc(), b)
        dx = np.zeros(n)
        dx[vp] = y
        dv = dx.reshape(self.nv, nb)[:, d:2 * d].reshape(-1)
        du = dt * (q * dv - ru)
        du[isd[allu]] = 0.0
        dx[allu] = du
        return dx

    def reduced_system(self, x, x0, dofs):
        """(A_red, b_red, the (v, p) dofs it is written for, r_u, Dirichlet flags, the u dofs): the system the device assembles."""
        d, nb, q, dt = self.d, self.nb, self.q, self.dt
        n = self.nv * nb
        R = self.residual(x, x0)
        R[dofs] = 0.0
        A = self.jacobian(x).tocsr()
        u, v, p = self.split(x)
        u0, v0, p0 = self.split(x0)
        ru = ((u - u0) / dt - q * v - (1.0 - q) * v0).reshape(-1)
        isd = np.zeros(n, dtype=bool)
        isd[dofs] = True
        allu = (np.arange(self.nv)[:, None] * nb + np.arange(d)[None, :]).reshape(-1)
        free_u = allu[~isd[allu]]
        vp = np.sort(np.concatenate([(np.arange(self.nv)[:, None] * nb + d + np.arange(d + 1)[None, :]).reshape(-1)]))
        ru_full = np.zeros(n)
        ru_full[allu] = ru
        ru_full[isd] = 0.0
        P = sps.csr_matrix((np.ones(len(free_u)), (free_u, free_u)), shape=(n, n))
        Ared = A[vp][:, vp] + dt * q * (A[vp] @ P)[:, allu] @ sps.csr_matrix(
            (np.ones(len(allu)), (np.arange(len(allu)), allu + d)), shape=(len(allu), n))[:, vp]
        b = -R[vp] + dt * (A[vp] @ ru_full)
        # Dirichlet v / p rows: identity, zero right-hand side
        loc = {int(g_): i for i, g_ in enumerate(vp)}
        dl = [loc[int(i)] for i in dofs if int(i) in loc]
        Ared = self.with_dirichlet(Ared, dl)
        b[dl] = 0.0
        return Ared, b, vp, ru, isd, allu

    def residual_norm(self, x, x0, dofs):
        R = self.residual(x, x0)
        R[dofs] = 0.0
        return float(np.linalg.norm(R))

    def newton(self, x_start, x0, dofs, vals, atol=1e-9, rtol=1e-7, max_it=50):
        """(solution, iterations) of one time step; x_start: previous solution, boundary values imposed on the first iterate."""
        x = np.array(x_start, dtype=np.float64)
        x[dofs] = vals
        r0 = None
        for it in range(max_it + 1):
            R = self.residual(x, x0)
            R[dofs] = 0.0
            rn = float(np.linalg.norm(R))
            if r0 is None:
                r0 = rn
            if rn < atol or (r0 > 0 and rn / r0 < rtol):
                return x, it
            if it == max_it:
                raise RuntimeError('host Newton did not converge (residual %.3e)' % rn)
            A = self.with_dirichlet(self.jacobian(x), dofs)
            x = x + spla.spsolve(A.tocsc(), -R)
        return x, max_it


def crossed_rectangle(x0, y0, x1, y1, nx, ny):
    """DOLFIN's RectangleMesh(..., 'crossed') numbering: grid vertices x-fastest, then one centre vertex per square in square order;
    per square (v0, v1, c), (v0, v2, c), (v1, v3, c), (v2, v3, c)."""
    x = x0 + np.arange(nx + 1) * (x1 - x0) / nx
    y = y0 + np.arange(ny + 1) * (y1 - y0) / ny
    grid = np.stack([np.tile(x, ny + 1), np.repeat(y, nx + 1)], axis=1)
    iy, ix = np.meshgrid(np.arange(ny), np.arange(nx), indexing='ij')
    cx = x0 + (ix.ravel() + 0.5) * (x1 - x0) / nx
    cy = y0 + (iy.ravel() + 0.5) * (y1 - y0) / ny
    co = np.concatenate([grid, np.stack([cx, cy], axis=1)])
    v0 = (iy * (nx + 1) + ix).ravel()
    v1, v2 = v0 + 1, v0 + nx + 1
    v3 = v2 + 1
    c = (nx + 1) * (ny + 1) + np.arange(nx * ny)
    cells = np.stack([np.stack([v0, v1, c], 1), np.stack([v0, v2, c], 1), np.stack([v1, v3, c], 1), np.stack([v2, v3, c], 1)], 1)
    return co, cells.reshape(-1, 3)
