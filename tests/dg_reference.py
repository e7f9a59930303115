"""Numpy restatement of the upwind SIPG DG1 advection-diffusion form of ScalarTransportDGSolver (host, fp64).

Every integral is evaluated by quadrature with the basis functions evaluated at physical points through each cell's inverse map,
normals from the facet geometry and h from the circumcentre - not by the closed forms the device kernels use - so that it is an
independent derivation.  Dof (K, a) = (d+1) K + a in the caller's numbering.  On an interior facet '+' is the cell with the larger
key (key = marker * n_cells - cell number: the lower number, or the larger marker where the markers differ).

    A = op c a(T, v) + mass int T v dx + sum_listed int_F h T v ds
    b = int f_h v dx + sum_listed int_F g_h v ds      (f_h, g_h: P1 interpolants of the dof / vertex values)
"""
import numpy as np
import scipy.sparse as sp

# degree-2 rules: barycentric points, weights summing to 1
_TRI_Q = (np.array([[0.5, 0.5, 0.0], [0.0, 0.5, 0.5], [0.5, 0.0, 0.5]]), np.full(3, 1.0 / 3.0))
_A, _B = 0.5854101966249685, 0.1381966011250105
_TET_Q = (np.array([[_A, _B, _B, _B], [_B, _A, _B, _B], [_B, _B, _A, _B], [_B, _B, _B, _A]]), np.full(4, 0.25))
_G = 0.5 / np.sqrt(3.0)
_SEG_Q = (np.array([[0.5 + _G, 0.5 - _G], [0.5 - _G, 0.5 + _G]]), np.full(2, 0.5))


def _cell_maps(co, cells):
    X = co[cells]                                            # [nc, L, d]
    J = np.stack([X[:, k + 1] - X[:, 0] for k in range(X.shape[2])], axis=2)   # columns x_k - x_0
    Jinv = np.linalg.inv(J)
    d = X.shape[2]
    vol = np.abs(np.linalg.det(J)) / (2.0 if d == 2 else 6.0)
    grad = np.concatenate([-Jinv.sum(axis=1, keepdims=True), Jinv], axis=1)   # [nc, L, d]
    return X, Jinv, vol, grad


def _bary(X0, Jinv, p):
    """barycentric coordinates of points p [n, q, d] in cells (X0 [n, d], Jinv [n, d, d]) -> [n, q, d+1]"""
    lam = np.einsum("nij,nqj->nqi", Jinv, p - X0[:, None, :])
    return np.concatenate([1.0 - lam.sum(axis=2, keepdims=True), lam], axis=2)


def circum_h(X):
    """2 x circumradius of simplices X [n, d+1, d] (circumcentre from its linear system)."""
    x0 = X[:, 0]
    E = X[:, 1:] - x0[:, None, :]
    rhs = 0.5 * (E ** 2).sum(axis=2)
    c = np.linalg.solve(E, rhs[..., None])[..., 0]
    return 2.0 * np.linalg.norm(c, axis=1)


def _facet_quad(P):
    """quadrature on facets with vertices P [n, d, d]: points [n, q, d], weights*measure [n, q], unit normal (any sign) [n, d]"""
    d = P.shape[2]
    if d == 2:
        xi, w = _SEG_Q
        e = P[:, 1] - P[:, 0]
        meas = np.linalg.norm(e, axis=1)
        nrm = np.stack([e[:, 1], -e[:, 0]], axis=1) / meas[:, None]
    else:
        xi, w = _TRI_Q
        c = np.cross(P[:, 1] - P[:, 0], P[:, 2] - P[:, 0])
        meas = 0.5 * np.linalg.norm(c, axis=1)
        nrm = c / (2.0 * meas[:, None])
    pts = np.einsum("qj,njd->nqd", xi, P)
    return pts, w[None, :] * meas[:, None], nrm


def _outward(nrm, Xc, P):
    """flip normals to point away from the cell (Xc [n, L, d] its vertices, P the facet's)"""
    s = np.sign(np.einsum("nd,nd->n", nrm, P[:, 0] - Xc.mean(axis=1)))
    return nrm * s[:, None]


def assemble(mesh, conductivity, capacity, velocity, alpha, op=1.0, mass=0.0, facet_cell=None, facet_local=None, facet_h=None,
             facet_g=None, source=None, key=None):
    """(A as scipy CSR, b) in the API dof order of the DG1 space of ``mesh``."""
    co = mesh.coordinates()
    cells = mesh.cells().astype(np.int64)
    nc, L = cells.shape
    d = L - 1
    beta = np.asarray(velocity, dtype=np.float64)[:d]
    k, c = float(conductivity), float(capacity)
    X, Jinv, vol, grad = _cell_maps(co, cells)
    hK = circum_h(X)
    if key is None:
        key = -np.arange(nc)
    rows, cols, vals = [], [], []
    b = np.zeros(nc * L)

    def add(r_cells, c_cells, blocks):                     # blocks [n, L, L]
        r = r_cells[:, None, None] * L + np.arange(L)[None, :, None]
        cc = c_cells[:, None, None] * L + np.arange(L)[None, None, :]
        rows.append(np.broadcast_to(r, blocks.shape).ravel())
        cols.append(np.broadcast_to(cc, blocks.shape).ravel())
        vals.append(blocks.ravel())

    # cells
    xi, w = _TET_Q if d == 3 else _TRI_Q
    pts = np.einsum("qj,njd->nqd", xi, X)
    phi = _bary(X[:, 0], Jinv, pts)                         # [nc, q, L]
    wq = w[None, :] * vol[:, None]
    stiff = k * np.einsum("nad,nbd->nab", grad, grad) * vol[:, None, None]
    adv = -c * np.einsum("nq,nqb,na->nab", wq, phi, grad @ beta)
    Mk = np.einsum("nq,nqa,nqb->nab", wq, phi, phi)
    add(np.arange(nc), np.arange(nc), op * (stiff + adv) + mass * Mk)
    if source is not None:
        fq = np.einsum("nqa,na->nq", phi, np.asarray(source, dtype=np.float64).reshape(nc, L))
        b += np.einsum("nq,nq,nqa->na", wq, fq, phi).ravel()

    # interior facets
    pairs, _ = mesh.interior_facet_cells()
    ca, cb = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    shared = np.array([[v for v in cells[i] if v in set(cells[j])] for i, j in zip(ca, cb)], dtype=np.int64)
    P = co[shared]
    fp, fw, nrm = _facet_quad(P)
    plus_is_a = key[ca] > key[cb]
    cp, cm = np.where(plus_is_a, ca, cb), np.where(plus_is_a, cb, ca)
    n_plus = _outward(nrm, X[cp], P)
    hp = hK[cp]
    ph_p, ph_m = _bary(X[cp, 0], Jinv[cp], fp), _bary(X[cm, 0], Jinv[cm], fp)
    gn_p, gn_m = np.einsum("nad,nd->na", grad[cp], n_plus), np.einsum("nad,nd->na", grad[cm], n_plus)
    bn = n_plus @ beta
    bplus, bminus = np.maximum(bn, 0.0), np.maximum(-bn, 0.0)
    side = {0: (cp, ph_p, gn_p, 1.0), 1: (cm, ph_m, gn_m, -1.0)}
    for s in (0, 1):
        cs, phs, gs, sig_s = side[s]
        for t in (0, 1):
            ct, pht, gt, sig_t = side[t]
            pen = (k * alpha / hp)[:, None, None] * sig_s * sig_t * np.einsum("nq,nqa,nqb->nab", fw, phs, pht)
            t2 = -k * 0.5 * gs[:, :, None] * sig_t * np.einsum("nq,nqb->nb", fw, pht)[:, None, :]
            t3 = -k * 0.5 * sig_s * np.einsum("nq,nqa->na", fw, phs)[:, :, None] * gt[:, None, :]
            up = (bplus if t == 0 else -bminus)[:, None, None] * c * sig_s * np.einsum("nq,nqa,nqb->nab", fw, phs, pht)
            add(cs, ct, op * (pen + t2 + t3 + up))

    # boundary facets: outflow
    cf = mesh.cell_facets().astype(np.int64)
    ext = mesh.exterior_facets()
    bc_, bl_ = np.nonzero(ext[cf])
    Pb = co[np.stack([cells[bc_][:, j] for j in range(L)], axis=1)]
    Pb = np.stack([Pb[i][np.arange(L) != bl_[i]] for i in range(len(bc_))]) if len(bc_) else np.zeros((0, d, d))
    if len(bc_):
        bp, bw, bn_ = _facet_quad(Pb)
        nb = _outward(bn_, X[bc_], Pb)
        bout = np.maximum(nb @ beta, 0.0)
        phb = _bary(X[bc_, 0], Jinv[bc_], bp)
        add(bc_, bc_, op * c * bout[:, None, None] * np.einsum("nq,nqa,nqb->nab", bw, phb, phb))
    # listed facets
    if facet_cell is not None and len(facet_cell):
        fc, fl = np.asarray(facet_cell, dtype=np.int64), np.asarray(facet_local, dtype=np.int64)
        Pf = np.stack([co[cells[fc[i]][np.arange(L) != fl[i]]] for i in range(len(fc))])
        qp, qw, _ = _facet_quad(Pf)
        phf = _bary(X[fc, 0], Jinv[fc], qp)
        if facet_h is not None:
            h = np.broadcast_to(np.asarray(facet_h, dtype=np.float64), (len(fc),))
            add(fc, fc, h[:, None, None] * np.einsum("nq,nqa,nqb->nab", qw, phf, phf))
        if facet_g is not None:
            g = np.asarray(facet_g, dtype=np.float64).reshape(len(fc), L)
            gq = np.einsum("nqa,na->nq", phf, g)
            contrib = np.einsum("nq,nq,nqa->na", qw, gq, phf)
            np.add.at(b, (fc[:, None] * L + np.arange(L)[None, :]).ravel(), contrib.ravel())
    A = sp.coo_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(nc * L, nc * L)).tocsr()
    A.sum_duplicates()
    return A, b


def geometric_dirichlet_dofs(mesh, facet_ids):
    """DG dofs whose vertex lies on one of the facets (DOLFIN's "geometric" DirichletBC on a DG space)."""
    verts = np.unique(mesh.facets()[facet_ids].ravel())
    on = np.zeros(mesh.num_vertices(), dtype=bool)
    on[verts] = True
    return np.nonzero(on[mesh.cells().ravel()])[0]


def apply_dirichlet(A, b, dofs, vals):
    """rows -> identity rows, b_i = g (the later entry wins on duplicates)"""
    A = A.tolil(copy=True)
    b = b.copy()
    for i, g in zip(dofs, vals):
        A.rows[i] = [int(i)]
        A.data[i] = [1.0]
        b[i] = g
    return A.tocsr(), b


def cg1_projection(mesh, T):
    """L2 projection of the DG1 field T (API dof order) onto CG1: consistent mass matrix, no boundary conditions."""
    from scipy.sparse.linalg import spsolve
    co = mesh.coordinates()
    cells = mesh.cells().astype(np.int64)
    nc, L = cells.shape
    X, Jinv, vol, _ = _cell_maps(co, cells)
    xi, w = _TET_Q if L == 4 else _TRI_Q
    phi = _bary(X[:, 0], Jinv, np.einsum("qj,njd->nqd", xi, X))
    Mk = np.einsum("nq,nqa,nqb->nab", w[None, :] * vol[:, None], phi, phi)
    r = np.broadcast_to(cells[:, :, None], Mk.shape).ravel()
    cc = np.broadcast_to(cells[:, None, :], Mk.shape).ravel()
    M = sp.coo_matrix((Mk.ravel(), (r, cc)), shape=(len(co), len(co))).tocsr()
    rhs = np.zeros(len(co))
    np.add.at(rhs, cells.ravel(), np.einsum("nab,nb->na", Mk, np.asarray(T).reshape(nc, L)).ravel())
    return spsolve(M.tocsc(), rhs)
