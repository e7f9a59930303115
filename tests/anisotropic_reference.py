"""Dense fp64 numpy reference of anisotropic linear elasticity on P1 tetrahedra / triangles (plane strain), for
tests/test_anisotropic_host.py and tests/test_gpu_anisotropic.py.

It is written the textbook way, on purpose unlike the kernels: the rank-4 tensor of every cell is ROTATED into the global axes,
C'_ijkl = R_ia R_jb R_kc R_ld C_abcd, folded to a 6x6, and the local matrices are V B^T D B with the strain-displacement matrix B.
The kernels (fs_anisotropic.hip) rotate the gradients instead and never form a rotated tensor.

Orders: the LIBRARY's tensor order (xx, yy, zz, xy, xz, yz) with engineering shears in the strain vector; the standard Voigt order
(11, 22, 33, 23, 13, 12) only where a function says so.  Tensor storage of stresses and eigenstrains: tensor components, 6 per cell
in 3-D, (xx, yy, zz, xy) in plane strain.
"""
import numpy as np
import scipy.sparse as sp

LIB = [(0, 0), (1, 1), (2, 2), (0, 1), (0, 2), (1, 2)]
VOIGT = [(0, 0), (1, 1), (2, 2), (1, 2), (0, 2), (0, 1)]
VOIGT_TO_LIBRARY = [0, 1, 2, 5, 4, 3]

# a CFRP-like orthotropic material (Pa): fibres along axis 1
CFRP = {'elastic_moduli': [140e9, 10e9, 8e9], 'poisson_ratios': [0.3, 0.25, 0.4], 'shear_moduli': [5e9, 4.5e9, 3e9]}


# ---- materials ---------------------------------------------------------------------------------------------------------------------
def compliance_voigt(E, nu, G):
    """Orthotropic compliance, standard Voigt order: nu = (nu12, nu13, nu23), G = (G12, G13, G23)."""
    E1, E2, E3 = E
    n12, n13, n23 = nu
    G12, G13, G23 = G
    S = np.zeros((6, 6))
    S[0] = [1 / E1, -n12 / E1, -n13 / E1, 0, 0, 0]
    S[1] = [-n12 / E1, 1 / E2, -n23 / E2, 0, 0, 0]
    S[2] = [-n13 / E1, -n23 / E2, 1 / E3, 0, 0, 0]
    S[3, 3], S[4, 4], S[5, 5] = 1 / G23, 1 / G13, 1 / G12
    return S


def orthotropic_voigt(E, nu, G):
    return np.linalg.inv(compliance_voigt(E, nu, G))


def isotropic_voigt(E, nu):
    mu, lm = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    C = np.zeros((6, 6))
    C[:3, :3] = lm
    for i in range(3):
        C[i, i] += 2 * mu
        C[3 + i, 3 + i] = mu
    return C


def to_library(Cv):
    """6x6 in the standard Voigt order -> the library order."""
    return np.asarray(Cv)[np.ix_(VOIGT_TO_LIBRARY, VOIGT_TO_LIBRARY)]


def plane_strain_compliance(S):
    """The 2x2 normal part of the plane-strain compliance (e_zz = 0 eliminates sigma_zz): S_ij - S_i3 S_j3 / S_33, i, j in x, y."""
    return S[:2, :2] - np.outer(S[:2, 2], S[:2, 2]) / S[2, 2]


def tensor4(D, order=LIB):
    """6x6 (engineering shears) -> C[3,3,3,3] with the minor and major symmetries."""
    C = np.zeros((3, 3, 3, 3))
    for I, (i, j) in enumerate(order):
        for J, (k, l) in enumerate(order):
            C[i, j, k, l] = C[j, i, k, l] = C[i, j, l, k] = C[j, i, l, k] = D[I, J]
    return C


def matrix6(C, order=LIB):
    return np.array([[C[i, j, k, l] for (k, l) in order] for (i, j) in order])


def rotate4(C, R):
    """C'_ijkl = R_ia R_jb R_kc R_ld C_abcd: columns of R = material axes in global coordinates."""
    return np.einsum('ia,jb,kc,ld,abcd->ijkl', R, R, R, R, C)


def global_D(table, index, frames, nc):
    """The 6x6 (library order) of every cell in global axes, [nc, 6, 6], by rotating the rank-4 tensor."""
    table = np.asarray(table, dtype=np.float64)
    if index is None:
        index = np.arange(nc) if len(table) == nc and nc > 1 else np.zeros(nc, dtype=np.int64)
    if frames is None:
        return table[index]
    C4 = np.stack([tensor4(D) for D in table])[index]
    R = np.asarray(frames, dtype=np.float64).reshape(nc, 3, 3)
    C4 = np.einsum('nia,njb,nkc,nld,nabcd->nijkl', R, R, R, R, C4, optimize=True)
    ii, jj = np.array(LIB).T
    return C4[:, ii[:, None], jj[:, None], ii[None, :], jj[None, :]]


def random_rotations(n, seed, about_z=False):
    rng = np.random.default_rng(seed)
    if about_z:
        t = rng.uniform(0, 2 * np.pi, n)
        R = np.zeros((n, 3, 3))
        R[:, 0, 0], R[:, 0, 1], R[:, 1, 0], R[:, 1, 1], R[:, 2, 2] = np.cos(t), -np.sin(t), np.sin(t), np.cos(t), 1.0
        return R
    Q = np.linalg.qr(rng.standard_normal((n, 3, 3)))[0]
    Q[:, :, 2] *= np.sign(np.linalg.det(Q))[:, None]
    return Q


def rotation_about(axis, angle):
    """Rodrigues' rotation matrix."""
    a = np.asarray(axis, dtype=np.float64) / np.linalg.norm(axis)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * K + (1 - np.cos(angle)) * K @ K


# ---- P1 cells ------------------------------------------------------------------------------------------------------------------------
def geometry(co, ce):
    """(volume or area [nc], gradients [nc, d+1, d]) of the barycentric functions."""
    X = np.asarray(co, dtype=np.float64)[np.asarray(ce, dtype=np.int64)]
    d = X.shape[1] - 1
    J = np.stack([X[:, k, :d] - X[:, 0, :d] for k in range(1, d + 1)], axis=2)
    Ji = np.linalg.inv(J)
    g = np.zeros((len(X), d + 1, d))
    g[:, 1:] = Ji
    g[:, 0] = -Ji.sum(axis=1)
    return np.abs(np.linalg.det(J)) / (6.0 if d == 3 else 2.0), g


def strain_displacement(g):
    """B [nc, 6, d (d+1)]: (e_xx, e_yy, e_zz, 2e_xy, 2e_xz, 2e_yz) = B u_cell, dofs node-major; plane strain: rows zz, xz, yz are 0."""
    nc, nn, d = g.shape
    B = np.zeros((nc, 6, nn * d))
    for a in range(nn):
        for i in range(d):
            B[:, i, a * d + i] = g[:, a, i]
        B[:, 3, a * d + 0] = g[:, a, 1]
        B[:, 3, a * d + 1] = g[:, a, 0]
        if d == 3:
            B[:, 4, a * d + 0] = g[:, a, 2]
            B[:, 4, a * d + 2] = g[:, a, 0]
            B[:, 5, a * d + 1] = g[:, a, 2]
            B[:, 5, a * d + 2] = g[:, a, 1]
    return B


def cell_dofs(ce, d):
    return (np.asarray(ce, dtype=np.int64)[:, :d + 1, None] * d + np.arange(d)).reshape(len(ce), d * (d + 1))


def local_stiffness(co, ce, Dg):
    vol, g = geometry(co, ce)
    B = strain_displacement(g)
    return vol[:, None, None] * np.einsum('cIp,cIJ,cJq->cpq', B, Dg, B)


def local_mass(co, ce, rho):
    vol, g = geometry(co, ce)
    nn, d = g.shape[1], g.shape[2]
    base = (np.ones((nn, nn)) + np.eye(nn)) / ((nn + 1.0) * nn)           # int phi_a phi_b / V: (1 + delta) / 20 or / 12
    M = np.kron(base, np.eye(d))
    return (vol * np.broadcast_to(np.asarray(rho, dtype=np.float64), vol.shape))[:, None, None] * M[None]


def assemble(n_nodes, ce, Ke, d):
    cd = cell_dofs(ce, d)
    nd = cd.shape[1]
    A = sp.coo_matrix((Ke.ravel(), (np.repeat(cd, nd, axis=1).ravel(), np.tile(cd, (1, nd)).ravel())),
                      shape=(d * n_nodes, d * n_nodes)).tocsr()
    A.sum_duplicates()
    A.sort_indices()
    return A


def to_vector(T, d):
    """tensor storage [nc, 6 or 4] -> strain-type vectors [nc, 6] (engineering shears, library order)."""
    T = np.asarray(T, dtype=np.float64)
    v = np.zeros((len(T), 6))
    v[:, :3] = T[:, :3]
    v[:, 3] = 2.0 * T[:, 3]
    if d == 3:
        v[:, 4], v[:, 5] = 2.0 * T[:, 4], 2.0 * T[:, 5]
    return v


def to_storage(sv, d):
    """stress vectors [nc, 6] (library order) -> the tensor storage."""
    return sv if d == 3 else sv[:, :4]


def cell_stress(co, ce, u, Dg, eigenstrain=None):
    """sigma = C : (eps(u) - eps*) per cell in the tensor storage; u: [n_nodes * d] or None."""
    vol, g = geometry(co, ce)
    d = g.shape[2]
    ev = np.zeros((len(ce), 6))
    if u is not None:
        ev = np.einsum('cIp,cp->cI', strain_displacement(g), np.asarray(u)[cell_dofs(ce, d)])
    if eigenstrain is not None:
        ev = ev - to_vector(eigenstrain, d)
    return to_storage(np.einsum('cIJ,cJ->cI', Dg, ev), d)


def eigenstress_load(n_nodes, co, ce, Dg, eigenstrain):
    """b = int (C : eps*) : grad v dx."""
    vol, g = geometry(co, ce)
    d = g.shape[2]
    sv = np.einsum('cIJ,cJ->cI', Dg, to_vector(eigenstrain, d))
    be = vol[:, None] * np.einsum('cIp,cI->cp', strain_displacement(g), sv)
    b = np.zeros(d * n_nodes)
    np.add.at(b, cell_dofs(ce, d).ravel(), be.ravel())
    return b


def von_mises_cells(stress, d):
    """sqrt(3/2 s:s) per cell from the tensor storage; d == 2: the reference's expression with dimension 2, the 2x2 tensor less
    tr / 3 (LinearElasticitySolver.py:71-73 keeps the 1/3)."""
    s = np.asarray(stress)
    if d == 3:
        p = s[:, :3].sum(axis=1) / 3.0
        ss = ((s[:, :3] - p[:, None]) ** 2).sum(axis=1) + 2.0 * (s[:, 3:] ** 2).sum(axis=1)
    else:
        p = (s[:, 0] + s[:, 1]) / 3.0
        ss = (s[:, 0] - p) ** 2 + (s[:, 1] - p) ** 2 + 2.0 * s[:, 3] ** 2
    return np.sqrt(1.5 * ss)


def von_mises_rhs(n_nodes, co, ce, stress):
    """b_a = int vm lambda_a dx = sum over the cells of vertex a of vm V / (d + 1)."""
    vol, g = geometry(co, ce)
    d = g.shape[2]
    w = von_mises_cells(stress, d) * vol / (d + 1.0)
    b = np.zeros(n_nodes)
    np.add.at(b, np.asarray(ce, dtype=np.int64)[:, :d + 1].ravel(), np.repeat(w, d + 1))
    return b
