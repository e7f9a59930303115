"""numpy / scipy restatement of the P1 geometric stiffness of linear buckling: the cell stress of a displacement, the scalar
node-pair matrix s_ab = sum_cells |c| grad N_a . sigma_c grad N_b, its expansion K_G[(a,i),(b,j)] = delta_ij s_ab (tetrahedra and
plane-strain triangles) and the dense pencil solve K_G phi = nu K phi.  The independent check of fs_buckling.hip and
fs_buckling_solve."""
import numpy as np
import scipy.linalg as sla
import scipy.sparse as sps


def geometry(coords, cells):
    """(g [nc, d+1, d] gradients of the barycentric functions, vol [nc]) of a simplex mesh."""
    cells = np.asarray(cells, dtype=np.int64)
    d = cells.shape[1] - 1
    X = np.asarray(coords, dtype=np.float64)[:, :d][cells]
    J = np.stack([X[:, k] - X[:, 0] for k in range(1, d + 1)], axis=2)       # columns: edge vectors
    Ji = np.linalg.inv(J)
    g = np.zeros((len(cells), d + 1, d))
    g[:, 1:, :] = Ji
    g[:, 0, :] = -Ji.sum(axis=1)
    vol = np.abs(np.linalg.det(J)) / (6.0 if d == 3 else 2.0)
    return g, vol


def cell_stress(coords, cells, u, mu, lmbda):
    """(sigma [nc, d, d] in-plane tensor, record [nc, 6] as xx, yy, zz, xy, xz, yz or [nc, 4] as xx, yy, zz, xy in plane strain) of
    sigma = lambda tr(eps) I + 2 mu eps for the P1 displacement u [n_dofs]; mu / lmbda numbers or arrays [nc]."""
    cells = np.asarray(cells, dtype=np.int64)
    nc, d = cells.shape[0], cells.shape[1] - 1
    g, _ = geometry(coords, cells)
    U = np.asarray(u, dtype=np.float64).reshape(-1, d)[cells]                # [nc, d+1, d]
    H = np.einsum("cai,caj->cij", U, g)
    eps = 0.5 * (H + H.transpose(0, 2, 1))
    tr = np.trace(eps, axis1=1, axis2=2)
    mu = np.broadcast_to(np.asarray(mu, dtype=np.float64), (nc,))
    lmbda = np.broadcast_to(np.asarray(lmbda, dtype=np.float64), (nc,))
    sig = 2.0 * mu[:, None, None] * eps + (lmbda * tr)[:, None, None] * np.eye(d)[None]
    if d == 3:
        rec = np.stack([sig[:, 0, 0], sig[:, 1, 1], sig[:, 2, 2], sig[:, 0, 1], sig[:, 0, 2], sig[:, 1, 2]], axis=1)
    else:
        rec = np.stack([sig[:, 0, 0], sig[:, 1, 1], lmbda * tr, sig[:, 0, 1]], axis=1)
    return sig, rec


def scalar_geometric(coords, cells, sigma):
    """s [n_nodes, n_nodes] CSR with s_ab = sum_cells |c| g_a . sigma_c g_b for a per-cell stress sigma [nc, d, d]; every node pair
    that shares a cell has a stored entry, also where it sums to zero."""
    cells = np.asarray(cells, dtype=np.int64)
    nv = cells.shape[1]
    g, vol = geometry(coords, cells)
    se = vol[:, None, None] * np.einsum("cai,cij,cbj->cab", g, sigma, g)
    rows = np.repeat(cells, nv, axis=1).ravel()
    cols = np.tile(cells, (1, nv)).ravel()
    n = np.asarray(coords).shape[0]
    S = sps.coo_matrix((se.ravel(), (rows, cols)), shape=(n, n)).tocsr()     # duplicates summed, explicit zeros kept
    S.sort_indices()
    return S


def expand_blocks(S, d):
    """The block matrix with blocks s_ab I_d as CSR with FULL d x d blocks stored (off-diagonal block entries 0.0)."""
    S = S.tocsr()
    S.sort_indices()
    n = S.shape[0]
    indptr = [0]
    indices, data = [], []
    eye = np.eye(d)
    for a in range(n):
        sl = slice(S.indptr[a], S.indptr[a + 1])
        cols = (S.indices[sl].astype(np.int64)[:, None] * d + np.arange(d)[None, :]).ravel()
        for i in range(d):
            indices.append(cols)
            data.append((S.data[sl][:, None] * eye[i][None, :]).ravel())
            indptr.append(indptr[-1] + cols.size)
    return sps.csr_matrix((np.concatenate(data), np.concatenate(indices), np.asarray(indptr)), shape=(n * d, n * d))


def geometric_stiffness_csr(coords, cells, u, mu, lmbda, sigma=None):
    """K_G as CSR with full blocks (the storage the device matrix reports through to_csr)."""
    d = np.asarray(cells).shape[1] - 1
    if sigma is None:
        sigma, _ = cell_stress(coords, cells, u, mu, lmbda)
    return expand_blocks(scalar_geometric(coords, cells, sigma), d)


def geometric_stiffness(coords, cells, u, mu, lmbda, sigma=None):
    """K_G dense [n_dofs, n_dofs]."""
    return geometric_stiffness_csr(coords, cells, u, mu, lmbda, sigma).toarray()


def dense_pencil(KG_free, K_free):
    """(nu ascending, phi columns K-orthonormal) of K_G phi = nu K phi on the free dofs; the buckling factors are -1 / nu for nu < 0."""
    return sla.eigh(np.asarray(KG_free), np.asarray(K_free))
