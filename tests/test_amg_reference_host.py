"""The host replay of the AMG V-cycle (amg_reference.py) against the cycle formed as an explicit dense matrix in extended precision.

A three-level smoothed-aggregation hierarchy is built with scipy - blocks of consecutive nodes as aggregates, constants per
component as the near-null space, P = (I - 4 / (3 lmax) D^-1 A) T, A_c = P^T A P - for one Poisson operator and one 3-dof
(elasticity) operator.  The dense cycle composes the same steps as matrices of np.longdouble, written down independently of the
replay: the Chebyshev smoother as its iteration matrix, the coarse-grid correction as x + P M_c R (b - A x).  The replay has to
stay inside the bound it reports for a device, so has the same cycle in plain float64 (a stand-in for the device: other orders of
summation, a rounding after every operation), and the bound has to meet the tightness condition every GPU case is held to."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import fem_oracle as fo

import amg_reference as ar
from spmv_reference import EPS, _host_product

LD = np.longdouble


def _poisson():
    co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), 7, 3, 2)
    kc = np.random.default_rng(0).uniform(0.5, 1.5, len(ce))
    K = fo.assemble_p1_scalar(co, ce, kc)
    dofs = np.nonzero((co[:, 2] == 0) | (co[:, 2] == 1))[0].astype(np.int32)
    A, _ = fo.apply_dirichlet(K, np.zeros(K.shape[0]), dofs, np.zeros(len(dofs)), True)
    return A.tocsr(), 1


def _elasticity():
    co, ce = fo.box_mesh((0, 0, 0), (2.0, 1.0, 1.0), 7, 2, 2)
    K = fo.assemble_p1_elasticity(co, ce, 2e11, 0.27)
    left = np.nonzero(co[:, 0] == 0)[0]
    dofs = (left[:, None] * 3 + np.arange(3)).ravel().astype(np.int32)
    A, _ = fo.apply_dirichlet(K, np.zeros(K.shape[0]), dofs, np.zeros(len(dofs)), True)
    return A.tocsr(), 3


def _hierarchy(A, bs, group, fp32):
    """levels for vcycle_replay: two coarsenings by aggregates of `group` consecutive nodes."""
    levels = []
    for _ in range(2):
        n = A.shape[0]
        nn = n // bs
        agg = np.arange(nn) // group
        size = np.bincount(agg)
        rows = np.arange(n)
        T = sp.csr_matrix((1.0 / np.sqrt(size[agg[rows // bs]]), (rows, agg[rows // bs] * bs + rows % bs)), shape=(n, (agg.max() + 1) * bs))
        lam = ar.largest_jacobi_eigenvalue(A)
        lmax = 1.1 * 0.93 * lam                      # (the library: 1.1 times a Rayleigh quotient below the eigenvalue)
        P = (T - sp.diags(4.0 / (3.0 * lmax) / A.diagonal()) @ A @ T).tocsr()
        levels.append({"A": A, "P": P, "lmax": lmax, "a32": fp32 and len(levels) > 0, "p32": fp32})
        A = (P.T @ A @ P).tocsr()
    lam = ar.largest_jacobi_eigenvalue(A)
    levels.append({"A": A, "P": None, "lmax": 1.1 * 0.93 * lam, "a32": fp32, "p32": False})
    return levels


# ---- the dense cycle --------------------------------------------------------------------------------------------------------------
def _dense(Op, fp32):
    Op = Op.toarray()
    return (Op.astype(np.float32) if fp32 else Op).astype(LD)


def _smoother_matrices(A, dinv, lmax, steps):
    """(S, E): `steps` Chebyshev steps take x to E x + S b (E = I - S A)."""
    n = A.shape[0]
    up, lo = 1.1 * lmax, 0.1 * lmax
    theta, delta = 0.5 * (up + lo), 0.5 * (up - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    Dinv = np.diag(dinv.astype(LD))
    # x_k = X_k b, d_k = D_k b from a zero guess
    D = LD(1.0 / theta) * Dinv
    X = D.copy()
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        D = LD(rho_new * rho) * D + LD(2.0 * rho_new / delta) * (Dinv @ (np.eye(n, dtype=LD) - A @ X))
        X = X + D
        rho = rho_new
    return X, np.eye(n, dtype=LD) - X @ A


def _dense_cycle(levels, l, steps, cinv):
    L = levels[l]
    A64 = sp.csr_matrix(L["A"])
    A = _dense(A64, L["a32"])
    d = A64.diagonal()
    dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    S, E = _smoother_matrices(A, dinv, L["lmax"], steps)
    if l == len(levels) - 1:
        if cinv is not None and l > 0:
            return cinv.astype(LD)
        M = S
        for _ in range(4 if l > 0 else 0):
            M = E @ M + S
        return M
    P = _dense(sp.csr_matrix(L["P"]), L["p32"])
    Mc = _dense_cycle(levels, l + 1, steps, cinv)
    X = S + P @ (Mc @ (P.T @ (np.eye(A.shape[0], dtype=LD) - A @ S)))
    return E @ X + S


def _plain_smooth(A, dinv, lmax, x, b, steps):
    up, lo = 1.1 * lmax, 0.1 * lmax
    theta, delta = 0.5 * (up + lo), 0.5 * (up - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    d = (1.0 / theta) * dinv * (b if x is None else b - A @ x)
    x = d.copy() if x is None else x + d
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        d = rho_new * rho * d + 2.0 * rho_new / delta * dinv * (b - A @ x)
        x = x + d
        rho = rho_new
    return x


def _plain_cycle(levels, l, b, steps, cinv):
    L = levels[l]
    A64 = sp.csr_matrix(L["A"])
    A = ar.rounded_to_fp32(A64) if L["a32"] else A64
    d = A64.diagonal()
    dinv = np.where(d != 0.0, 1.0 / np.where(d != 0.0, d, 1.0), 1.0)
    if l == len(levels) - 1:
        if cinv is not None and l > 0:
            return cinv @ b
        x = _plain_smooth(A, dinv, L["lmax"], None, b, steps)
        for _ in range(4 if l > 0 else 0):
            x = _plain_smooth(A, dinv, L["lmax"], x, b, steps)
        return x
    P = ar.rounded_to_fp32(L["P"]) if L["p32"] else sp.csr_matrix(L["P"])
    x = _plain_smooth(A, dinv, L["lmax"], None, b, steps)
    x = x + P @ _plain_cycle(levels, l + 1, P.T @ (b - A @ x), steps, cinv)
    return _plain_smooth(A, dinv, L["lmax"], x, b, steps)


CASES = [("poisson", _poisson, 6, False), ("elasticity_fp32", _elasticity, 6, True)]


@pytest.fixture(scope="module", params=CASES, ids=[c[0] for c in CASES])
def hierarchy(request):
    name, make, group, fp32 = request.param
    A, bs = make()
    levels = _hierarchy(A, bs, group, fp32)
    assert [L["A"].shape[0] for L in levels][-1] >= 2 * bs and len(levels) == 3
    return name, levels, np.linalg.inv(levels[-1]["A"].toarray())


def _rhs(n):
    e = np.zeros(n)
    e[-1] = 1.0
    return {"normal": np.random.default_rng(5).standard_normal(n), "unit": e, "ones": np.ones(n)}


@pytest.mark.parametrize("steps", [1, 2, 3])
@pytest.mark.parametrize("depth,dense_coarse", [(3, True), (3, False), (2, True), (2, False), (1, False)])
def test_replay_stays_inside_its_own_bound(hierarchy, depth, dense_coarse, steps):
    name, levels, _ = hierarchy
    levels = [dict(L) for L in levels[:depth]]
    levels[-1]["P"] = None
    cinv = np.linalg.inv(levels[-1]["A"].toarray()) if dense_coarse else None
    M = _dense_cycle(levels, 0, steps, cinv)
    prepared = ar.prepare(levels)
    for what, r in _rhs(levels[0]["A"].shape[0]).items():
        z, e = ar.vcycle_replay(prepared, r, steps, cinv)
        z_dense = M @ r.astype(LD)
        err = np.abs(z.astype(LD) - z_dense).astype(np.float64)
        assert np.all(np.isfinite(z)) and np.all(e >= 0)
        assert np.all(err <= e), (name, what, float((err / np.maximum(e, 1e-300)).max()))
        tight = e.max() / np.abs(z).max()
        print(name, "depth", depth, "dense" if dense_coarse else "chebyshev", "steps", steps, what, "max(e) / max|z| %.1e" % tight)
        assert tight <= ar.TIGHT, (name, what, tight)
        # a stand-in for the device: the same cycle in plain float64, every product in scipy's order of summation
        zp = _plain_cycle(levels, 0, r, steps, cinv)
        errp = np.abs(zp.astype(LD) - z_dense).astype(np.float64)
        assert np.all(errp <= e), (name, what, "plain float64", float((errp / np.maximum(e, 1e-300)).max()))
        # the bound is not vacuous either: it is within a few orders of the rounding of the result itself
        assert e.max() >= 0.5 * EPS * np.abs(z).max()
    # and the cycle is the symmetric operator the method promises (fp64 storage: R = P^T exactly, pre = post smoothing)
    sym = np.abs(M - M.T).max() / np.abs(M).max()
    assert sym <= (1e-6 if any(L["a32"] or L["p32"] for L in levels) else 1e-13), sym


def test_a_wrong_cycle_leaves_the_bound(hierarchy):
    """What the bound is for: the mistakes the GPU test has to catch move the result far outside it."""
    name, levels, cinv = hierarchy
    n = levels[0]["A"].shape[0]
    r = np.random.default_rng(6).standard_normal(n)
    z, e = ar.vcycle_replay(levels, r, 2, cinv)
    # smoother coefficients that are off in the sixth digit (every eigenvalue bound times 1 + 1e-6)
    M_ok = _dense_cycle(levels, 0, 2, cinv)
    assert np.all(np.abs((M_ok @ r.astype(LD)).astype(np.float64) - z) <= e)
    wrong = [dict(L, lmax=L["lmax"] * (1.0 + 1e-6)) for L in levels]
    zw = (_dense_cycle(wrong, 0, 2, cinv) @ r.astype(LD)).astype(np.float64)
    assert (np.abs(zw - z) > e).any()
    # a restriction that drops one entry of one column
    dropped = [dict(L) for L in levels]
    P = sp.lil_matrix(dropped[0]["P"])
    i = P[:, 0].nonzero()[0][-1]
    P[i, 0] = 0.0
    dropped[0]["P"] = P.tocsr()
    zd = (_dense_cycle(dropped, 0, 2, cinv) @ r.astype(LD)).astype(np.float64)
    assert (np.abs(zd - z) > e).any()


def test_host_product_takes_a_scipy_matrix_with_empty_rows():
    rng = np.random.default_rng(1)
    A = sp.random(40, 30, density=0.1, random_state=3, format="csr")
    A = sp.vstack([A, sp.csr_matrix((3, 30))]).tocsr()                  # trailing rows without entries
    A = sp.vstack([sp.csr_matrix((1, 30)), A]).tocsr()                  # and a leading one
    x = rng.standard_normal(30)
    y, ax = _host_product(A, x)
    assert np.abs(y - A @ x).max() <= 4 * EPS * ax.max() and np.allclose(ax, abs(A) @ np.abs(x), rtol=1e-14, atol=0)
    empty = np.diff(A.indptr) == 0
    assert empty.sum() >= 4 and np.all(y[empty] == 0.0) and np.all(ax[empty] == 0.0)
