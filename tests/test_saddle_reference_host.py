"""The host replays of the saddle-point preconditioners (saddle_reference.py) against the same operators formed as explicit dense
matrices in extended precision, on the linearised lid-driven cavity of a 2 x 2 x 2 Taylor-Hood cube and on a reduced
large-deformation-like CG1 block system; power_lmax against dense eigenvalues; the dense helpers against numpy.linalg.qr.

The dense operators are written down independently of the replays: the Chebyshev polynomials as their iteration matrices, the block
elimination as products of selection matrices.  Each replay has to stay inside the bound it reports for a device, so has the same
sequence in plain float64 (a stand-in for the device: scipy's order of summation, a rounding after every operation), the bound has
to meet the tightness condition of the GPU cases, and the mistakes the GPU test is there to catch have to leave it."""
import numpy as np
import pytest
import scipy.sparse as sp

from oracle import fem_oracle as fo, ns_oracle as ns

import amg_reference as ar
import saddle_reference as sr
from spmv_reference import EPS
from test_amg_reference_host import _dense_cycle, _hierarchy, _plain_cycle

LD = np.longdouble


def cavity(n, inv_dt, nu):
    """(J, g, Kp, Mp, th) of one linearised step of the lid-driven cavity, pressure pinned at vertex 0: the system of
    test_saddle_solve_lid_driven_cavity_step, from the oracle."""
    co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), n, n, n)
    th = ns.TaylorHood(co, ce)
    X = th.node_coords
    bn = th.boundary_nodes(lambda x: True)
    lid = bn[X[bn, 2] == 1.0]
    vals = np.zeros((th.n_nodes, 4))
    vals[lid, 0] = 1.0
    bc_dofs = np.concatenate([th.velocity_dofs(bn), th.pressure_dofs([0])])
    bc_vals = vals.ravel()[bc_dofs]
    w0 = np.zeros(th.n)
    w0[bc_dofs] = bc_vals
    Jr, gr = ns.ns_system(th, w0, nu, 1.0, inv_dt, np.zeros(th.n))
    J, g = ns.apply_dirichlet_rows(Jr, gr.copy(), bc_dofs, bc_vals)
    Kp = fo.assemble_p1_scalar(co, ce, 1.0)
    Kp, _ = fo.apply_dirichlet(Kp, np.zeros(th.nv), np.array([0], dtype=np.int32), np.zeros(1), True)
    Mp = fo.assemble_matrix(th.nv, ce, fo.p1_mass_local(co, ce, 1.0))
    return sp.csr_matrix(J), g, sp.csr_matrix(Kp), sp.csr_matrix(Mp), th


def _cheb_matrix(A, dinv, lo, up, steps, wrong=False):
    """X with x = X b after `steps` Chebyshev steps from a zero guess (dense, extended precision)."""
    n = A.shape[0]
    theta, delta = 0.5 * (up + lo), 0.5 * (up - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    Dinv = np.diag(dinv.astype(LD))
    D = LD(1.0 / theta) * Dinv
    X = D.copy()
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        D = LD(rho_new * (rho_new if wrong else rho)) * D + LD(2.0 * rho_new / delta) * (Dinv @ (np.eye(n, dtype=LD) - A @ X))
        X = X + D
        rho = rho_new
    return X


def _plain_cheb(A, dinv, b, lo, up, steps):
    theta, delta = 0.5 * (up + lo), 0.5 * (up - lo)
    sigma = theta / delta
    rho = 1.0 / sigma
    d = 1.0 / theta * dinv * b
    x = d.copy()
    for _ in range(1, steps):
        rho_new = 1.0 / (2.0 * sigma - rho)
        d = rho_new * rho * d + 2.0 * rho_new / delta * dinv * (b - A @ x)
        x = x + d
        rho = rho_new
    return x


def _dense_cc(J, Mp, levels, opts, cinv, wrong_mass=False):
    """P^-1 of sd_precond as a dense matrix of np.longdouble."""
    n, nv = J.shape[0], opts["nv"]
    A = J.toarray().astype(LD)
    vel = ((np.arange(n) & 3) != 3)
    dv = sr.jacobi_dinv(J) * vel
    if opts["velocity_sweeps"] > 1:
        Sv = _cheb_matrix(A, dv, opts["vel_lmax"] / 8.0, 1.1 * opts["vel_lmax"], opts["velocity_sweeps"])
    else:
        Sv = np.diag(dv.astype(LD))
    Sv = Sv * vel[:, None]
    prow = 4 * np.arange(nv) + 3
    Ep = np.zeros((nv, n), dtype=LD)
    Ep[np.arange(nv), prow] = 1.0
    Rp = Ep - (A[prow] * vel[None, :]) @ Sv                              # rp = Rp r
    Xm = _cheb_matrix(Mp.toarray().astype(LD), sr.scalar_dinv(Mp), 0.5, 2.5, 5, wrong_mass)
    r2 = opts["rho"] * opts["rho"]
    S = LD(r2 * opts["nu"]) * Xm
    if opts["inv_dt"] > 0.0 and levels is not None:
        S = S + LD(r2 * opts["inv_dt"]) * _dense_cycle(levels, 0, 2, cinv)
    P = Sv.copy()
    P[3::4] = 0.0
    P[np.arange(3, n, 4), np.arange(3, n, 4)] = 1.0                      # dummy slots and identity rows: z = r
    ident = J.diagonal()[prow] != 0.0
    for v in np.flatnonzero(~ident):
        P[prow[v]] = S[v] @ Rp
    return P


def _plain_cc(J, Mp, levels, opts, cinv, r):
    n, nv = J.shape[0], opts["nv"]
    vel = ((np.arange(n) & 3) != 3)
    dv = sr.jacobi_dinv(J) * vel
    if opts["velocity_sweeps"] > 1:
        zu = _plain_cheb(J, dv, r, opts["vel_lmax"] / 8.0, 1.1 * opts["vel_lmax"], opts["velocity_sweeps"]) * vel
    else:
        zu = dv * r
    prow = 4 * np.arange(nv) + 3
    rp = r[prow] - (J @ zu)[prow]
    p2 = _plain_cheb(Mp, sr.scalar_dinv(Mp), rp, 0.5, 2.5, 5)
    r2 = opts["rho"] * opts["rho"]
    zp = r2 * opts["nu"] * p2
    if opts["inv_dt"] > 0.0 and levels is not None:
        zp = r2 * opts["inv_dt"] * _plain_cycle(levels, 0, rp, 2, cinv) + zp
    z = zu.copy()
    z[3::4] = r[3::4]
    ident = J.diagonal()[prow] != 0.0
    z[prow] = np.where(ident, r[prow], zp)
    return z


def _rhs(n, dummy):
    e = np.zeros(n)
    e[4] = 1.0
    out = {"normal": np.random.default_rng(5).standard_normal(n), "unit": e, "ones": np.ones(n)}
    for v in out.values():
        v[dummy] = 0.0
    return out


@pytest.fixture(scope="module")
def cavities():
    out = {}
    for name, inv_dt, nu in (("steady", 0.0, 0.1), ("transient", 100.0, 0.01)):
        J, g, Kp, Mp, th = cavity(2, inv_dt, nu)
        levels = _hierarchy(Kp, 1, 3, False)[:2]
        levels = [dict(L) for L in levels]
        levels[-1]["P"] = None
        out[name] = (J, g, Kp, Mp, th, levels, np.linalg.inv(levels[-1]["A"].toarray()), inv_dt, nu)
    return out


@pytest.mark.parametrize("name,sweeps", [("steady", 1), ("steady", 3), ("transient", 1), ("transient", 3)])
def test_cahouet_chabard_replay_against_dense(cavities, name, sweeps):
    J, g, Kp, Mp, th, levels, cinv, inv_dt, nu = cavities[name]
    opts = {"nu": nu, "rho": 1.3, "inv_dt": inv_dt, "velocity_sweeps": sweeps, "nv": th.nv, "coarse": cinv,
            "vel_lmax": sr.power_lmax(J)}
    lv = levels if inv_dt else None
    P = _dense_cc(J, Mp, lv, opts, cinv)
    assert (J.diagonal()[3:4 * th.nv:4] != 0).sum() == 1                  # the pinned pressure: one identity row
    for what, r in dict(_rhs(th.n, th.dummy_dofs()), physical=g).items():
        z, e = sr.cahouet_chabard_replay(J, Mp, lv, opts, r)
        z_dense = P @ r.astype(LD)
        err = np.abs(z.astype(LD) - z_dense).astype(np.float64)
        assert np.all(np.isfinite(z)) and np.all(e >= 0)
        assert np.all(err <= e), (name, what, float((err / np.maximum(e, 1e-300)).max()))
        tight = e.max() / np.abs(z).max()
        print(name, "sweeps", sweeps, what, "max(e) / max|z| %.1e" % tight)
        assert tight <= sr.TIGHT
        zp = _plain_cc(J, Mp, lv, opts, cinv, r)
        errp = np.abs(zp.astype(LD) - z_dense).astype(np.float64)
        assert np.all(errp <= e), (name, what, "plain float64", float((errp / np.maximum(e, 1e-300)).max()))
        nz = np.abs(z) > 0
        assert np.all(e[nz & (e > 0)] >= 0.5 * EPS * np.abs(z[nz & (e > 0)]))       # not vacuous: above the rounding of z itself
        assert np.array_equal(z[th.dummy_dofs()], r[th.dummy_dofs()]) and z[3] == r[3]
    # the mistakes the GPU test has to catch leave the bound: rho_new * rho_new in the mass polynomial, lmax off in the sixth digit
    r = _rhs(th.n, th.dummy_dofs())["normal"]
    z, e = sr.cahouet_chabard_replay(J, Mp, lv, opts, r)
    zw = (_dense_cc(J, Mp, lv, opts, cinv, wrong_mass=True) @ r.astype(LD)).astype(np.float64)
    assert (np.abs(zw - z) > e).any()
    if sweeps > 1:
        zw = sr.cahouet_chabard_replay(J, Mp, lv, dict(opts, vel_lmax=opts["vel_lmax"] * (1 + 1e-6)), r)[0]
        assert (np.abs(zw - z) > e).any()


def _block_upper_system(tdim):
    """A CG1 block-4 operator with the shape of fs_assemble_large_deformation's: a stiffness-like velocity block, gradient /
    divergence couplings, a pressure block, two identity pressure rows; in 2-D the third slot of every vertex is a dummy unit row."""
    if tdim == 3:
        co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), 3, 2, 2)
    else:
        co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), 4, 3, 1)
    nv = len(co)
    K = sp.csr_matrix(fo.assemble_p1_scalar(co, ce, 1.0, mass_coef=30.0))
    Mp = sp.csr_matrix(fo.assemble_matrix(nv, ce, fo.p1_mass_local(co, ce, 1.0)))
    rng = np.random.default_rng(3)
    blocks = [[None] * 4 for _ in range(4)]
    for i in range(4):
        for j in range(4):
            c = K.copy()
            c.data = c.data * rng.uniform(0.1, 0.3, len(c.data)) * (0.2 if i != j else 1.0)
            blocks[i][j] = (K + c) if i == j and i < 3 else c
    if tdim == 2:
        for k in range(4):
            blocks[2][k] = blocks[k][2] = sp.csr_matrix((nv, nv))
        blocks[2][2] = sp.identity(nv, format="csr")
    J = sp.bmat(blocks, format="csr")
    perm = (np.arange(4)[None, :] * nv + np.arange(nv)[:, None]).ravel()           # node-major: four unknowns per vertex
    J = J[perm][:, perm].tolil()
    for v in (0, nv - 1):
        J[4 * v + 3, :] = 0.0
        J[4 * v + 3, 4 * v + 3] = 1.0
    J = sp.csr_matrix(J)
    J.eliminate_zeros()
    a0 = sp.kron(K, sp.identity(tdim), format="csr")                              # vector CG1, node-major
    return J, Mp, a0, nv


@pytest.mark.parametrize("tdim", [2, 3])
def test_block_upper_replay_against_dense(tdim):
    J, Mp, a0, nv = _block_upper_system(tdim)
    n = 4 * nv
    levels = [dict(L) for L in _hierarchy(a0, tdim, 3, False)[:2]]
    levels[-1]["P"] = None
    cinv = np.linalg.inv(levels[-1]["A"].toarray())
    opts = {"schur_scale": 0.37, "tdim": tdim, "coarse": cinv}
    ident = sr.identity_pressure_rows_ld(J, nv)
    assert ident.sum() == 2 and ident[0] and ident[-1]
    # dense: z_p = S^-1 r_p, z_v = Ainv (r_v - J_vp z_p)
    A = J.toarray().astype(LD)
    prow = 4 * np.arange(nv) + 3
    vrow = (4 * np.arange(nv)[:, None] + np.arange(tdim)).ravel()
    Sp = LD(1.0 / opts["schur_scale"]) * _cheb_matrix(Mp.toarray().astype(LD), sr.scalar_dinv(Mp), 0.5, 2.5, 5)
    Sp[ident] = 0.0
    Sp[np.flatnonzero(ident), np.flatnonzero(ident)] = 1.0
    Mc = _dense_cycle(levels, 0, 2, cinv)
    rng = np.random.default_rng(9)
    for what, r in (("normal", rng.standard_normal(n)), ("ones", np.ones(n))):
        z, e = sr.block_upper_replay(J, Mp, levels, opts, r)
        zn, en = sr.block_upper_replay(J, Mp, None, opts, r)            # without a hierarchy: everything but the velocity components
        rest = np.setdiff1d(np.arange(n), vrow)
        assert np.array_equal(zn[rest], z[rest]) and np.array_equal(en[rest], e[rest]) and np.all(np.isnan(zn[vrow]))
        zp = Sp @ r[prow].astype(LD)
        zv = Mc @ (r[vrow].astype(LD) - A[vrow][:, prow] @ zp)
        zd = np.zeros(n, dtype=LD)
        zd[prow], zd[vrow] = zp, zv
        if tdim == 2:
            zd[2::4] = r[2::4]
        err = np.abs(z.astype(LD) - zd).astype(np.float64)
        assert np.all(err <= e), (tdim, what, float((err / np.maximum(e, 1e-300)).max()))
        tight = e.max() / np.abs(z).max()
        print("block_upper", tdim, what, "max(e) / max|z| %.1e" % tight)
        assert tight <= sr.TIGHT
        # plain float64 stand-in for the device
        p2 = _plain_cheb(Mp, sr.scalar_dinv(Mp), r[prow], 0.5, 2.5, 5)
        y = np.zeros(n)
        y[prow] = np.where(ident, r[prow], 1.0 / opts["schur_scale"] * p2)
        zpl = np.zeros(n)
        zpl[vrow] = _plain_cycle(levels, 0, r[vrow] - (J @ y)[vrow], 2, cinv)
        zpl[prow] = y[prow]
        if tdim == 2:
            zpl[2::4] = r[2::4]
        errp = np.abs(zpl.astype(LD) - zd).astype(np.float64)
        assert np.all(errp <= e), (tdim, what, "plain float64", float((errp / np.maximum(e, 1e-300)).max()))
        # a schur_scale off in the sixth digit leaves the bound
        zw, _ = sr.block_upper_replay(J, Mp, levels, dict(opts, schur_scale=0.37 * (1 + 1e-6)), r)
        assert (np.abs(zw - z) > e).any()


def test_vcycle_replay_carries_the_bound_of_its_input():
    J, g, Kp, Mp, th = cavity(2, 100.0, 0.01)
    levels = [dict(L) for L in _hierarchy(Kp, 1, 3, False)[:2]]
    levels[-1]["P"] = None
    cinv = np.linalg.inv(levels[-1]["A"].toarray())
    rng = np.random.default_rng(2)
    r = rng.standard_normal(th.nv)
    er = 1e-12 * rng.uniform(0.0, 1.0, th.nv)
    z0, e0 = ar.vcycle_replay(levels, r, 2, cinv)
    z1, e1 = ar.vcycle_replay(levels, r, 2, cinv, e_r=er)
    assert np.array_equal(z0, z1) and np.all(e1 >= e0)
    M = np.abs(_dense_cycle(levels, 0, 2, cinv)).astype(np.float64)
    for s in (1.0, -1.0):                                   # a perturbed right-hand side inside e_r stays inside e1
        dr = s * er * np.sign(rng.standard_normal(th.nv))
        zp, _ = ar.vcycle_replay(levels, r + dr, 2, cinv)
        assert np.all(np.abs(zp - z0) <= e1)
    assert np.all(e1 - e0 >= (1.0 - 1e-6) * (M @ er))       # at least what the linear map itself does to e_r


@pytest.mark.parametrize("n,inv_dt,nu,expected", [(2, 0.0, 0.1, 0.93), (3, 0.0, 0.1, 0.94), (4, 0.0, 0.1, 0.97), (3, 100.0, 0.01, None),
                                                  (4, 100.0, 0.01, 0.96)])
def test_power_lmax_bounds_the_spectrum(n, inv_dt, nu, expected):
    """1.1 vel_lmax is the upper end of the Chebyshev interval: it has to lie above the largest eigenvalue of D^-1 A, and not far."""
    J = cavity(n, inv_dt, nu)[0]
    lam_true = sr.velocity_lambda_true(J)
    lm, lm64 = sr.power_lmax(J), sr.power_lmax(J, extended=False)
    ratio = lam_true / (1.1 * lm)
    print("n", n, "inv_dt", inv_dt, "lambda_true / (1.1 lmax) %.4f" % ratio, "fp64 against extended %.1e" % (abs(lm - lm64) / lm))
    assert 0.85 <= ratio <= 1.0
    if expected is not None:
        assert abs(ratio - expected) <= 0.01
    assert abs(lm - lm64) <= 1e-12 * lm
    v = sr.hashed_seed(16)
    assert np.all(v[3::4] == 0) and np.all(np.abs(v) < 1) and len(np.unique(v)) > 10
    x = (0 * 2654435761 + 12345) & 0xffffffff                             # entry 0 by hand, in Python integers
    x ^= x >> 16; x = (x * 0x7feb352d) & 0xffffffff; x ^= x >> 15; x = (x * 0x846ca68b) & 0xffffffff; x ^= x >> 16  # noqa: E702
    assert v[0] == (x & 0xffffff) / 8388608.0 - 1.0


def test_dense_helpers_against_qr():
    rng = np.random.default_rng(4)
    for k in (1, 5, 20):
        Hbar = np.triu(rng.standard_normal((k + 1, k)), -1)
        beta = 1.7
        # the rotations as k_sd_givens forms them
        R = Hbar.copy()
        cs, sn = np.zeros(k), np.zeros(k)
        gam = np.zeros(k + 1)
        gam[0] = beta
        for j in range(k):
            for i in range(j):
                a, c = R[i, j], R[i + 1, j]
                R[i, j], R[i + 1, j] = cs[i] * a + sn[i] * c, -sn[i] * a + cs[i] * c
            a, c = R[j, j], R[j + 1, j]
            d = np.hypot(a, c)
            cs[j], sn[j] = a / d, c / d
            R[j, j], R[j + 1, j] = d, 0.0
            gam[j + 1] = -sn[j] * gam[j]
            gam[j] = cs[j] * gam[j]
        back = sr.hessenberg_from_rotations(R, cs, sn, k)
        assert np.abs(back - Hbar).max() <= 64 * EPS * np.abs(Hbar).max()
        y, res = sr.least_squares(Hbar, beta)
        Q, Rq = np.linalg.qr(Hbar, mode="complete")
        rhs = Q.T[:, 0] * beta
        y_qr = np.linalg.solve(Rq[:k], rhs[:k])
        assert np.abs(y - y_qr).max() <= 1e-10 * np.abs(y_qr).max() * np.linalg.cond(Hbar)
        assert abs(res - abs(rhs[k])) <= 1e-12 * beta and abs(abs(gam[k]) - abs(rhs[k])) <= 1e-12 * beta
        assert np.abs(np.linalg.solve(np.triu(R[:k, :k]), gam[:k]) - y_qr).max() <= 1e-10 * np.abs(y_qr).max() * np.linalg.cond(Hbar)
    # two full passes leave an orthonormal basis even from nearly dependent columns
    n = 200
    base = rng.standard_normal(n)
    W = [base + 1e-7 * rng.standard_normal(n) for _ in range(6)]
    V = sr.two_pass_arnoldi(W, rng.standard_normal(n))
    assert sr.orthogonality_loss(V) <= 50 * EPS
