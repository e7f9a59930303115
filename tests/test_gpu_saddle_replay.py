"""fs_saddle_solve (fs_saddle_solve.inc, part of fs_saddle.hip: restarted FGMRES with the Arnoldi state on the device, the Cahouet-Chabard
and the block-upper preconditioner) held to a host replay of its last cycle.  The solver recomputes the true residual at every restart
and stops on it, so a wrong preconditioner or a wrong Hessenberg column only costs iterations and every test that looks at the
solution, `converged` and an iteration ceiling stays green.  Here every case is ONE saddle_solve / large_deformation_solve call with
rtol = atol = 0 and max_iter the wanted iteration count, then backend.saddle_last_cycle() (the inspection hook fs_saddle_last_cycle),
and the matrices are the device's own (to_csr, AMG.level_matrix, level_info()["lambda_max"], coarse_inverse()).  Per cycle read:

 (a) every Z_j within the carried bound of saddle_reference.cahouet_chabard_replay / block_upper_replay applied to the device's own
     V_j, in every component, the bound inside the tightness condition max(e_z) <= 1e-9 max|z_ref| (amg_reference.TIGHT); with
     velocity_sweeps = 3 the device's vel_lmax against power_lmax and lambda_true <= 1.1 vel_lmax;
 (b) J Z_j = V_{0..j+1} Hbar_j with Hbar rebuilt from the device's R, cs, sn: defect <= 64 (j + 2) eps sum_i |Hbar_ij| ||V_i||_inf + the
     product's own row bound, whatever the orthogonality is (the products, k_sd_multi_axpy, k_sd_hess_pass, k_sd_givens);
 (c) the largest entry of |V^T V - I| at most 1000 times that of the same J Z orthogonalised on the host by two full fp64 passes;
 (d) the device's count of second Gram-Schmidt passes inside [sure, sure + borderline] of the ratios the host computes from the
     device's V and J Z (borderline: within 5 % of the threshold);
 (e) |gamma_kuse| = ||b - J x||, x = x0 + Z y_ls, (J Z)^T (b - J x) = 0, each defect at most 10 times the same defect of the host's
     own fp64 solution from the same V and Z with a floor of 64 eps scale; iterations == max_iter, converged == 0, rel_residual the
     host's true residual.
One converging run per regime: converged == 1, the true residual below rtol ||b|| and the iteration count of the host FGMRES
(saddle_reference.host_fgmres) driven by the replayed preconditioner, at an rtol that the test places in the middle of the
largest single-iteration drop of the host's history (at least a factor 2 on both sides).

Not every (system, right-hand side, plan) combination runs: every system runs the 20-iteration cycle (three groups of SD_DOT_GROUP);
on the edge-3 cube every regime runs every plan, and every regime and both block_upper systems run both right-hand sides, see CASES.
The 2-D block_upper system has no hierarchy (fs_amg_setup takes no blocks of 2) and its velocity solve is the inner CG, no fixed
operator: (a) holds the pressure rows (take-p, the Mp polynomial, 1 / schur_scale, identity rows) and the dummy slot of every Z_j to
the replay - both bit for bit where the replay's bound is 0 - and only the two velocity components are left to (b) to (e).  The large case (Taylor-Hood cube of edge 16, 143 748 rows: a
second pass of the strided loops of k_sd_multi_dot, k_sd_multi_axpy, k_sd_scale_dev) takes (b) to (e) in plain fp64.

Tolerance of vel_lmax: 100 times the spread of power_lmax between float64 and extended-precision products, the spread taken as at
least eps lmax (measured on the CPU: 0 to 1.4e-16 relative, so the tolerance is 2.2e-14 relative)."""
# Measured on the MI355X (the whole file: 3.3 s).  Per case the largest err / e_z of (a) and next to it the largest max(e_z) / max|z_ref|,
# the tightness figure (condition 1e-9); then the largest defect / bound of (b); then (c): the device's largest |V^T V - I| and L_ref of
# the two host passes; then the second passes of the device / the iterations of the cycle; levels = those of the hierarchy.
#   cube3_steady1 normal one      0.44, 7.4e-13     0.0038   6.7e-16, 4.4e-16   20/20
#   cube3_steady3 normal one      0.0085, 9.0e-12   0.0031   7.8e-16, 8.9e-16   20/20   lambda_true / (1.1 vel_lmax) 0.941
#   cube3_transient normal one    0.45, 1.0e-11     0.0051   4.4e-16, 4.4e-16   19/20   2 levels
#   cube4_steady1 normal one      0.49, 4.8e-13     0.0054   3.3e-16, 4.4e-16   20/20
#   cube4_steady3 normal one      0.0079, 1.2e-11   0.0043   6.7e-16, 6.7e-16   20/20   lambda_true / (1.1 vel_lmax) 0.966
#   cube4_transient normal one    0.37, 4.5e-11     0.0052   4.4e-16, 4.4e-16   19/20   3 levels
#   cube4_steady1 physical one    0.39, 4.7e-12     0.0025   5.6e-16, 6.7e-16   20/20
#   cube3_steady3 physical one    0.0047, 1.6e-11   0.0050   4.4e-16, 4.4e-16   19/20
#   cube3_transient physical one  0.25, 1.9e-11     0.0041   4.4e-16, 7.8e-16   20/20
#   the nine Taylor-Hood restart  <= 0.27, <= 1.9e-11   <= 0.0053   <= 8.9e-16, <= 8.9e-16   1/2 eight times, 2/2 once
#   cases
#   tri2d_transient normal one    0.0024, 1.7e-12   0.011    4.4e-16, 4.4e-16   19/20   2 levels
#   ld2 physical one              0.0075, 6.3e-14   0.0044   6.7e-16, 6.7e-16   20/20   (a) on the pressure rows and the dummy slot
#   ld2 normal restart(_guess)    <= 0.0087, <= 4.9e-14   <= 0.0074   <= 4.4e-16, <= 4.4e-16   1/2 twice
#   ld3 physical one              0.0040, 7.4e-12   0.0035   8.9e-16, 6.7e-16   20/20   3 levels, fp32 transfers
#   ld3 normal one                0.014, 4.0e-12    0.0082   8.9e-16, 7.8e-16   19/20
#   ld3 restart (both)            <= 0.0093, <= 3.2e-12   <= 0.0075   <= 6.7e-16, <= 6.7e-16   2/2 twice
#   cube16_transient normal large (not taken)       0.0080   8.9e-16, 8.9e-16   10/10   4 levels
# vel_lmax equals power_lmax bit for bit in the four cases with three sweeps (tolerance 4.9e-14 absolute).
# The gate over all cases: 296 iterations, 281 with the second pass (ratio hh^2 / ||w||^2 0.00 to 0.43), 15 without (0.58 to 0.96: the
# first iteration from a seeded right-hand side in the transient regime and of a restarted cycle, the second from the physical
# right-hand side with three sweeps), none borderline; the device's count equals the host's in every case.  (e): every defect of
# the device at or below ten times the host's own or under the floor of 64 eps scale, most of them below the host's.
# With the criterion the kernel had before (hh^2 > 0.1 ||w||^2; the same file with the threshold of (d) set to 0.1) (a), (b), (d) and (e)
# passed as above and (c) failed in 7 of the 20-iteration cases: |V^T V - I| 8.5e-13 to 7.7e-10 against 1000 L_ref = 4.4e-13 to 6.7e-13
# (6.6e-14 to 1.8e-13 in the three steady cases with one sweep that passed, 2.1e-14 after the 10 iterations of the large case), with 0 to 5 second passes in 20 iterations; the three
# converging runs lost 2.8e-8, 3.8e-13 and 1.3e-11, and the first stopped on a recurrence residual 3 % below the true one.  Hence
# eta^2 = 0.5 in k_sd_hess_pass.
# (The mistakes below and the run with the old criterion were made with the 19 cases and the seed search the file first had.)
# Converging runs (full GMRES on the edge-2 cube): steady1 seed 11 stops after 75 iterations at rtol 4.49e-9 (a factor 2.14 on both
# sides), steady3 seed 11 after 51 at 3.61e-7 (2.43), transient seed 24 after 53 at 2.47e-11 (2.04; seeds 11 to 23 offer at most
# 1.95); device and host agree in the count and in the residual to the digits printed.
# Three deliberate mistakes in scratch builds of fs_saddle.hip (the solve is now fs_saddle_solve.inc), each against this file and against tests/test_gpu_navier_stokes.py,
# test_gpu_navier_stokes_2d.py and test_gpu_large_deformation.py (55 tests):
#   rho_new * rho_new for rho_new * rho_c in the Mp     here: (a) in all 15 Taylor-Hood cases, 63 / 124 / 29 pressure rows outside the bound
#   Chebyshev of sd_precond                             (err / e_z 5.6e6 to 2.3e11); the 55 existing tests: all pass
#   k += 8 for k += 4 in k_sd_pressure_rows             here: (a) in the same 15 cases (err / e_z 2.4e10 to 3.5e12) and the three converging
#                                                       runs (77, 52, 58 iterations for 75, 51, 53); existing: 1 of 55 fails (the steady
#                                                       cavity, at its iteration ceiling)
#   H[j * m + k] not reset at pass == 0                 here: (b) in 16 of 19 cases (defect / bound 6e12 to 3e13; the three that pass run on a
#                                                       workspace whose H is still zero) and converged == 0 in the converging runs;
#                                                       existing: 32 of 55 fail (no convergence)
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp

import amg_reference as ar
import saddle_reference as sr
from spmv_reference import EPS, _host_product

pytestmark = pytest.mark.gpu
LD = np.longdouble
SEED = 11
_SYS, _RUNS = {}, {}

# (system, right-hand side, plan).  Plans: "one" = 20 iterations in one cycle; "restart" = restart 5, max_iter 12 (cycles of 5, 5, 2);
# "restart_guess" = the same from a non-zero guess; "large" = 10 iterations.
CASES = [
    ("cube3_steady1", "normal", "one"), ("cube3_steady3", "normal", "one"), ("cube3_transient", "normal", "one"),
    ("cube4_steady1", "normal", "one"), ("cube4_steady3", "normal", "one"), ("cube4_transient", "normal", "one"),
    ("cube4_steady1", "physical", "one"), ("cube3_steady3", "physical", "one"), ("cube3_transient", "physical", "one"),
    ("cube3_steady1", "normal", "restart"), ("cube4_steady3", "normal", "restart_guess"), ("cube4_transient", "physical", "restart"),
    ("cube3_transient", "normal", "restart_guess"), ("cube3_steady1", "physical", "restart_guess"), ("cube3_steady3", "normal", "restart"),
    ("cube3_steady3", "physical", "restart_guess"), ("cube3_transient", "physical", "restart"),
    ("tri2d_transient", "normal", "one"), ("tri2d_transient", "physical", "restart_guess"),
    ("ld2", "physical", "one"), ("ld2", "normal", "restart_guess"), ("ld2", "normal", "restart"),
    ("ld3", "physical", "one"), ("ld3", "normal", "one"), ("ld3", "normal", "restart_guess"), ("ld3", "physical", "restart"),
    ("cube16_transient", "normal", "large"),
]
PLANS = {"one": dict(max_iter=20, restart=0), "restart": dict(max_iter=12, restart=5), "restart_guess": dict(max_iter=12, restart=5),
         "large": dict(max_iter=10, restart=12)}


def _csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


def _hierarchy(amg):
    """(levels for vcycle_replay, the dense coarse inverse or None) from the inspection hooks, as amg_vcycle_worker.py reads them."""
    fp32 = os.environ.get("FS_AMG_FP32", "1")[:1] != "0"
    node_waves = "FS_AMG_NO_NODE_WAVES" not in os.environ
    n_levels = amg.info()["levels"]
    levels = []
    for l in range(n_levels):
        li = amg.level_info(l)
        P = amg.level_matrix(l, "P") if l + 1 < n_levels else None
        levels.append({"A": amg.level_matrix(l, "A"), "P": P, "lmax": li["lambda_max"],
                       "a32": l > 0 and ar.operator_is_fp32(li["block_size"], li["nnz_blocks"], li["n_nodes"], fp32, node_waves),
                       "p32": P is not None and ar.transfers_are_fp32(li["block_size"], li["p_block_cols"], fp32)})
    return ar.prepare(levels), amg.coarse_inverse()


def _taylor_hood(gpu, dim, n, inv_dt, nu, sweeps):
    """One linearised step of the lid-driven cavity, pressure pinned at vertex 0 (test_saddle_solve_lid_driven_cavity_step and its
    2-D twin): every wall velocity held, the lid moving."""
    if dim == 3:
        from test_gpu_navier_stokes import _pressure_operators, _setup
        co, ce, th, mesh, W, Q = _setup(gpu, n)
    else:
        from test_gpu_navier_stokes_2d import _pressure_operators, _setup
        co, ce, th, mesh, W, Q = _setup(gpu)
    X = th.node_coords
    bn = th.boundary_nodes(lambda x: True)
    lid = bn[X[bn, dim - 1] == X[:, dim - 1].max()]
    vals = np.zeros((th.n_nodes, 4))
    vals[lid, 0] = 1.0
    bc_dofs = np.concatenate([th.velocity_dofs(bn), th.pressure_dofs([0])])
    bc_vals = vals.ravel()[bc_dofs]
    w0 = np.zeros(th.n)
    w0[bc_dofs] = bc_vals
    J = gpu.DeviceMatrix(W)
    g = gpu.DeviceVector(W.n_owned)
    gpu.assemble_navier_stokes(J, g, gpu.DeviceVector(W.n_local, w0), gpu.DeviceVector(W.n_local, np.zeros(th.n)), nu=nu, rho=1.0,
                               inv_dt=inv_dt)
    J.apply_dirichlet(g, bc_dofs.astype(np.int32), bc_vals, symmetric=False)
    Kp, Mp = _pressure_operators(gpu, Q, [0])
    S = {"kind": "th", "J": J, "Jc": _csr(J), "Mp": Mp, "Mpc": _csr(Mp), "n": th.n, "nv": th.nv, "b_phys": g.get()[:th.n].copy(),
         "dummy": th.dummy_dofs(), "sweeps": sweeps, "keep": (mesh, W, Q, Kp)}
    opts = {"nu": nu, "rho": 1.0, "inv_dt": inv_dt, "velocity_sweeps": sweeps, "nv": th.nv}
    amg, levels = None, None
    if inv_dt:
        amg = gpu.AMG(Kp, coarse_size=10)           # (64 and 125 vertices: a single level otherwise)
        levels, opts["coarse"] = _hierarchy(amg)
        S["levels"] = len(levels)
    S["opts"] = opts

    def solve(b, x, **kw):
        return gpu.saddle_solve(J, Kp if inv_dt else None, Mp, b, x, nu=nu, rho=1.0, inv_dt=inv_dt, velocity_sweeps=sweeps,
                                Kp_amg=amg, **kw)

    def replay(r, vel_lmax):
        return sr.cahouet_chabard_replay(S["Jc"], S["Mpc"], levels, dict(opts, vel_lmax=vel_lmax), r)
    S["solve"], S["replay"] = solve, replay
    return S


def _large_deformation(gpu, d):
    """The reduced Newton system of test_gpu_large_deformation.py's random case with the velocity operator, its hierarchy and the
    Schur scale as LargeDeformationSolver forms them.  2-D: fs_amg_setup takes no blocks of 2, the velocity solve is the inner
    Jacobi-CG to 1e-2, which is no fixed operator: the replay covers the pressure rows and the dummy slot, S["rows"]."""
    from test_gpu_large_deformation import _Dev, _random_case
    mesh, P, x, x0, mask, dofs, fl, g = _random_case(d, 20 + d)
    dev = _Dev(mesh)
    Jc, rhs, _ = dev.assemble(P, x, x0, mask, fl, g)
    Q = gpu.DeviceSpace(dev.W4.mesh, 1, 1)
    Mp = gpu.DeviceMatrix(Q)
    Mp.assemble(mass=1.0)
    A0 = gpu.DeviceMatrix(dev.V.device())
    A0.assemble(lame=(P.q * P.q * P.dt * P.mu, 0.0), mass=1.0 / P.dt)
    left = np.nonzero(mesh.coordinates()[:, 0] == 0.0)[0]
    vdofs = np.sort((left[:, None] * d + np.arange(d)).ravel()).astype(np.int32)
    A0.apply_dirichlet(None, vdofs, 0.0, symmetric=True)
    amg, levels, cinv = None, [], None
    if d == 3:
        amg = gpu.AMG(A0, nullspace="rigid_body", coarse_size=10)
        levels, cinv = _hierarchy(amg)
    schur = P.q * (1.0 / P.lmbda + 1.0 / P.mu)
    n = 4 * dev.nv
    S = {"kind": "ld", "J": dev.J, "Jc": Jc, "Mp": Mp, "Mpc": _csr(Mp), "n": n, "nv": dev.nv, "b_phys": rhs.copy(),
         "dummy": np.arange(dev.nv) * 4 + 2 if d == 2 else np.zeros(0, dtype=np.int64), "sweeps": 1, "keep": (dev, Q, A0, amg),
         "levels": len(levels), "rows": None if d == 3 else np.flatnonzero((np.arange(n) & 3) >= 2)}
    opts = {"schur_scale": schur, "tdim": d, "coarse": cinv}

    def solve(b, x, **kw):
        return gpu.large_deformation_solve(dev.J, Mp, b, x, A0, schur, a0_amg=amg, **kw)

    def replay(r, vel_lmax):
        return sr.block_upper_replay(S["Jc"], S["Mpc"], levels if d == 3 else None, opts, r)
    S["solve"], S["replay"] = solve, replay
    return S


def _system(gpu, name):
    if name not in _SYS:
        if name.startswith("ld"):
            _SYS[name] = _large_deformation(gpu, int(name[2]))
        else:
            geo, mode = name.split("_")
            inv_dt, nu = (100.0, 0.01) if mode == "transient" else (0.0, 0.1)
            sweeps = 3 if mode == "steady3" else 1
            _SYS[name] = _taylor_hood(gpu, 2 if geo == "tri2d" else 3, int(geo[4:]) if geo != "tri2d" else 0, inv_dt, nu, sweeps)
    return _SYS[name]


def _rhs(S, what, seed=SEED):
    if what == "physical":
        return S["b_phys"].copy()
    b = np.random.default_rng(seed).standard_normal(S["n"])
    b[S["dummy"]] = 0.0
    return b


def _products(S, Z, extended):
    """(J Z_j, its row bound) per column: extended-precision row sums rounded once, or scipy's float64."""
    Jc = S["Jc"]
    terms = np.diff(Jc.indptr)
    if extended:
        pairs = [_host_product(Jc, z) for z in Z]
        return np.array([p[0] for p in pairs]), np.array([terms * EPS * p[1] for p in pairs])
    absJ = abs(Jc)
    return np.array([Jc @ z for z in Z]), np.array([2.0 * terms * EPS * (absJ @ np.abs(z)) for z in Z])


def _defects(S, JZ, b, x, gam):
    """(| g - ||b - J x|| |, ||(J Z)^T (b - J x)||_inf) of a solution x with its recurrence residual g."""
    r = b - S["Jc"] @ x
    return abs(gam - float(np.linalg.norm(r))), float(np.abs(JZ @ r).max())


def _run(gpu, sysname, what, plan):
    key = (sysname, what, plan)
    if key in _RUNS:
        return _RUNS[key]
    t0 = time.time()
    S = _system(gpu, sysname)
    n, Jc = S["n"], S["Jc"]
    full = plan != "large"                      # products in extended precision
    b = _rhs(S, what)
    x0 = np.zeros(n)
    if plan == "restart_guess":
        x0 = 0.1 * np.random.default_rng(SEED + 100).standard_normal(n)
        x0[S["dummy"]] = 0.0
    bd, xd = gpu.DeviceVector(n, b), gpu.DeviceVector(n, x0)
    kw = PLANS[plan]
    st = S["solve"](bd, xd, rtol=0.0, atol=0.0, nonzero_guess=plan == "restart_guess", **kw)
    c = gpu.saddle_last_cycle()
    x = xd.get()[:n]
    for h in (bd, xd):
        h.close()
    assert c is not None
    m, k = c["m"], c["kuse"]
    V, Z = c["V"], c["Z"]
    bnorm = float(np.linalg.norm(b))
    F = {"case": key, "n": n, "kuse": k, "stats": st}
    assert m == (kw["restart"] or 60) and k == (kw["max_iter"] if kw["max_iter"] <= m else kw["max_iter"] % m), (m, k)
    assert np.all(np.isfinite(V)) and np.all(np.isfinite(Z)) and np.all(np.isfinite(x))
    # (a) the preconditioner, column by column on the device's own V_j
    if full:
        fig = [sr.check_inside(Z[j], *S["replay"](V[j], c["vel_lmax"]), (key, "Z", j), S.get("rows")) for j in range(k)]
        F["a_ratio"], F["a_tight"] = max(f[0] for f in fig), max(f[1] for f in fig)
        if S["sweeps"] > 1:
            lm, lm64 = sr.power_lmax(Jc), sr.power_lmax(Jc, extended=False)
            F["lmax_err"], F["lmax_tol"] = abs(c["vel_lmax"] - lm), 100.0 * max(abs(lm - lm64), EPS * lm)
            if "lam_true" not in S:
                S["lam_true"] = sr.velocity_lambda_true(Jc)
            F["lam_ratio"] = S["lam_true"] / (1.1 * c["vel_lmax"])
    # (b) the Arnoldi relation
    JZ, row = _products(S, Z, full)
    Hbar = sr.hessenberg_from_rotations(c["R"], c["cs"], c["sn"], k)
    vinf = np.abs(V).max(axis=1)
    VL = V.astype(LD)
    F["b_ratio"] = 0.0
    for j in range(k):
        defect = np.abs((JZ[j].astype(LD) - Hbar[:j + 2, j].astype(LD) @ VL[:j + 2]).astype(np.float64))
        bound = 64.0 * (j + 2) * EPS * float(np.abs(Hbar[:j + 2, j]) @ vinf[:j + 2]) + row[j]
        F["b_ratio"] = max(F["b_ratio"], float((defect / bound).max()))
    # (c) orthogonality against two full passes on the host
    F["c_loss"] = sr.orthogonality_loss(V)
    F["c_ref"] = sr.orthogonality_loss(sr.two_pass_arnoldi(JZ, V[0]))
    # (d) the gate, from the device's V and the host's J Z
    ratios = []
    for j in range(k):
        before = float(JZ[j] @ JZ[j])
        h1 = V[:j + 1] @ JZ[j]
        ratios.append((before - float(h1 @ h1)) / before)
    ratios = np.array(ratios)
    border = np.abs(ratios - sr.GATE) <= 0.05 * sr.GATE
    F["d_sure"], F["d_border"] = int(((ratios <= sr.GATE) & ~border).sum()), int(border.sum())
    F["d_without"], F["d_passes"], F["d_ratios"] = int(((ratios > sr.GATE) & ~border).sum()), c["second_passes"], ratios
    # (e) recurrence, update and stop.  x0 of the LAST cycle is x - Z y; the cycle started from b - J x0 = beta V_0
    y_dev = c["y"][:k]
    x0c = (x.astype(LD) - y_dev.astype(LD) @ Z.astype(LD)).astype(np.float64)
    if plan in ("one", "large"):            # a single cycle: its x0 is the caller's
        F["e_x0"], F["e_x0_floor"] = float(np.abs(x0c - x0).max()), 64 * EPS * float(np.abs(y_dev) @ np.abs(Z).max(axis=1))
        x0c = x0
    r0 = b - Jc @ x0c
    beta = float(np.linalg.norm(r0))
    absJ = abs(Jc)
    terms = np.diff(Jc.indptr)
    F["e_v0"] = float(np.abs(r0 - beta * V[0]).max())
    F["e_v0_bound"] = float(((terms + 4) * EPS * (absJ @ np.abs(x0c) + np.abs(b)) + 4.0 * EPS * beta * np.abs(V[0])).max()) + 64 * EPS * beta * vinf[0]
    y_ls, res_ls = sr.least_squares(Hbar, beta)
    x_h = x0c + y_ls @ Z
    zsum = float(np.abs(y_ls) @ np.abs(Z).max(axis=1))
    scale_r = beta * float(np.linalg.norm(JZ))
    F["e_dev"] = _defects(S, JZ, b, x, abs(c["gamma"][k]))
    F["e_host"] = _defects(S, JZ, b, x_h, res_ls)
    F["e_floor"] = (64 * EPS * beta, 64 * EPS * scale_r)
    # (y of a backward-stable least-squares solve is within cond(Hbar) eps of y_ls; x0c and x_h each round at the size of x)
    F["e_x"], F["e_x_floor"] = float(np.abs(x - x_h).max()), 64 * EPS * (float(np.linalg.cond(Hbar)) * zsum + float(np.abs(x).max()))
    rtrue = b - Jc @ x
    F["e_rel"] = float(np.linalg.norm(rtrue)) / bnorm
    F["e_rel_tol"] = float(np.linalg.norm((terms + 2) * EPS * (absJ @ np.abs(x) + np.abs(b)))) / bnorm + 4 * EPS * F["e_rel"]
    F["seconds"] = time.time() - t0             # (reported, not asserted: the first case of a system pays for its set-up)
    print("figures", sysname, what, plan, {a: (("%.3g" % v) if isinstance(v, float) else v) for a, v in F.items()
                                            if a not in ("case", "stats", "d_ratios")},
          "ratios", np.round(ratios, 3).tolist(), "levels", S.get("levels"))
    _RUNS[key] = F
    return F


@pytest.mark.parametrize("sysname,what,plan", CASES, ids=["-".join(c) for c in CASES])
def test_last_cycle_is_the_replay(gpu, sysname, what, plan):
    F = _run(gpu, sysname, what, plan)
    st, kw = F["stats"], PLANS[plan]
    if "a_ratio" in F:
        assert F["a_ratio"] <= 1.0
        assert F["a_tight"] <= sr.TIGHT, "the replay's bound has grown loose: replace the case"
        if "lmax_err" in F:
            assert F["lmax_err"] <= F["lmax_tol"], (F["lmax_err"], F["lmax_tol"])
            assert F["lam_ratio"] <= 1.0, F["lam_ratio"]
    assert F["b_ratio"] <= 1.0, F["b_ratio"]
    assert F["c_loss"] <= 1000.0 * F["c_ref"], (F["c_loss"], F["c_ref"])
    assert F["d_sure"] <= F["d_passes"] <= F["d_sure"] + F["d_border"], (F["d_sure"], F["d_border"], F["d_passes"], F["d_ratios"])
    assert F["e_v0"] <= F["e_v0_bound"], (F["e_v0"], F["e_v0_bound"])
    if "e_x0" in F:
        assert F["e_x0"] <= F["e_x0_floor"], (F["e_x0"], F["e_x0_floor"])
    for dev, host, floor in zip(F["e_dev"], F["e_host"], F["e_floor"]):
        assert dev <= max(10.0 * host, floor), (F["e_dev"], F["e_host"], F["e_floor"])
    assert F["e_x"] <= F["e_x_floor"], (F["e_x"], F["e_x_floor"])
    assert st["iterations"] == kw["max_iter"] and st["converged"] == 0, st
    assert abs(st["rel_residual"] - F["e_rel"]) <= F["e_rel_tol"], (st["rel_residual"], F["e_rel"], F["e_rel_tol"])


def test_both_sides_of_the_gate_ran(gpu):
    """The coverage conditions over all cases: iterations with and without the second pass, few borderline ones."""
    F = [_run(gpu, *c) for c in CASES]
    total = sum(f["kuse"] for f in F)
    with_pass, without, border = sum(f["d_sure"] for f in F), sum(f["d_without"] for f in F), sum(f["d_border"] for f in F)
    print("iterations", total, "with the second pass", with_pass, "without", without, "borderline", border,
          "device passes", sum(f["d_passes"] for f in F))
    assert with_pass >= 1 and without >= 1
    assert border <= 0.1 * total
    assert any(f["kuse"] + 2 > 16 for f in F) and any(f["n"] > 512 * 256 for f in F)


def test_no_cycle_no_state(gpu):
    """A call that stops on its first residual ran no cycle: the hook says so instead of handing out the state of an earlier call."""
    S = _system(gpu, "cube3_steady1")
    _run(gpu, "cube3_steady1", "normal", "restart")
    bd, xd = gpu.DeviceVector(S["n"], _rhs(S, "normal")), gpu.DeviceVector(S["n"], np.zeros(S["n"]))
    st = S["solve"](bd, xd, rtol=0.0, atol=1e300, max_iter=12, restart=5)
    assert st["converged"] == 1 and st["iterations"] == 0
    assert gpu.saddle_last_cycle() is None
    for h in (bd, xd):
        h.close()


# the right-hand side seeds of the converging runs: the first from SEED whose host history has a single-iteration drop by a factor 4.
# (No block_upper run: ld3 converges in 34 iterations without such a drop - the seeds 11 to 50 offer a margin of 1.87 at most.)
CONVERGING = {"cube2_steady1": 11, "cube2_steady3": 11, "cube2_transient": 24}


def _stopping_point(S, seed):
    """(b, index i of the host history before the largest drop between 1e-5 and 1e-11, rtol in its geometric middle, the margin
    on both sides, the history, the host run)."""
    vel_lmax = sr.power_lmax(S["Jc"]) if S["sweeps"] > 1 else 0.0
    b = _rhs(S, "normal", seed)
    host = sr.host_fgmres(S["Jc"], lambda r: S["replay"](r, vel_lmax)[0], b, restart=100, max_iter=100, rtol=1e-12)
    h = np.array(host["history"]) / float(np.linalg.norm(b))
    window = np.flatnonzero((h[:-1] <= 1e-5) & (h[1:] >= 1e-11))
    i = int(window[np.argmax(h[window] / h[window + 1])])
    return b, i, float(np.sqrt(h[i] * h[i + 1])), float(np.sqrt(h[i] / h[i + 1])), h, host


@pytest.mark.parametrize("name", list(CONVERGING))
def test_converging_run_counts_the_hosts_iterations(gpu, name):
    """The smallest cube, full GMRES (restart 100 > the iterations needed): the residual history has its
    large single-iteration drops near the end.  rtol sits in the geometric middle of the largest drop of the host's history between
    1e-5 and 1e-11, which has to be a factor 4 (2 on both sides of the threshold)."""
    S = _system(gpu, name)
    n, Jc, seed = S["n"], S["Jc"], CONVERGING[name]
    b, i, rtol, margin, h, host = _stopping_point(S, seed)
    bnorm = float(np.linalg.norm(b))
    print(name, "seed", seed, "host iterations to 1e-12", host["iterations"], "stop after", i + 2, "rtol %.2e" % rtol, "margin %.2f" % margin,
          "host loss %.1e" % max(host["loss"]))
    assert margin >= 2.0, "no drop by a factor 4 in the host's history: choose another seed"
    bd, xd = gpu.DeviceVector(n, b), gpu.DeviceVector(n, np.zeros(n))
    st = S["solve"](bd, xd, rtol=rtol, atol=0.0, max_iter=100, restart=100)
    x = xd.get()[:n]
    c = gpu.saddle_last_cycle()
    for d in (bd, xd):
        d.close()
    true = float(np.linalg.norm(b - Jc @ x))
    # (the iteration enqueued ahead of the stopping test has rotated gamma[kuse] on into gamma[kuse + 1]: the norm of the two is it)
    rec = float(np.hypot(c["gamma"][c["kuse"]], c["gamma"][c["kuse"] + 1])) if c["kuse"] < c["m"] else abs(c["gamma"][c["kuse"]])
    print(name, "device", st["iterations"], "true residual / ||b|| %.3e" % (true / bnorm), "recurrence %.3e" % (rec / bnorm),
          "host %.3e" % h[i + 1], "loss %.1e" % sr.orthogonality_loss(c["V"]))
    assert st["converged"] == 1 and true <= rtol * bnorm
    assert st["iterations"] == i + 2 == c["kuse"], (st["iterations"], i + 2, c["kuse"])
    tol = float(np.linalg.norm((np.diff(Jc.indptr) + 2) * EPS * (abs(Jc) @ np.abs(x) + np.abs(b)))) / bnorm
    # the recurrence residual the cycle stopped on is the residual, to the rounding of b - J x and of the update (floor as in (e))
    assert abs(rec - true) <= tol * bnorm + 64 * EPS * bnorm, (rec, true, tol * bnorm)
    assert abs(st["rel_residual"] - true / bnorm) <= tol, (st["rel_residual"], true / bnorm, tol)
