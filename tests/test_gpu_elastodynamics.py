"""ElastodynamicsSolver and the fs_dyn_* kernels on the MI355X: the kernels against numpy row by row, the solver against the reference
marcher (tests/elastodynamics_reference.py) step by step, single modes against their closed form, the energy identities of the
trapezoidal rule, the build discipline, determinism and restart, and the refusals of the library."""
import copy
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import elastodynamics_reference as er

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E_, NU_, RHO_ = 200.0, 0.3, 1.0
MU_, LM_ = E_ / (2 * (1 + NU_)), E_ * NU_ / ((1 + NU_) * (1 - 2 * NU_))

ROW_TOL = 32 * 2.0 ** -53       # set by the issue: per row |device - numpy| <= 32 x 2^-53 x (sum of the absolute terms of that row)
ENERGY_TOL = 1e-12              # set by the issue: fs_dyn_energy against numpy with the device's u, v, relative

# Measured on the MI355X (this file: the tests print every figure before they assert), every solver test with the Krylov tolerance at
# 1e-12 ('krylov_relative_tolerance'), as GPU minus reference relative to the largest entry of the reference field at that step, and
# the bounds derived from them: 10 x the measured difference, since the residue the stopping test leaves belongs to the mesh family,
# not to one mesh.  The acceleration carries the 1 / (beta dt^2) of the Newmark update and has a bound of its own.
# Solver against the reference marcher, eight steps, largest over the steps as (u, v, a, traces), with the CG iterations per step:
#   cantilever 8 x 3 x 3 (AMG-CG, 29 - 31)     1.44e-11  8.65e-12  4.88e-12  5.95e-12
#   rectangle 16 x 8 (Jacobi-CG, 100 - 102)    4.27e-12  1.59e-11  1.98e-11  2.02e-12
#   CG2 4 x 2 x 2 (AMG-CG, 22 - 23)            6.56e-12  2.03e-11  2.32e-11  5.47e-12
#   per-region E and density (26 - 28)         5.26e-12  5.76e-12  4.55e-12  3.07e-12
#   tests/golden/data/mesh.xml (12 - 13)       5.02e-12  1.09e-11  9.46e-12  1.10e-12
MARCH_MEASURED = {"u": 1.44e-11, "v": 2.03e-11, "a": 2.32e-11, "traces": 5.95e-12}
MARCH_TOL = {k: 10 * v for k, v in MARCH_MEASURED.items()}
# Single mode over 12 steps of 0.2 / omega, relative to max |phi|.  rho_inf = 1 against phi cos(omega_h n dt): cantilever mode 0
# 6.79e-13, mode 7 1.37e-12, rectangle mode 2 3.84e-12.  Damped, rho_inf = 0.6, against the scalar recursion (u, v, a, each relative to
# its largest modal value): 4.42e-11, 1.12e-10, 6.85e-11.
MODE_MEASURED = 3.84e-12
MODE_TOL = 10 * MODE_MEASURED
MODE_DAMPED_MEASURED = 1.12e-10
MODE_DAMPED_TOL = 10 * MODE_DAMPED_MEASURED
# Energy of the trapezoidal rule over 40 steps, relative to E_0: drift undamped and unloaded 3.77e-12 (cantilever), 7.01e-12
# (rectangle); damped, the defect of E_{n+1} - E_n = -dt vbar^T C vbar 1.15e-12, 5.16e-13 - held to the same bound.
ENERGY_DRIFT_MEASURED = 7.01e-12
ENERGY_DRIFT_TOL = 10 * ENERGY_DRIFT_MEASURED
# Kernels against numpy, largest row figure in units of 2^-53 (the issue's bound is 32): 81 dofs 3.4, 375 dofs 3.3, rectangle 2.7,
# CG2 3.3, 273 375 dofs 5.2; fs_dyn_energy against numpy 2.5e-16 or better (the issue's bound is 1e-12).

# ---- 1. the kernels against numpy ------------------------------------------------------------------------------------------------
def _space(shape):
    """(device space, dimension) of a shape of the issue's list"""
    from fenicssolver_amd import backend
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace
    backend.init()
    kind, n = shape
    if kind == "box":
        mesh = backend.DeviceMesh.box(n, n, n)
        return backend.DeviceSpace(mesh, 3, 1), 3, mesh
    if kind == "rect":
        V = VectorFunctionSpace(RectangleMesh(Point(0, 0), Point(1.0, 0.7), 6, 5), "Lagrange", 1)
        return V.device(), 2, V
    V = VectorFunctionSpace(BoxMesh(Point(0, 0, 0), Point(1, 1, 1), n, n, n), "Lagrange", 2)
    return V.device(), 3, V


def _host_csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


SHAPES = [("box", 2), ("box", 4), ("rect", 0), ("cg2", 2), ("box", 44)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s%d" % s)
def test_kernels_match_numpy_row_by_row(shape):
    from fenicssolver_amd import backend
    dV, d, keep = _space(shape)
    n = dV.n_owned
    assert shape != ("box", 2) or n == 81
    assert shape != ("box", 4) or n == 375
    assert shape != ("box", 44) or (n == 273375 and n > 1024 * 256)         # the grid-stride loop makes a second trip
    K, M = backend.DeviceMatrix(dV), backend.DeviceMatrix(dV)
    K.assemble(lame=(MU_, LM_))
    M.assemble(lame=(0.0, 0.0), mass=RHO_)
    rng = np.random.default_rng(100 + n)
    u, v, a, F, xs = (rng.standard_normal(n) * s for s in (1e-2, 1e-1, 1.0, 0.5, 1e-2))
    # Dirichlet dofs, some named twice (the last value holds), receivers on a Dirichlet dof, on a free one and one named twice
    dd = rng.choice(n, size=max(n // 9, 4), replace=False).astype(np.int32)
    dofs = np.concatenate([dd, dd[:3]])
    vals = rng.standard_normal(len(dofs))
    g = np.zeros(n)
    is_d = np.zeros(n, dtype=bool)
    for i, val in zip(dofs, vals):
        g[i], is_d[i] = val, True
    free = np.nonzero(~is_d)[0]
    rec = np.array([dd[0], free[0], free[-1], dd[1], free[0], n - 1], dtype=np.int32)
    eta_m, eta_k, dt, sf, sg = 0.3, 0.02, 0.05, 0.7, -1.3
    st = backend.DynamicsState(dV)
    rhs, x = backend.DeviceVector(dV.n_owned), backend.DeviceVector(dV.n_local, xs)
    pd_, qd_, yd_ = backend.DeviceVector(dV.n_local), backend.DeviceVector(dV.n_local), backend.DeviceVector(dV.n_owned)
    Kh = Mh = None
    for rho_inf in (0.0, 0.5, 1.0):
        am, af, beta, gamma = er.parameters(rho_inf)
        st.configure(dt, am, af, beta, gamma, eta_m, eta_k, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)
        st.set(u, v, a, step=3)
        st.predict(K, M, sf, sg, rhs)
        p, q, mp, kq = st.work()
        # numpy, term by term, with the sum of the absolute terms of every row beside it
        cm = (1 - am) / (beta * dt * dt) + (1 - af) * gamma * eta_m / (beta * dt)
        ck = (1 - af) * (1 + gamma * eta_k / (beta * dt))
        ut, s_ut = u + dt * v + dt * dt * (0.5 - beta) * a, np.abs(u) + np.abs(dt * v) + np.abs(dt * dt * (0.5 - beta) * a)
        vt, s_vt = v + dt * (1 - gamma) * a, np.abs(v) + np.abs(dt * (1 - gamma) * a)
        gb = gamma / (beta * dt)
        cv, s_cv = (1 - af) * (vt - gb * ut) + af * v, abs(1 - af) * (s_vt + gb * s_ut) + np.abs(af * v)
        gext = np.where(is_d, g * sg, 0.0)
        um = (1 - am) / (beta * dt * dt)
        p_ref, s_p = um * ut - am * a - eta_m * cv - cm * gext, um * s_ut + np.abs(am * a) + eta_m * s_cv + np.abs(cm * gext)
        q_ref, s_q = -af * u - eta_k * cv - ck * gext, np.abs(af * u) + eta_k * s_cv + np.abs(ck * gext)
        figs = {"p": (np.abs(p - p_ref) / s_p).max(), "q": (np.abs(q - q_ref) / s_q).max()}
        # the products enter through the device's own fs_spmv result
        pd_.set(p)
        M.spmv(pd_, yd_)
        assert np.array_equal(yd_.get(), mp)
        qd_.set(q)
        K.spmv(qd_, yd_)
        assert np.array_equal(yd_.get(), kq)
        r_ref, s_r = np.where(is_d, g * sg, sf * F + mp + kq), np.where(is_d, np.abs(g * sg), np.abs(sf * F) + np.abs(mp) + np.abs(kq))
        r = rhs.get()
        figs["rhs"] = (np.abs(r - r_ref) / np.maximum(s_r, 1e-300)).max()
        samples = st.correct(x, rec)
        u1, v1, a1, step = st.get()
        ib = 1.0 / (beta * dt * dt)
        a_ref, s_a = (xs - ut) * ib, (np.abs(xs) + s_ut) * ib
        v_ref, s_v = vt + gamma * dt * a_ref, s_vt + gamma * dt * s_a
        figs["a"], figs["v"] = (np.abs(a1 - a_ref) / s_a).max(), (np.abs(v1 - v_ref) / s_v).max()
        print("\n%s%d rho_inf = %g: largest |device - numpy| / (sum of absolute terms) per row, in units of 2^-53: %s" % (
            shape + (rho_inf, {k: "%.2f" % (f * 2.0 ** 53) for k, f in figs.items()})))
        assert step == 4 and np.array_equal(u1, xs) and np.array_equal(samples, xs[rec])
        assert st.info()["n_nonfinite"] == 0 and st.info()["first_nonfinite_step"] == -1
        assert max(figs.values()) <= ROW_TOL
        # energy against numpy with the device's u, v
        if Kh is None:
            Kh, Mh = _host_csr(K), _host_csr(M)
        ek, ep = st.energy(K, M)
        ek_ref, ep_ref = er.energy(Kh, Mh, u1, v1)
        print("energy: relative difference (kinetic, potential) %.2e %.2e" % (abs(ek - ek_ref) / ek_ref, abs(ep - ep_ref) / ep_ref))
        assert abs(ek - ek_ref) <= ENERGY_TOL * ek_ref and abs(ep - ep_ref) <= ENERGY_TOL * ep_ref
        assert st.energy(K, M) == (ek, ep)                                  # a fixed order of summation
    # a non-finite solution is counted, and the step that had it is named
    xs_bad = xs.copy()
    xs_bad[[1, n - 2]] = np.nan, np.inf
    x.set(xs_bad)
    st.correct(x)
    info = st.info()
    assert info["n_nonfinite"] == 2 and info["first_nonfinite_step"] == 5 and info["step"] == 5


def test_the_receiver_list_may_change_from_call_to_call_on_one_state():
    """The receiver bits of the device flags follow the list of the call; a bit that is not set leaves its slot of the sample buffer
    unwritten.  Exact: a sample of correct() is the entry of x itself."""
    from fenicssolver_amd import backend
    dV, d, keep = _space(("box", 2))
    n = dV.n_owned
    assert n == 81
    rng = np.random.default_rng(25)
    u, v, a, F = (rng.standard_normal(n) * s for s in (1e-2, 1e-1, 1.0, 0.5))
    dofs, vals = np.array([0, 1, 2, 30, 31], dtype=np.int32), 0.01 * np.arange(1.0, 6.0)
    A = np.array([5, 30, 80], dtype=np.int32)                              # one of them a Dirichlet dof
    B = np.array([7, 1, 44], dtype=np.int32)                               # disjoint from A
    C = np.array([80, 80], dtype=np.int32)                                 # shorter, a dof of A, named twice
    par = (0.05,) + tuple(er.parameters(0.5)) + (0.3, 0.02)
    st = backend.DynamicsState(dV)
    st.configure(*par, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)
    st.set(u, v, a, step=0)
    x = backend.DeviceVector(dV.n_local)

    def step_with(rec, k):
        x.set(rng.standard_normal(n) * 1e-2)
        samples = st.correct(x, rec)
        uu, _, _, step = st.get()
        assert step == k
        if rec is None:
            assert samples is None
        else:
            assert samples.shape == (len(rec),) and np.array_equal(samples, uu[rec]), (k, rec)
    for k, rec in enumerate((A, B, C, None, A), start=1):
        step_with(rec, k)
    uu, vv, aa, step = st.get()
    st.configure(*par, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)     # the flags are uploaded anew, without receiver bits
    st.set(uu, vv, aa, step)
    step_with(B, 6)
    assert st.info()["n_nonfinite"] == 0
    st.close()


def test_start_forms_the_initial_residual_and_takes_the_acceleration():
    from fenicssolver_amd import backend
    dV, d, keep = _space(("box", 3))
    n = dV.n_owned
    K, M = backend.DeviceMatrix(dV), backend.DeviceMatrix(dV)
    K.assemble(lame=(MU_, LM_))
    M.assemble(lame=(0.0, 0.0), mass=RHO_)
    Kh, Mh = _host_csr(K), _host_csr(M)
    rng = np.random.default_rng(8)
    u0, v0, F, a0 = (rng.standard_normal(n) for _ in range(4))
    dofs = np.arange(0, 12, dtype=np.int32)
    st = backend.DynamicsState(dV)
    st.configure(0.1, *er.parameters(0.8), 0.3, 0.02, load=F, dirichlet_dofs=dofs, dirichlet_values=np.ones(12))
    rhs = backend.DeviceVector(n)
    st.start_rhs(K, M, u0, v0, 0.6, rhs)
    ref = 0.6 * F - 0.3 * (Mh @ v0) - Kh @ (u0 + 0.02 * v0)
    ref[dofs] = 0.0
    scale = np.abs(0.6 * F) + np.abs(0.3 * (Mh @ v0)) + np.abs(Kh) @ np.abs(u0 + 0.02 * v0)
    r = rhs.get()
    assert not r[dofs].any()
    # (the two products sum some 40 terms per row in the device's own order: n_row x 2^-53 per row, 64 terms at the most)
    assert (np.abs(r - ref) / scale).max() <= 64 * 2.0 ** -53
    with pytest.raises(backend.BackendError, match="holds no"):
        st.predict(K, M, 1.0, 1.0, rhs)                                    # started only once a_0 is in
    st.start(backend.DeviceVector(n, a0))
    u, v, a, step = st.get()
    a0[dofs] = 0.0
    assert step == 0 and np.array_equal(u, u0) and np.array_equal(v, v0) and np.array_equal(a, a0)


# ---- the cases of the solver tests -----------------------------------------------------------------------------------------------
DT, STEPS = 0.05, 8
RICKER = {'type': 'ricker', 'frequency': 2.5, 'delay': 0.2}


def _face_motion(t):
    return math.sin(8.0 * t)


def _xml_mesh():
    from fenicssolver_amd.fem import Mesh
    return Mesh(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "mesh.xml"))


def _case(kind, dynamics=None, steps=STEPS, dt=DT, loaded=True, moving=True, times=None, receivers=True, krylov=1e-12):
    """cantilever / regions: a 4 x 1 x 1 box of 8 x 3 x 3 cells whose face x = 0 moves by 0.01 sin(8 t) in z, under a Ricker end traction
    on x = 4 (regions: E and the density differ between x < 2 and beyond); cg2: the same box, 4 x 2 x 2 cells, CG2; rectangle: 2 x 1 in
    plane strain, 16 x 8 cells, the edge y = 0 moving in x, a Ricker traction on part of the top edge; xml: tests/golden/data/mesh.xml
    (a 10 x 5 x 20 block) in file order, the face z = 0 moving in x, sheared at z = 20."""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, MeshFunction, near
    from fenicssolver_amd import SolverBase as SB
    bcs = OrderedDict()
    amp = 0.01 if moving else 0.0
    tf = {'time_function': _face_motion} if moving else {}
    if kind in ("cantilever", "regions", "cg2"):
        mesh = BoxMesh(Point(0, 0, 0), Point(4, 1, 1), *((4, 2, 2) if kind == "cg2" else (8, 3, 3)))
        bcs["fixed"] = dict({'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                             'value': Constant((0.0, 0.0, amp))}, **tf)
        bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 4.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': Constant((0.0, 0.0, -1.0 if loaded else 0.0))}
        rec = [(4.0, 1.0, 1.0), (2.0, 0.5, 0.4), (0.0, 0.0, 0.0)]          # the last one sits on the moving face
    elif kind == "rectangle":
        mesh = RectangleMesh(Point(0, 0), Point(2, 1), 16, 8)
        bcs["fixed"] = dict({'boundary': AutoSubDomain(lambda x: near(x[1], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                             'value': Constant((amp, 0.0))}, **tf)
        bcs["punch"] = {'boundary': AutoSubDomain(lambda x: near(x[1], 1.0) and 0.5 - 1e-12 <= x[0] <= 1.5 + 1e-12), 'boundary_id': 2,
                        'type': 'stress', 'value': Constant((0.0, -1.0 if loaded else 0.0))}
        rec = [(1.0, 1.0), (0.3, 0.5), (2.0, 0.0)]
    else:
        mesh = _xml_mesh()
        bcs["fixed"] = dict({'boundary': AutoSubDomain(lambda x: near(x[2], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                             'value': Constant((amp, 0.0, 0.0))}, **tf)
        bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 20.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': Constant((1.0 if loaded else 0.0, 0.0, 0.0))}
        rec = [(10.0, 5.0, 20.0), (5.0, 2.0, 10.0), (0.0, 0.0, 0.0)]
    d = mesh.coordinates().shape[1]
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'solid', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': RHO_, 'thermal_expansion_coefficient': 0.0}
    if kind == "regions":
        s['material']['elastic_modulus'] = {'near': {'subdomain_id': 1, 'value': E_}, 'far': {'subdomain_id': 2, 'value': 0.6 * E_}}
        s['material']['density'] = {'near': {'subdomain_id': 1, 'value': RHO_}, 'far': {'subdomain_id': 2, 'value': 2.5 * RHO_}}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 2 if kind == "cg2" else 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': krylov}
    if times is None:
        s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': dt, 'ending_time': steps * dt}
    else:
        s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': times[0], 'time_series': list(times),
                                                      'ending_time': times[-1] - 1e-9 * (times[-1] - times[-2])}
    s['solver_settings']['dynamics_settings'] = dict({'spectral_radius': 0.8, 'rayleigh_mass': 0.4, 'rayleigh_stiffness': 0.002},
                                                     **(dynamics or {}))
    if loaded:
        s['load_time_function'] = dict(RICKER)
    if receivers:
        s['receivers'] = rec
    sub = MeshFunction("size_t", mesh, d)
    sub.array()[:] = np.where(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1)[:, 0] < 2.0, 1, 2)
    return s, sub


def _solver(kind, monkeypatch=None, **kw):
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    if monkeypatch is not None:
        monkeypatch.setenv("FS_RENUMBER", "0")                              # a file mesh in file order
    s, sub = _case(kind, **kw)
    solver = ElastodynamicsSolver(s)
    solver.subdomains = sub
    return solver


def _record_states(monkeypatch):
    """every (u, v, a) the marcher reaches, in device order"""
    from fenicssolver_amd import backend
    states = []
    correct = backend.DynamicsState.correct

    def recording(self, x, receivers=None):
        out = correct(self, x, receivers)
        states.append(self.get()[:3])
        return out
    monkeypatch.setattr(backend.DynamicsState, "correct", recording)
    return states


def _reference_of(solver, **kw):
    """the reference march of the case the solver has just run, on the exported K and M and the device's load vector"""
    assert solver.function_space.localizer() is None                       # device order = host order
    p = solver.generalized_alpha_parameters()
    sf, sg = solver.time_factors()
    u0, v0 = solver.initial_fields()
    dofs, vals = solver._dirichlet
    Kh, Mh = _host_csr(solver._K), _host_csr(solver._M)
    ref = er.march(Kh, Mh, solver._load, u0, v0, solver.step_lengths(), (p['alpha_m'], p['alpha_f'], p['beta'], p['gamma']),
                   eta_m=p['rayleigh_mass'], eta_k=p['rayleigh_stiffness'], sf=sf, sf0=solver._load_factor_at_start(sf), dofs=dofs, g=vals,
                   sg=sg, **kw)
    return ref, Kh, Mh


# ---- 2. the solver against the reference marcher, step by step ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle", "cg2", "regions", "xml"])
def test_solver_matches_the_reference_marcher_step_by_step(monkeypatch, kind):
    solver = _solver(kind, monkeypatch)
    states = _record_states(monkeypatch)
    u_last = solver.solve().vector()._values()
    ref, _, _ = _reference_of(solver)
    assert len(states) == STEPS and len(ref) == STEPS + 1
    d = solver.dimension
    worst = {"u": 0.0, "v": 0.0, "a": 0.0}
    for n, (got, want) in enumerate(zip(states, ref[1:])):
        for k, field in zip("uva", got):
            worst[k] = max(worst[k], np.abs(field - want[k]).max() / np.abs(want[k]).max())
    # the traces are the reference's displacement at the receiver dofs, the start included; all components
    rv = solver.receiver_vertices
    rdofs = (rv[:, None] * d + np.arange(d)[None, :]).ravel()
    tr_ref = np.stack([s['u'][rdofs].reshape(-1, d) for s in ref])
    tr = solver.receiver_traces()
    assert tr.shape == (STEPS + 1, 3, d) and np.array_equal(tr[0], tr_ref[0])
    worst["traces"] = np.abs(tr - tr_ref).max() / np.abs(tr_ref).max()
    print("\nsolver against the reference marcher, %s: largest relative difference over %d steps %s; iterations %s" % (
        kind, STEPS, {k: "%.2e" % v for k, v in worst.items()}, [s['iterations'] for s in solver.step_stats]))
    # it moves: the face drives the body and the load arrives
    assert np.abs(ref[-1]['u']).max() > 1e-3 and np.abs(tr[-1, 0]).max() > 0.0
    assert np.array_equal(u_last, states[-1][0])
    assert np.array_equal(solver.velocity().vector()._values(), states[-1][1])
    assert np.array_equal(solver.acceleration().vector()._values(), states[-1][2])
    for k in worst:
        assert worst[k] <= MARCH_TOL[k], (k, worst[k])
    assert solver.operator_assemblies == 1 and solver.amg_setups == (1 if d == 3 else 0)
    assert all(set(('predict_ms', 'solve_ms', 'correct_ms', 'iterations')) <= set(s) for s in solver.step_stats)


# ---- 3. single modes -------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _modes(kind):
    """(omega, Phi) of the eliminated (K, M) of an unloaded case with a fixed face, Phi M-orthonormal and zero on the Dirichlet dofs"""
    solver = _solver(kind, loaded=False, moving=False)
    solver._setup()
    Kh, Mh = _host_csr(solver._K).toarray(), _host_csr(solver._M).toarray()
    dofs, _ = solver._dirichlet
    free = np.setdiff1d(np.arange(Kh.shape[0]), dofs)
    lam, vec = scipy.linalg.eigh(Kh[np.ix_(free, free)], Mh[np.ix_(free, free)])
    Phi = np.zeros((Kh.shape[0], len(free)))
    Phi[free] = vec
    solver.close()
    return np.sqrt(lam), Phi


@pytest.mark.parametrize("kind, k", [("cantilever", 0), ("cantilever", 7), ("rectangle", 2)])
def test_a_single_mode_marches_at_the_discrete_frequency(monkeypatch, kind, k):
    om, Phi = _modes(kind)
    phi, steps = Phi[:, k], 12
    dt = 0.2 / om[k]
    amp = np.abs(phi).max()
    # undamped, trapezoidal rule: every step is phi cos(omega_h n dt)
    solver = _solver(kind, loaded=False, moving=False, steps=steps, dt=dt, dynamics={'spectral_radius': 1.0, 'rayleigh_mass': 0.0, 'rayleigh_stiffness': 0.0})
    solver.initial_values = {'displacement': phi}
    states = _record_states(monkeypatch)
    solver.solve()
    oh = er.discrete_frequency(om[k], dt)
    err = max(np.abs(s[0] - phi * math.cos(oh * (n + 1) * dt)).max() for n, s in enumerate(states)) / amp
    # damped, rho_inf = 0.6: the modal coordinate follows the scalar recursion at (omega_k, eta_M, eta_K)
    eta_m, eta_k = 0.3 * om[k], 0.05 / om[k]
    solver = _solver(kind, loaded=False, moving=False, steps=steps, dt=dt, dynamics={'spectral_radius': 0.6, 'rayleigh_mass': eta_m, 'rayleigh_stiffness': eta_k})
    solver.initial_values = {'displacement': phi}
    del states[:]
    solver.solve()
    scalar = er.march(np.array([[om[k] ** 2]]), np.array([[1.0]]), None, [1.0], [0.0], [dt] * steps, er.parameters(0.6), eta_m=eta_m, eta_k=eta_k)
    # (every field relative to its largest modal value over the run: v passes through zero)
    top = {f: max(abs(sc[f][0]) for sc in scalar) for f in "uva"}
    err_d = max(np.abs(s[j] - phi * scalar[n + 1][f][0]).max() / top[f] for n, s in enumerate(states) for j, f in enumerate("uva")) / amp
    print("\nmode %d of the %s (omega = %.4g, dt = %.4g): undamped against the closed form %.2e, damped against the scalar recursion %.2e" % (
        k, kind, om[k], dt, err, err_d))
    assert scalar[-1]['u'][0] < 0.9                                         # it decays
    assert err <= MODE_TOL and err_d <= MODE_DAMPED_TOL


# ---- 4. the energy identities of the trapezoidal rule ---------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle"])
def test_energy_is_conserved_undamped_and_dissipated_by_the_damping_matrix(monkeypatch, kind):
    om, Phi = _modes(kind)
    u0 = Phi[:, :6] @ np.array([1.0, -0.7, 0.5, 0.4, -0.3, 0.2])
    steps, dt = 40, 0.3 / om[3]
    trap = {'spectral_radius': 1.0, 'energy_freq': 1}
    solver = _solver(kind, loaded=False, moving=False, steps=steps, dt=dt, dynamics=dict(trap, rayleigh_mass=0.0, rayleigh_stiffness=0.0))
    solver.initial_values = {'displacement': u0}
    solver.solve()
    en = solver.energy()
    assert en.shape == (steps + 1, 3) and np.array_equal(en[:, 0], np.arange(steps + 1))
    E = en[:, 1] + en[:, 2]
    drift = np.abs(E - E[0]).max() / E[0]
    assert en[:, 1].max() > 0.05 * E[0]                                     # the energy does change hands
    # damped: E_{n+1} - E_n = -dt vbar^T C vbar, vbar = (v_n + v_{n+1}) / 2, C from the exported matrices
    eta_m, eta_k = 0.2 * om[0], 0.02 / om[5]
    solver = _solver(kind, loaded=False, moving=False, steps=steps, dt=dt, dynamics=dict(trap, rayleigh_mass=eta_m, rayleigh_stiffness=eta_k))
    solver.initial_values = {'displacement': u0}
    states = _record_states(monkeypatch)
    solver.solve()
    Kh, Mh = _host_csr(solver._K), _host_csr(solver._M)
    C = eta_m * Mh + eta_k * Kh
    en = solver.energy()
    Ed = en[:, 1] + en[:, 2]
    vs = [np.zeros(len(u0))] + [s[1] for s in states]
    loss = np.array([dt * float((0.5 * (vs[n] + vs[n + 1])) @ (C @ (0.5 * (vs[n] + vs[n + 1])))) for n in range(steps)])
    defect = np.abs(np.diff(Ed) + loss).max() / Ed[0]
    print("\nenergy of the trapezoidal rule, %s, %d steps: drift %.2e of E_0; damped: defect of the dissipation identity %.2e of E_0, "
          "E_end / E_0 = %.3f" % (kind, steps, drift, defect, Ed[-1] / Ed[0]))
    assert np.all(np.diff(Ed) < 0.0)                                        # strictly decreasing: a condition, not a measurement
    assert drift <= ENERGY_DRIFT_TOL and defect <= ENERGY_DRIFT_TOL


# ---- 5. build discipline ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle"])
@pytest.mark.parametrize("times", [None, (0.0, 0.05, 0.1, 0.2, 0.3, 0.4)], ids=["uniform", "two_step_lengths"])
def test_operator_and_hierarchy_are_built_once_per_step_length(monkeypatch, kind, times):
    from fenicssolver_amd import backend
    events = []
    apply_dirichlet, predict = backend.DeviceMatrix.apply_dirichlet, backend.DynamicsState.predict

    def counted(self, *a, **k):
        events.append("eliminate")
        return apply_dirichlet(self, *a, **k)

    def noted(self, *a, **k):
        events.append("step")
        return predict(self, *a, **k)
    monkeypatch.setattr(backend.DeviceMatrix, "apply_dirichlet", counted)
    monkeypatch.setattr(backend.DynamicsState, "predict", noted)
    solver = _solver(kind, steps=5, times=times, krylov=1e-10)
    solver.solve()
    lengths = 1 if times is None else 2
    assert solver.operator_assemblies == lengths
    assert solver.amg_setups == (lengths if solver.dimension == 3 else 0)
    # K_eff and the mass matrix of the initial acceleration are eliminated before the first step, K_eff again where the step length
    # changes (before the third step of the series), and no step eliminates anything else
    want = ["eliminate", "eliminate"] + ["step"] * 5 if times is None else ["eliminate", "eliminate", "step", "step", "eliminate", "step", "step", "step"]
    assert events == want
    assert len(solver.step_stats) == 5


# ---- 6. determinism and restart ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle"])
def test_two_solves_give_the_same_bits_and_outputs_do_not_disturb_the_march(kind):
    solver = _solver(kind, dynamics={'energy_freq': 2})

    def run(s):
        u = s.solve().vector()._values().copy()
        return u, s.velocity().vector()._values().copy(), s.acceleration().vector()._values().copy(), s.receiver_traces().copy(), s.energy().copy()
    first = run(solver)
    second = run(solver)                                                    # a second solve() starts from the initial state
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    assert first[4].shape == (STEPS // 2 + 1, 3) and np.abs(first[0]).max() > 0.0
    third = run(_solver(kind))                                              # a new solver, no energy
    assert third[4].shape == (0, 3)
    for a, b in zip(first[:4], third[:4]):
        assert np.array_equal(a, b)
    fourth = run(_solver(kind, receivers=False))                            # no receivers: correct() hands nothing back
    assert fourth[3].shape == (STEPS + 1, 0, solver.dimension)
    for a, b in zip(first[:3], fourth[:3]):
        assert np.array_equal(a, b)


def test_a_blow_up_names_the_step(monkeypatch):
    from fenicssolver_amd import backend
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver("rectangle", steps=4)
    correct = backend.DynamicsState.correct
    calls = []

    def poisoned(self, x, receivers=None):
        calls.append(1)
        if len(calls) == 3:
            xs = x.get()
            xs[5] = np.nan
            x.set(xs)
        return correct(self, x, receivers)
    monkeypatch.setattr(backend.DynamicsState, "correct", poisoned)
    with pytest.raises(SolverError, match="not finite after step 3"):
        solver.solve()


# ---- 7. the refusals of the library -----------------------------------------------------------------------------------------------
def test_library_refusals_leave_the_state_unchanged():
    from fenicssolver_amd import backend, _lib as L
    import ctypes as C
    backend.init()
    mesh = backend.DeviceMesh.box(2, 2, 2)
    V, V1 = backend.DeviceSpace(mesh, 3, 1), backend.DeviceSpace(mesh, 1, 1)
    Vb = backend.DeviceSpace(backend.DeviceMesh.box(3, 2, 2), 3, 1)
    n = V.n_owned
    h = C.c_void_p()
    for space, msg in ((V1, "vector CG1 or CG2 spaces"), (backend.DeviceDGSpace(mesh), "not built for DG spaces")):
        rc = L.load().fs_dyn_state_create(space.h, C.byref(h))
        assert rc == -1 and msg in L.load().fs_last_error().decode(), (rc, L.load().fs_last_error())
    K, M, Kb = backend.DeviceMatrix(V), backend.DeviceMatrix(V), backend.DeviceMatrix(Vb)
    K.assemble(lame=(MU_, LM_))
    M.assemble(lame=(0.0, 0.0), mass=RHO_)
    Kb.assemble(lame=(MU_, LM_))
    st = backend.DynamicsState(V)
    rhs, x = backend.DeviceVector(n), backend.DeviceVector(n)
    par = er.parameters(0.5)

    def refused(call, msg):
        with pytest.raises(backend.BackendError, match=msg) as e:
            call()
        assert e.value.rc == -1                                             # FS_ERR_INVALID

    refused(lambda: st.predict(K, M, 1.0, 1.0, rhs), "was not configured")
    refused(lambda: st.correct(x), "was not configured")
    refused(lambda: st.energy(K, M), "was not configured")
    rng = np.random.default_rng(1)
    u, v, a, F = (rng.standard_normal(n) for _ in range(4))
    st.configure(0.1, *par, 0.1, 0.01, load=F, dirichlet_dofs=[0, 4], dirichlet_values=[1.0, 2.0])
    refused(lambda: st.predict(K, M, 1.0, 1.0, rhs), "holds no")
    refused(lambda: st.correct(x), "holds no")
    refused(lambda: st.energy(K, M), "holds no")
    refused(lambda: st.start(x), "no initial state is waiting")
    st.set(u, v, a, step=2)
    st.predict(K, M, 0.5, 0.25, rhs)
    before = st.get(), st.work(), rhs.get()

    for bad_dt in (0.0, -0.1, float('inf'), float('nan')):
        refused(lambda: st.configure(bad_dt, *par), "dt > 0 and finite")
    refused(lambda: st.configure(0.1, 0.0, 0.0, 1.0 / 6.0, 0.5), "not unconditionally stable")
    refused(lambda: st.configure(0.1, 0.3, 0.2, 0.3, 0.5), "not unconditionally stable")
    refused(lambda: st.configure(0.1, 0.0, 0.6, 0.6, 0.5), "not unconditionally stable")
    refused(lambda: st.configure(0.1, 0.0, 0.0, float('nan'), 0.5), "not finite")
    refused(lambda: st.configure(0.1, *par, -0.1, 0.0), "must be >= 0")
    refused(lambda: st.configure(0.1, *par, 0.0, -0.1), "must be >= 0")
    refused(lambda: st.configure(0.1, *par, dirichlet_dofs=[0, n], dirichlet_values=[1.0, 1.0]), "outside the space")
    refused(lambda: st.configure(0.1, *par, dirichlet_dofs=[-1], dirichlet_values=[1.0]), "outside the space")
    refused(lambda: st.predict(Kb, M, 1.0, 1.0, rhs), "another space")
    refused(lambda: st.predict(K, Kb, 1.0, 1.0, rhs), "another space")
    refused(lambda: st.energy(Kb, M), "another space")
    refused(lambda: st.predict(K, M, float('nan'), 1.0, rhs), "not finite")
    refused(lambda: st.predict(K, M, 1.0, 1.0, backend.DeviceVector(n - 1)), "right-hand side has")
    refused(lambda: st.correct(backend.DeviceVector(n - 1)), "solution has")
    refused(lambda: st.correct(x, [0, n]), "receiver dof")
    refused(lambda: st.correct(x, [-1]), "receiver dof")
    refused(lambda: st.set(u, v, a, step=-1), "n >= 0")
    after = st.get(), st.work(), rhs.get()
    assert before[0][3] == after[0][3] == 2
    for x0, x1 in zip(before[0][:3] + before[1] + (before[2],), after[0][:3] + after[1] + (after[2],)):
        assert np.array_equal(x0, x1)
    # ... and the constants too: the same predict gives the same bits
    st.predict(K, M, 0.5, 0.25, rhs)
    assert np.array_equal(rhs.get(), before[2])
