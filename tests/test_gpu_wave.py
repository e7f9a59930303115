"""WaveSolver and the fs_wave_* entry points on the MI355X: the start and the update kernel against the numpy reference
(tests/wave_reference.py), the batch discipline (any split of a march gives the same bits), the state hand-over, the discrete energy on
the device, the solver end to end against the reference marcher, the step bounds and the hygiene of the state object."""
import copy
import gc
import math
from collections import OrderedDict

import numpy as np
import pytest

import wave_reference as wr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}

KERNEL_TOL = 1e-12          # set by the issue: fields, traces and both energy halves against the reference, relative to the largest entry

# Measured on the MI355X (the tests print every figure before they assert).
# Closed domain, 17 x 13 x 11 box, 200 steps at 0.9 x 2/sqrt(lambda_G): ptp(E)/max(E) of the device energy MEASURED_ENERGY_GPU, of the numpy
# reference on the same case MEASURED_ENERGY_REF; the bound is 10 x the reference's figure, computed by the test on the same case.
MEASURED_ENERGY_GPU = 4.44e-16
MEASURED_ENERGY_REF = 4.44e-16
# Kernel against the reference (start and 10 steps; KERNEL_TOL is the issue's): fields 7.2e-15, traces 1.6e-14, energy halves 1.6e-15.
# Solver against the reference marcher, step by step (field at the end, every trace sample, the energy, the velocity; relative to the
# largest entry): standing wave 16 x 16 SOLVER_MEASURED_2D, box 8 x 6 x 5 with a Ricker point source SOLVER_MEASURED_3D.  The bound is
# 10 x the larger.
SOLVER_MEASURED_2D = 1.53e-14     # velocity; field 1.13e-14, traces 2.4e-15, energy 1.9e-15
SOLVER_MEASURED_3D = 1.04e-14     # field; traces 1.8e-15, energy 1.4e-15
SOLVER_MEASURED = max(SOLVER_MEASURED_2D, SOLVER_MEASURED_3D)
SOLVER_TOL = 10 * SOLVER_MEASURED


# ---- meshes and problems ---------------------------------------------------------------------------------------------------------
def _mesh(kind):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point
    if kind == "rect":
        return RectangleMesh(Point(0, 0), Point(1.0, 0.7), 6, 5)
    if kind == "box":
        return BoxMesh(Point(0, 0, 0), Point(1.0, 0.8, 0.6), 4, 3, 3)
    if kind == "tiny":
        return BoxMesh(Point(0, 0, 0), Point(1.0, 0.8, 0.6), 2, 2, 2)          # 27 dofs
    return BoxMesh(Point(0, 0, 0), Point(1.0, 0.8, 0.6), 17, 13, 11)          # 3024 dofs: several workgroups, no multiple of 64


class Problem:
    """One mesh with a per-region speed, a Dirichlet side (x = 0), a flux side (x = 1) and an absorbing side (y = 0), on the host
    (reference arrays) and on the device (assembled there)."""

    def __init__(self, kind, seed=11, closed=False, absorbing=True, dirichlet_values=True):
        from fenicssolver_amd.fem import FunctionSpace
        from fenicssolver_amd import backend
        backend.init()
        self.backend = backend
        mesh = _mesh(kind)
        self.coords, self.cells = mesh.coordinates().copy(), mesh.cells().astype(np.int64)
        co, ce = self.coords, self.cells
        rng = np.random.default_rng(seed)
        n = len(co)
        self.n = n
        self.c_cell = np.where(co[ce].mean(axis=1)[:, 0] < 0.5, 1.0, 1.5)
        facets, fcell = wr.boundary_facets(ce)
        fx = co[facets]
        side = lambda axis, v: np.all(fx[:, :, axis] == v, axis=1)      # noqa: E731
        self.K, self.m = wr.stiffness(co, ce, self.c_cell), wr.lumped_mass(co, ce)
        ab = side(1, 0.0) & (not closed) & absorbing
        fl = side(0, 1.0) & (not closed)
        self.d = wr.damping(co, facets[ab], fcell[ab], self.c_cell) if ab.any() else np.zeros(n)
        self.F = np.zeros(n) if closed else rng.standard_normal(n) * self.m + wr.facet_vector(co, facets[fl], 0.7)
        self.bc = np.nonzero(co[:, 0] == 0.0)[0].astype(np.int32)
        self.g = rng.standard_normal(len(self.bc)) if (dirichlet_values and not closed) else np.zeros(len(self.bc))
        self.u0, self.v0 = rng.standard_normal(n), rng.standard_normal(n)
        if closed:
            self.u0[self.bc] = 0.0
        self.dt = 0.9 * wr.critical_time_step(self.K, self.m)
        # the device side
        self.V = FunctionSpace(mesh, "Lagrange", 1)
        dV = self.dV = self.V.device()
        self.Kd = backend.DeviceMatrix(dV)
        self.Kd.assemble(stiffness=("cell", self.c_cell ** 2))
        vec = backend.DeviceVector(n)
        backend.assemble_vector(dV, vec, source=1.0)
        self.m_dev = vec.get()
        vec.fill(0.0)
        if ab.any():
            backend.assemble_facet_vector(dV, vec, facets[ab].astype(np.int32), self.c_cell[fcell[ab]])
        self.d_dev = vec.get()
        vec.fill(0.0)
        if fl.any():
            backend.assemble_facet_vector(dV, vec, facets[fl].astype(np.int32), 0.7)
        self.F_dev = self.F - (wr.facet_vector(co, facets[fl], 0.7) if fl.any() else 0.0) + vec.get()
        vec.close()

    def state(self, dt=None):
        st = self.backend.WaveState(self.dV)
        st.configure(self.dt if dt is None else dt, self.m_dev, self.d_dev, self.F_dev, self.bc, self.g)
        return st

    def reference(self, n_steps, sf, sg, receivers=None, dt=None):
        return wr.march(self.K, self.m, self.d, self.F, self.dt if dt is None else dt, self.u0, self.v0, n_steps, sf, sg, self.bc, self.g, receivers)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300))


@pytest.fixture(scope="module")
def big():
    """the 17 x 13 x 11 box with loads, shared by the tests that only read it"""
    return Problem("big")


@pytest.fixture(scope="module")
def big_closed():
    return Problem("big", closed=True)


# ---- kernel against the reference ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["rect", "box", "big"])
def test_start_and_update_kernel_against_the_reference(kind):
    P = Problem(kind)
    for name, dev, ref in (("mass", P.m_dev, P.m), ("damping", P.d_dev, P.d), ("load", P.F_dev, P.F)):
        print("%s %s: device assembly against the reference %.3g" % (kind, name, _rel(dev, ref)))
        assert _rel(dev, ref) <= KERNEL_TOL
    rng = np.random.default_rng(5)
    N = 11                                                    # the start and 10 steps of fs_wave_advance
    sf, sg = rng.standard_normal(N), rng.standard_normal(N + 1)
    rec = np.array([int(P.bc[1]), P.n - 1, 7, 7, P.n // 2], dtype=np.int32)        # a Dirichlet dof, the last row, one dof twice
    ref = P.reference(N, sf, sg, rec)
    st = P.state()
    st.start(P.Kd, P.u0, P.v0, sf[0], sg[1])
    up, u, step = st.get()
    assert step == 1 and np.array_equal(up, P.u0)
    u1_ref = wr.start(P.K, P.m, P.d, P.F, P.dt, P.u0, P.v0, sf[0], sg[1], P.bc, P.g)
    print("%s start: %.3g" % (kind, _rel(u, u1_ref)))
    assert _rel(u, u1_ref) <= KERNEL_TOL
    out = st.advance(P.Kd, sf[1:], sg[2:], receivers=rec)
    up, u, step = st.get()
    figs = {"u": _rel(u, ref["u"]), "u_prev": _rel(up, ref["u_prev"]), "traces": _rel(out["traces"], ref["traces"][2:]),
            "kinetic": _rel(out["energy"][:, 0], ref["energy"][1:, 0]), "potential": _rel(out["energy"][:, 1], ref["energy"][1:, 1])}
    print("%s 10 steps against the reference:" % kind, figs)
    assert step == N and out["step"] == N and out["n_nonfinite"] == 0 and out["first_nonfinite_step"] == -1
    assert max(figs.values()) <= KERNEL_TOL
    assert np.array_equal(out["traces"][-1], u[rec]) and out["device_ms"] > 0.0
    st.close()


# ---- batch discipline ------------------------------------------------------------------------------------------------------------
def _march(P, splits, sf, sg, rec, traces=True, energy=True):
    st = P.state()
    st.start(P.Kd, P.u0, P.v0, sf[0], sg[1])
    tr, en, n = [], [], 1
    for k in splits:
        out = st.advance(P.Kd, sf[n:n + k], sg[n + 1:n + k + 1], receivers=rec, traces=traces, energy=energy, info=energy)
        tr.append(out["traces"])
        en.append(out["energy"])
        n += k
    up, u, step = st.get()
    st.close()
    assert step == n
    return up, u, (np.concatenate(tr) if traces else None), (np.concatenate(en) if energy else None)


def test_any_split_of_a_march_gives_the_same_bits(big):
    rng = np.random.default_rng(8)
    sf, sg = rng.standard_normal(13), rng.standard_normal(14)
    rec = np.array([5, 3000, 1500], dtype=np.int32)
    one = _march(big, [12], sf, sg, rec)
    for splits in ([1] * 12, [4, 4, 4], [12]):           # ... and a repeated run from the same state
        other = _march(big, splits, sf, sg, rec)
        for a, b in zip(one, other):
            assert np.array_equal(a, b), splits
    assert np.all(np.isfinite(one[1])) and np.abs(one[3]).max() > 0.0


def test_a_march_longer_than_one_chunk_of_partials_gives_the_same_bits():
    """the energy partials are summed every 64 steps: 150 steps in one call (three finishing passes) against 64 + 64 + 22 and 50 x 3"""
    P = Problem("box")
    rng = np.random.default_rng(9)
    sf, sg = 0.1 * rng.standard_normal(151), 0.1 * rng.standard_normal(152)
    rec = np.array([0, 9], dtype=np.int32)
    one = _march(P, [150], sf, sg, rec)
    assert np.all(np.isfinite(one[3])) and one[3].shape == (150, 2) and one[2].shape == (150, 2)
    for splits in ([64, 64, 22], [3] * 50):
        for a, b in zip(one, _march(P, splits, sf, sg, rec)):
            assert np.array_equal(a, b), splits


def test_get_then_set_continues_the_march_bit_for_bit(big):
    rng = np.random.default_rng(10)
    sf, sg = rng.standard_normal(13), rng.standard_normal(14)
    rec = np.array([17], dtype=np.int32)
    up_a, u_a, tr_a, en_a = _march(big, [12], sf, sg, rec)
    st = big.state()
    st.start(big.Kd, big.u0, big.v0, sf[0], sg[1])
    o1 = st.advance(big.Kd, sf[1:6], sg[2:7], receivers=rec)
    up, u, step = st.get()
    st.close()
    st2 = big.state()                                       # another state object takes over
    st2.set(up, u, step)
    o2 = st2.advance(big.Kd, sf[6:13], sg[7:14], receivers=rec)
    up_b, u_b, step_b = st2.get()
    st2.close()
    assert step == 6 and step_b == 13
    assert np.array_equal(up_a, up_b) and np.array_equal(u_a, u_b)
    assert np.array_equal(tr_a, np.concatenate([o1["traces"], o2["traces"]])) and np.array_equal(en_a, np.concatenate([o1["energy"], o2["energy"]]))


def test_the_receiver_list_may_change_from_call_to_call_on_one_state():
    """The receiver bits of the device flags follow the list of the call; a bit that is not set leaves its slot of a freshly allocated
    trace buffer unwritten.  Exact: a sample is the field value itself."""
    P = Problem("tiny")
    assert P.n == 27
    free = np.setdiff1d(np.arange(P.n), P.bc)
    A = np.array([free[0], P.bc[1], free[5]], dtype=np.int32)              # one of them a Dirichlet dof
    B = np.array([free[2], P.bc[0], free[7]], dtype=np.int32)              # disjoint from A
    C = np.array([A[2], A[2]], dtype=np.int32)                             # shorter, a dof of A, named twice
    rng = np.random.default_rng(21)
    sf, sg = rng.standard_normal(7), rng.standard_normal(8)
    st = P.state()
    st.start(P.Kd, P.u0, P.v0, sf[0], sg[1])

    def step_with(rec, n):
        out = st.advance(P.Kd, sf[n:n + 1], sg[n + 1:n + 2], receivers=rec)
        _, u, step = st.get()
        assert step == n + 1 and out["step"] == n + 1
        if rec is None:
            assert out["traces"] is None
        else:
            assert out["traces"].shape == (1, len(rec)) and np.array_equal(out["traces"][0], u[rec]), (n, rec)
    for n, rec in enumerate((A, B, C, None, A), start=1):
        step_with(rec, n)
    up, u, step = st.get()
    st.configure(P.dt, P.m_dev, P.d_dev, P.F_dev, P.bc, P.g)                 # the flags are uploaded anew, without receiver bits
    st.set(up, u, step)
    step_with(B, 6)
    st.close()


def test_null_traces_and_null_energy_advance_the_state_identically(big):
    rng = np.random.default_rng(12)
    sf, sg = rng.standard_normal(13), rng.standard_normal(14)
    rec = np.array([5, 3000], dtype=np.int32)
    a = _march(big, [12], sf, sg, rec)
    b = _march(big, [5, 7], sf, sg, rec, traces=False, energy=False)
    assert b[2] is None and b[3] is None
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])


# ---- the discrete energy on the device -------------------------------------------------------------------------------------------
def test_closed_domain_conserves_the_discrete_energy(big_closed):
    P = big_closed
    N = 201                                                  # the start and 200 device steps at 0.9 x 2/sqrt(lambda_G)
    ones = np.ones(N + 1)
    up, u, _, en = _march(P, [200], ones[:N], ones, np.zeros(0, dtype=np.int32), traces=False)
    E = en.sum(axis=1)
    ref = P.reference(N, ones[:N], ones)
    E_ref = ref["energy"][1:].sum(axis=1)
    drift, drift_ref = np.ptp(E) / E.max(), np.ptp(E_ref) / E_ref.max()
    print("closed 17 x 13 x 11 box, 200 steps: ptp(E)/max(E) device %.3g reference %.3g; E device / reference - 1 = %.3g" % (
        drift, drift_ref, _rel(E, E_ref)))
    assert np.all(np.isfinite(u)) and _rel(E, E_ref) <= 1e-10
    assert drift <= 10.0 * drift_ref


def test_an_absorbing_side_only_removes_energy():
    N = 201
    ones = np.ones(N + 1)
    E = {}
    for absorbing in (True, False):
        P = Problem("big", absorbing=absorbing, dirichlet_values=False)
        P.F_dev[:] = 0.0                                     # no source: Dirichlet (zero), natural and absorbing sides only
        P.F[:] = 0.0
        P.u0[P.bc] = 0.0
        E[absorbing] = _march(P, [200], ones[:N], ones, np.zeros(0, dtype=np.int32), traces=False)[3].sum(axis=1)
    Ea, En = E[True], E[False]
    print("absorbing side: E0 %.6g E_end %.6g largest increase / E0 %.3g; natural side instead: E_end %.6g" % (
        Ea[0], Ea[-1], np.diff(Ea).max() / Ea[0], En[-1]))
    assert np.diff(Ea).max() <= 1e-14 * Ea[0]
    assert Ea[-1] < En[-1]


# ---- the solver end to end ---------------------------------------------------------------------------------------------------------
def _settings(V, bcs, dt, t_end, **extra):
    from fenicssolver_amd import SolverBase as SB
    s = copy.deepcopy(SB.default_case_settings)
    s['solver_name'] = 'WaveSolver'
    s['material'] = {'wave_speed': 1.0}
    s['function_space'] = V
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': dt, 'ending_time': t_end}
    s.update(extra)
    return s


def _square_case(n=16, **extra):
    from fenicssolver_amd.fem import UnitSquareMesh, FunctionSpace, CompiledSubDomain
    mesh = UnitSquareMesh(n, n)
    bcs = OrderedDict()
    bcs["all"] = {'boundary': CompiledSubDomain("on_boundary"), 'boundary_id': 1, 'type': 'Dirichlet', 'value': 0.0}
    err_ref, en_ref, dt, N, lam, u_ref = wr.standing_wave(n)
    s = _settings(FunctionSpace(mesh, "Lagrange", 1), bcs, dt, 1.0, **extra)
    s['initial_values'] = {'displacement': 'sin(pi*x[0])*sin(pi*x[1])'}
    return s, (err_ref, en_ref, dt, N, lam, u_ref)


def test_solver_standing_wave_against_the_reference_marcher(gpu):
    from fenicssolver_amd.WaveSolver import WaveSolver
    s, (err_ref, en_ref, dt, N, lam, u_ref) = _square_case(16, receivers=[(0.5, 0.5), (0.26, 0.7)])
    solver = WaveSolver(s)
    u = solver.solve().vector().get_local()
    co = solver.mesh.coordinates()
    exact = np.sin(math.pi * co[:, 0]) * np.sin(math.pi * co[:, 1]) * math.cos(math.sqrt(2.0) * math.pi)
    err = float(np.abs(u - exact).max())
    coords, cells = wr.unit_square(16)
    K, m = wr.stiffness(coords, cells, 1.0), wr.lumped_mass(coords, cells)
    bc = np.nonzero((coords == 0).any(axis=1) | (coords == 1).any(axis=1))[0]
    u0 = np.sin(math.pi * co[:, 0]) * np.sin(math.pi * co[:, 1])
    ref = wr.march(K, m, 0 * m, 0 * m, dt, u0, 0 * m, N, bc_dofs=bc, bc_vals=np.zeros(len(bc)), receivers=solver.receiver_vertices)
    figs = {"u": _rel(u, ref["u"]), "traces": _rel(solver.receiver_traces(), ref["traces"]), "energy": _rel(solver.energy(), ref["energy"]),
            "velocity": _rel(solver.velocity(), (ref["u"] - wr.march(K, m, 0 * m, 0 * m, dt, u0, 0 * m, N - 2, bc_dofs=bc,
                                                                     bc_vals=np.zeros(len(bc)))["u"]) / (2 * dt))}
    print("standing wave 16 x 16, %d steps: error at T = 1 device %.6g reference %.6g; against the reference marcher" % (N, err, err_ref), figs)
    assert solver.receiver_traces().shape == (N + 1, 2) and solver.energy().shape == (N, 2)
    assert solver.receiver_vertices.tolist() == [8 * 17 + 8, 11 * 17 + 4]
    assert abs(err - err_ref) <= 0.01 * err_ref
    assert abs(solver.critical_time_step() - 2.0 / math.sqrt(lam)) <= 1e-12 * 2.0 / math.sqrt(lam)
    assert len(solver.step_stats) >= 1 and sum(b['steps'] for b in solver.step_stats) == N - 1 and solver.step_stats[0]['ms_per_step'] > 0
    assert max(figs.values()) <= SOLVER_TOL
    solver.close()


def test_solver_ricker_point_source_in_a_box_against_the_reference_marcher(gpu):
    from fenicssolver_amd.fem import BoxMesh, Point, FunctionSpace, CompiledSubDomain
    from fenicssolver_amd.WaveSolver import WaveSolver
    mesh = BoxMesh(Point(0, 0, 0), Point(1.0, 0.8, 0.6), 8, 6, 5)
    coords, cells = mesh.coordinates().copy(), mesh.cells().astype(np.int64)
    region = (coords[cells].mean(axis=1)[:, 0] >= 0.5).astype(np.int64)
    c_cell = np.where(region == 0, 1.0, 1.5)
    K, m = wr.stiffness(coords, cells, c_cell), wr.lumped_mass(coords, cells)
    dt = 0.5 * wr.critical_time_step(K, m)
    N = 60
    bcs = OrderedDict()
    bcs["left"] = {'boundary': CompiledSubDomain("near(x[0], 0.0) && on_boundary"), 'boundary_id': 1, 'type': 'Dirichlet', 'value': 0.0}
    bcs["right"] = {'boundary': CompiledSubDomain("near(x[0], 1.0) && on_boundary"), 'boundary_id': 2, 'type': 'absorbing'}
    bcs["top"] = {'boundary': CompiledSubDomain("near(x[2], 0.6) && on_boundary"), 'boundary_id': 3, 'type': 'flux', 'value': 0.2}
    wavelet = {'type': 'ricker', 'frequency': 3.0, 'delay': 10 * dt}
    s = _settings(FunctionSpace(mesh, "Lagrange", 1), bcs, dt, N * dt, source_time_function=wavelet,
                  point_source=[((0.4, 0.3, 0.3), 2.0)], receivers=[(0.7, 0.4, 0.3), (0.2, 0.6, 0.1)], batch_steps=25)
    s['material'] = {'wave_speed': {'slow': {'subdomain_id': 0, 'value': 1.0}, 'fast': {'subdomain_id': 1, 'value': 1.5}}}
    solver = WaveSolver(s)
    solver.subdomains.array()[:] = region
    u = solver.solve().vector().get_local()
    # the reference on the same case
    facets, fcell = wr.boundary_facets(cells)
    fx = coords[facets]
    right, top = np.all(fx[:, :, 0] == 1.0, axis=1), np.all(fx[:, :, 2] == 0.6, axis=1)
    d = wr.damping(coords, facets[right], fcell[right], c_cell)
    F = wr.facet_vector(coords, facets[top], 0.2)
    pd, pw = wr.point_load(coords, cells, (0.4, 0.3, 0.3), 2.0)
    np.add.at(F, pd, pw)
    bc = np.nonzero(coords[:, 0] == 0.0)[0]
    sf = wr.ricker(dt * np.arange(N), 3.0, 10 * dt)
    rec = [int(np.argmin(((coords - np.asarray(p)) ** 2).sum(axis=1))) for p in ((0.7, 0.4, 0.3), (0.2, 0.6, 0.1))]
    ref = wr.march(K, m, d, F, dt, 0 * m, 0 * m, N, sf=sf, bc_dofs=bc, bc_vals=np.zeros(len(bc)), receivers=rec)
    figs = {"u": _rel(u, ref["u"]), "traces": _rel(solver.receiver_traces(), ref["traces"]), "energy": _rel(solver.energy(), ref["energy"])}
    print("box 8 x 6 x 5 with a Ricker point source, %d steps, against the reference marcher:" % N, figs)
    assert solver.receiver_vertices.tolist() == rec and np.abs(ref["traces"]).max() > 1e-3
    assert [b['steps'] for b in solver.step_stats] == [25, 25, 8, 1]
    assert abs(solver.critical_time_step() - wr.critical_time_step(K, m)) <= 1e-12 * wr.critical_time_step(K, m)
    assert max(figs.values()) <= SOLVER_TOL
    solver.close()


# ---- step bounds ---------------------------------------------------------------------------------------------------------------------
def test_a_step_above_the_power_iteration_bound_raises_before_any_marching_call(gpu, monkeypatch):
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    s, _ = _square_case(16)
    probe = WaveSolver(copy.copy(s))
    stable, certain = probe.time_step_bounds()
    probe.close()
    assert stable < certain <= stable * 1.5                 # lambda_P <= lambda_max <= lambda_G (the ratio of the last two: 1.446)
    calls = {"march": 0, "products": 0}
    spmv = gpu.DeviceMatrix.spmv
    monkeypatch.setattr(gpu.WaveState, "start", lambda *a, **k: calls.__setitem__("march", calls["march"] + 1))
    monkeypatch.setattr(gpu.WaveState, "advance", lambda *a, **k: calls.__setitem__("march", calls["march"] + 1))
    monkeypatch.setattr(gpu.DeviceMatrix, "spmv", lambda self, x, y: (calls.__setitem__("products", calls["products"] + 1), spmv(self, x, y))[1])
    s['solver_settings']['transient_settings'].update(time_step=1.05 * certain, ending_time=20 * 1.05 * certain)
    solver = WaveSolver(s)
    with pytest.raises(SolverError, match="certain to blow up"):
        solver.solve()
    solver.close()
    assert calls["march"] == 0 and calls["products"] >= 30   # the power iteration's products did run


def test_a_step_just_below_the_gershgorin_bound_runs(gpu):
    from fenicssolver_amd.WaveSolver import WaveSolver
    s, _ = _square_case(16)
    probe = WaveSolver(copy.copy(s))
    stable = probe.critical_time_step()
    probe.close()
    s['solver_settings']['transient_settings'].update(time_step=0.99 * stable, ending_time=200 * 0.99 * stable)
    solver = WaveSolver(s)
    solver.solve()
    E = solver.energy().sum(axis=1)
    print("0.99 x 2/sqrt(lambda_G), 200 steps: ptp(E)/max(E) = %.3g" % (np.ptp(E) / E.max()))
    assert E.shape == (200,) and np.all(np.isfinite(E)) and np.ptp(E) <= 1e-10 * E.max()
    solver.close()


def test_a_blow_up_names_the_steps_and_both_bounds(gpu, monkeypatch):
    """between the two bounds nothing is certain, so the march runs (with a warning); a field that leaves the finite numbers is reported"""
    from fenicssolver_amd import WaveSolver as W
    from fenicssolver_amd.SolverBase import SolverError
    s, _ = _square_case(16)
    s['initial_values'] = {'displacement': np.random.default_rng(1).standard_normal(17 * 17) * 1e100}
    monkeypatch.setattr(W.WaveSolver, "_power_iteration", lambda self, K, m, dofs: 1e-30)      # no certainty: lambda_P tiny
    probe = W.WaveSolver(copy.copy(s))
    stable = probe.critical_time_step()
    probe.close()
    s['solver_settings']['transient_settings'].update(time_step=3.0 * stable, ending_time=400 * 3.0 * stable)
    solver = W.WaveSolver(s)
    with pytest.raises(SolverError, match=r"not finite in steps \d+ \.\. \d+ .*lambda_G.*lambda_P"):
        solver.solve()
    solver.close()


# ---- hygiene -------------------------------------------------------------------------------------------------------------------------
def test_memory_returns_to_its_starting_level_after_close(big):
    B = big.backend
    x, y = B.DeviceVector(big.n), B.DeviceVector(big.n)
    big.Kd.spmv(x, y)                                       # what the first product of a space builds stays with the space
    gc.collect()                                            # device objects of earlier tests that wait for the collector go now, not below
    before = B.memory_info()["live_bytes"]
    st = big.state()
    st.start(big.Kd, big.u0, big.v0)
    st.advance(big.Kd, np.ones(70), np.ones(70), receivers=np.array([1, 2], dtype=np.int32))
    assert B.memory_info()["live_bytes"] > before
    st.close()
    assert B.memory_info()["live_bytes"] == before


def test_invalid_arguments_are_refused_with_a_message(big):
    from fenicssolver_amd.fem import VectorFunctionSpace, FunctionSpace
    B = big.backend
    with pytest.raises(B.BackendError, match="scalar CG1 spaces"):
        B.WaveState(VectorFunctionSpace(_mesh("box"), "Lagrange", 1).device())
    with pytest.raises(B.BackendError, match="scalar CG1 spaces"):
        B.WaveState(FunctionSpace(_mesh("box"), "Lagrange", 2).device())
    st = B.WaveState(big.dV)
    with pytest.raises(B.BackendError, match="not configured"):
        st.start(big.Kd, big.u0, big.v0)
    for dt in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(B.BackendError, match="dt > 0 and finite"):
            st.configure(dt, big.m_dev)
    m = big.m_dev.copy()
    m[77] = 0.0
    with pytest.raises(B.BackendError, match="lumped mass of row 77"):
        st.configure(0.1, m)
    d = np.zeros(big.n)
    d[5] = -1e-3
    with pytest.raises(B.BackendError, match="damping of row 5"):
        st.configure(0.1, big.m_dev, d)
    for dof in (-1, big.n):
        with pytest.raises(B.BackendError, match="Dirichlet dof %d outside" % dof):
            st.configure(0.1, big.m_dev, None, None, [3, dof], [0.0, 0.0])
    st.configure(big.dt, big.m_dev)
    with pytest.raises(B.BackendError, match="holds no"):
        st.advance(big.Kd, [1.0], [1.0])
    st.start(big.Kd, big.u0, big.v0)
    for dof in (-1, big.n):
        with pytest.raises(B.BackendError, match="receiver dof %d outside" % dof):
            st.advance(big.Kd, [1.0], [1.0], receivers=[0, dof])
    other = Problem("box")
    with pytest.raises(B.BackendError, match="another space"):
        st.advance(other.Kd, [1.0], [1.0])
    assert st.get()[2] == 1                                  # none of the refused calls moved the state
    st.close()
