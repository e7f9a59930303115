"""WaveSolver without a device: the numpy reference (tests/wave_reference.py) against the standing wave and the energy laws of the
model, the refusals of the solver class, its time functions and the receiver snapping."""
import copy
import math
from collections import OrderedDict

import numpy as np
import pytest

import wave_reference as wr

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}


# ---- the reference itself ------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def standing():
    """n -> (max error at T = 1, energy [N, 2], dt, N, lambda_G): right-diagonal triangles, half the Gershgorin step"""
    return {n: wr.standing_wave(n, safety=0.5, T=1.0)[:5] for n in (8, 16, 32)}


def test_reference_standing_wave_converges_at_second_order(standing):
    e8, e16, e32 = (standing[n][0] for n in (8, 16, 32))
    print("standing wave: max error", e8, e16, e32, "ratios", e8 / e16, e16 / e32)
    assert e8 / e16 >= 3.0 and e16 / e32 >= 3.0        # a second-order condition (found: 3.99, 4.01)


def test_reference_standing_wave_conserves_the_discrete_energy(standing):
    for n in (8, 16, 32):
        E = standing[n][1].sum(axis=1)
        drift = np.ptp(E) / E.max()
        print("standing wave n = %d: ptp(E)/max(E) = %.3g over %d steps" % (n, drift, len(E)))
        assert drift <= 1e-13                           # found: <= 3e-15


def test_reference_step_is_half_the_gershgorin_step_and_a_whole_number_of_steps(standing):
    for n in (8, 16, 32):
        _, _, dt, N, lam = standing[n]
        assert abs(N * dt - 1.0) <= 1e-15 and dt <= 0.5 * 2.0 / math.sqrt(lam) and (N - 1) * 0.5 * 2.0 / math.sqrt(lam) < 1.0


def test_gershgorin_bounds_the_largest_eigenvalue_from_above():
    coords, cells = wr.unit_square(8)
    K, m = wr.stiffness(coords, cells, 1.0), wr.lumped_mass(coords, cells)
    ratio = wr.gershgorin(K, m) / wr.lambda_max(K, m)
    assert 1.0 <= ratio <= 1.5                          # found: 1.446


def _absorbing_case(absorb):
    coords, cells = wr.unit_square(12)
    rng = np.random.default_rng(3)
    c_cell = np.where(coords[cells].mean(axis=1)[:, 0] < 0.5, 1.0, 1.6)
    K, m = wr.stiffness(coords, cells, c_cell), wr.lumped_mass(coords, cells)
    facets, fcell = wr.boundary_facets(cells)
    right = np.all(coords[facets][:, :, 0] == 1.0, axis=1)
    d = wr.damping(coords, facets[right], fcell[right], c_cell) if absorb else np.zeros(len(m))
    left = np.nonzero(coords[:, 0] == 0.0)[0]
    u0 = rng.standard_normal(len(m))
    u0[left] = 0.0
    dt = 0.9 * wr.critical_time_step(K, m)
    return wr.march(K, m, d, np.zeros(len(m)), dt, u0, rng.standard_normal(len(m)), 300, bc_dofs=left, bc_vals=np.zeros(len(left)))


def test_reference_energy_does_not_grow_with_an_absorbing_side():
    E = _absorbing_case(True)["energy"].sum(axis=1)
    E_closed = _absorbing_case(False)["energy"].sum(axis=1)
    print("absorbing side: E0 %.6g E_end %.6g largest increase %.3g; closed: ptp/max %.3g" % (
        E[0], E[-1], np.diff(E).max(), np.ptp(E_closed) / E_closed.max()))
    assert np.diff(E).max() <= 1e-14 * E[0]
    assert E[-1] < E_closed[-1]


def test_reference_damping_is_the_lumped_facet_measure_times_the_speed():
    coords, cells = wr.unit_square(4)
    facets, fcell = wr.boundary_facets(cells)
    assert len(facets) == 16 and abs(wr.facet_measure(coords, facets).sum() - 4.0) <= 1e-14
    d = wr.damping(coords, facets, fcell, 2.0)
    assert abs(d.sum() - 2.0 * 4.0) <= 1e-13 and abs(wr.lumped_mass(coords, cells).sum() - 1.0) <= 1e-14


# ---- the solver class without a device ---------------------------------------------------------------------------------------
def _case(**extra):
    from fenicssolver_amd.fem import UnitSquareMesh, FunctionSpace, CompiledSubDomain
    from fenicssolver_amd import SolverBase as SB
    mesh = UnitSquareMesh(4, 4)
    bcs = OrderedDict()
    bcs["left"] = {'boundary': CompiledSubDomain("near(x[0], side) && on_boundary", side=0.0), 'boundary_id': 1, 'type': 'Dirichlet', 'value': 0.0}
    bcs["right"] = {'boundary': CompiledSubDomain("near(x[0], side) && on_boundary", side=1.0), 'boundary_id': 2, 'type': 'absorbing'}
    s = copy.deepcopy(SB.default_case_settings)
    s['solver_name'] = 'WaveSolver'
    s['material'] = {'wave_speed': 1.0}
    s['material'].update(extra.pop('material', {}))
    s['function_space'] = FunctionSpace(mesh, "Lagrange", extra.pop('degree', 1))
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 0.05, 'ending_time': 0.5}
    s['solver_settings']['transient_settings'].update(extra.pop('transient_settings', {}))
    s.update(extra)
    return s


def _no_device(monkeypatch):
    from fenicssolver_amd import backend, _lib

    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(backend.DeviceMatrix, "__init__", refuse)


@pytest.mark.parametrize("extra, match", [
    ({'degree': 2}, "CG2"),
    ({'transient_settings': {'transient': False}}, "'transient': False"),
    ({'transient_settings': {'time_step': None, 'time_series': [0.0, 0.1, 0.3, 0.5]}}, "non-uniform"),
    ({'transient_settings': {'time_series': [0.0, 0.1, 0.3, 0.5]}}, "non-uniform"),
    ({'material': {'wave_speed': 0.0}}, "'wave_speed' must be positive"),
    ({'material': {'wave_speed': -2.0}}, "'wave_speed' must be positive"),
    ({'material': {'wave_speed': None}}, "'wave_speed' must be a positive number or a per-region dict"),
    ({'convective_velocity': (1.0, 0.0)}, "advection velocity"),
    ({'source_time_function': {'type': 'table', 'values': [1.0] * 9}}, "the table holds 9 values, the run needs 10"),
    ({'source_time_function': {'type': 'sine'}}, "source_time_function must be"),
])
def test_refusals_raise_before_any_device_call(monkeypatch, extra, match):
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    solver = WaveSolver(_case(**extra))
    with pytest.raises(SolverError, match=match):
        solver.solve()


def test_refusal_of_a_short_dirichlet_table(monkeypatch):
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    s = _case()
    s['boundary_conditions']['left'].update(value=1.0, time_function={'type': 'table', 'values': [1.0] * 10})
    with pytest.raises(SolverError, match="boundary 'left': time_function: the table holds 10 values, the run needs 11"):
        WaveSolver(s).solve()


def test_refusal_of_several_ranks(monkeypatch):
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    _no_device(monkeypatch)
    solver = WaveSolver(_case())
    monkeypatch.setattr(parallel, "world", lambda: (0, 2, None))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve()


def test_refusal_of_periodic_spaces(monkeypatch):
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import SubDomain, FunctionSpace, near

    class PeriodicY(SubDomain):
        def inside(self, x, on_boundary):
            return near(x[1], 0.0) and on_boundary

        def map(self, x, y):
            y[0], y[1] = x[0], x[1] - 1.0
    _no_device(monkeypatch)
    s = _case()
    s['function_space'] = FunctionSpace(s['function_space'].mesh(), "CG", 1, constrained_domain=PeriodicY())
    with pytest.raises(SolverError, match="WaveSolver: periodic spaces"):
        WaveSolver(s).solve()


def test_main_dispatches_the_solver_by_name(monkeypatch):
    import fenicssolver_amd as M
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    with pytest.raises(SolverError, match="CG2"):
        M.main(_case(degree=2))


def test_time_functions_tabulate_the_expected_values():
    from fenicssolver_amd.WaveSolver import WaveSolver, tabulate_time_function, ricker
    t = 0.05 * np.arange(11)
    f, t0 = 4.0, 0.3
    a = (math.pi * f * (t - t0)) ** 2
    assert np.array_equal(tabulate_time_function(None, t), np.ones(11))
    assert np.allclose(tabulate_time_function({'type': 'ricker', 'frequency': f, 'delay': t0}, t), (1 - 2 * a) * np.exp(-a), rtol=0, atol=1e-15)
    assert ricker(t0, f, t0) == 1.0 and np.allclose(ricker(t, f, t0), wr.ricker(t, f, t0), rtol=0, atol=1e-15)
    assert np.array_equal(tabulate_time_function({'type': 'table', 'values': list(range(20))}, t), np.arange(11.0))
    assert np.array_equal(tabulate_time_function(lambda x: 2.0 * x, t), 2.0 * t)
    # the solver: N = 10 steps; the load factor of step n at t_n (n < N), the Dirichlet factor at every time point (n <= N)
    s = _case(source_time_function={'type': 'ricker', 'frequency': f, 'delay': t0})
    s['boundary_conditions']['left'].update(value=2.0, time_function=lambda x: math.cos(x))
    solver = WaveSolver(s)
    assert solver.time_grid() == (0.0, 0.05, 10)
    sf, sg = solver.time_factors()
    assert sf.shape == (10,) and sg.shape == (11,)
    assert np.allclose(sf, wr.ricker(t[:10], f, t0), rtol=0, atol=1e-15) and np.allclose(sg, np.cos(t), rtol=0, atol=1e-15)


def test_dirichlet_sides_with_values_share_one_time_function():
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    s = _case()
    s['boundary_conditions']['left'].update(value=2.0, time_function=lambda x: math.cos(x))
    s['boundary_conditions']['right'] = dict(s['boundary_conditions']['right'], type='Dirichlet', value=1.0)
    with pytest.raises(SolverError, match="different time functions"):
        WaveSolver(s).time_factors()
    s['boundary_conditions']['right']['value'] = 0.0            # a homogeneous side takes any factor
    assert np.allclose(WaveSolver(s).time_factors()[1], np.cos(0.05 * np.arange(11)))


def test_receivers_snap_to_the_nearest_vertex():
    from fenicssolver_amd.WaveSolver import WaveSolver, nearest_vertices
    solver = WaveSolver(_case(receivers=[(0.26, 0.49), (0.9, 0.1), (0.5, 0.5)]))
    v = solver.snap_receivers()
    co = solver.mesh.coordinates()
    assert np.allclose(co[v], [(0.25, 0.5), (1.0, 0.0), (0.5, 0.5)])
    assert v.tolist() == [2 * 5 + 1, 4, 2 * 5 + 2] and solver.receiver_vertices is v
    # equally near vertices: the lowest index
    assert nearest_vertices(co, [(0.125, 0.0)]).tolist() == [0]


def test_initial_fields_take_numbers_expressions_and_nodal_arrays():
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    s = _case(initial_velocity=np.arange(25.0))
    s['initial_values'] = {'displacement': 'sin(pi*x[0])*x[1]'}
    solver = WaveSolver(s)
    u0, v0 = solver.initial_fields()
    co = solver.mesh.coordinates()
    assert np.allclose(u0, np.sin(math.pi * co[:, 0]) * co[:, 1], rtol=0, atol=1e-15) and np.array_equal(v0, np.arange(25.0))
    solver.settings['initial_velocity'] = 0.5
    assert np.array_equal(solver.initial_fields()[1], np.full(25, 0.5))
    solver.settings['initial_velocity'] = np.zeros(7)
    with pytest.raises(SolverError, match="initial_velocity holds 7 values"):
        solver.initial_fields()


def test_results_before_a_run_are_an_error():
    from fenicssolver_amd.WaveSolver import WaveSolver
    from fenicssolver_amd.SolverBase import SolverError
    solver = WaveSolver(_case())
    for call in (solver.velocity, solver.energy, solver.receiver_traces):
        with pytest.raises(SolverError, match="no run has been marched"):
            call()
