"""ElastodynamicsSolver without a device: the parameter map, the refusals, and the properties of the reference marcher
(tests/elastodynamics_reference.py) that the GPU tests lean on, on a random SPD pair."""
import copy
from collections import OrderedDict

import numpy as np
import pytest
import scipy.linalg

import elastodynamics_reference as er

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
EPS = 2.0 ** -52


# ---- the parameter map ---------------------------------------------------------------------------------------------------------
def test_parameter_map_of_the_spectral_radius():
    from fenicssolver_amd.ElastodynamicsSolver import generalized_alpha, unconditionally_stable, effective_coefficients
    assert generalized_alpha(1.0) == (0.5, 0.5, 0.25, 0.5)
    assert generalized_alpha(0.0) == (-1.0, 0.0, 1.0, 1.5)
    for r in np.linspace(0.0, 1.0, 21):
        am, af, beta, gamma = generalized_alpha(r)
        assert (am, af, beta, gamma) == er.parameters(r)
        assert gamma == 0.5 - am + af and beta == 0.25 * (1.0 - am + af) ** 2
        assert unconditionally_stable(am, af, beta, gamma)
    # Newmark average acceleration and HHT-alpha (alpha = 0.1) are inside the set, linear acceleration and central differences are not
    assert unconditionally_stable(0.0, 0.0, 0.25, 0.5)
    assert unconditionally_stable(0.0, 0.1, 0.3025, 0.6)
    assert not unconditionally_stable(0.0, 0.0, 1.0 / 6.0, 0.5)
    assert not unconditionally_stable(0.0, 0.0, 0.0, 0.5)
    assert not unconditionally_stable(0.3, 0.2, 0.25, 0.5)
    assert not unconditionally_stable(0.0, 0.6, 0.6, 0.5)
    assert not unconditionally_stable(0.0, 0.0, float('nan'), 0.5)
    # K_eff of the trapezoidal rule without damping: (2 / dt^2) M + K / 2, i.e. the classical 4 M / dt^2 + K up to the factor 1 - alpha_f
    assert effective_coefficients(0.5, 0.5, 0.25, 0.5, 0.1) == (0.5 / (0.25 * 0.1 * 0.1), 0.5)


# ---- the solver class without a device -------------------------------------------------------------------------------------------
def _case(**extra):
    from fenicssolver_amd.fem import UnitCubeMesh, VectorFunctionSpace, CompiledSubDomain, Constant
    from fenicssolver_amd import SolverBase as SB
    mesh = UnitCubeMesh(3, 2, 2)
    bcs = OrderedDict()
    bcs["left"] = {'boundary': CompiledSubDomain("near(x[0], side) && on_boundary", side=0.0), 'boundary_id': 1,
                   'type': 'Dirichlet', 'value': Constant((0.0, 0.0, 0.0))}
    bcs["right"] = {'boundary': CompiledSubDomain("near(x[0], side) && on_boundary", side=1.0), 'boundary_id': 2,
                    'type': 'stress', 'value': Constant((0.1, 0.0, 0.0))}
    bcs["left"].update(extra.pop('left', {}))
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': 200.0, 'poisson_ratio': 0.3, 'density': 8.0, 'thermal_expansion_coefficient': 0.0}
    s['material'].update(extra.pop('material', {}))
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", extra.pop('degree', 1))
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 0.5, 'ending_time': 2.0}
    s['solver_settings']['transient_settings'].update(extra.pop('transient_settings', {}))
    if 'dynamics' in extra:
        s['solver_settings']['dynamics_settings'] = extra.pop('dynamics')
    s.update(extra)
    return s


def _no_device(monkeypatch):
    from fenicssolver_amd import backend, _lib

    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(backend.DeviceMatrix, "__init__", refuse)


@pytest.mark.parametrize("extra, match", [
    ({'transient_settings': {'transient': False}}, "'transient': False"),
    ({'temperature_distribution': 350.0}, "temperature_distribution"),
    ({'point_source': {'value': 1.0}}, "point_source"),
    ({'surface_source': {'value': 1.0}}, "surface_source"),
    ({'material': {'density': 0.0}}, "'density' must be positive"),
    ({'material': {'density': -1.0}}, "'density' must be positive"),
    ({'dynamics': {'alpha_m': 0.0, 'alpha_f': 0.0, 'beta': 1.0 / 6.0, 'gamma': 0.5}}, "not unconditionally stable"),
    ({'dynamics': {'alpha_m': 0.3, 'alpha_f': 0.2, 'beta': 0.3, 'gamma': 0.5}}, "not unconditionally stable"),
    ({'dynamics': {'spectral_radius': 0.5, 'alpha_m': 0.0, 'alpha_f': 0.0, 'beta': 0.25, 'gamma': 0.5}}, "not both"),
    ({'dynamics': {'alpha_m': 0.0, 'beta': 0.25}}, "all four"),
    ({'dynamics': {'spectral_radius': 1.5}}, r"spectral_radius must lie in \[0, 1\]"),
    ({'dynamics': {'rayleigh_mass': -0.1}}, "must be >= 0"),
    ({'dynamics': {'rayleigh_stiffness': -0.1}}, "must be >= 0"),
    ({'dynamics': {'energy_freq': -1}}, "energy_freq"),
    ({'dynamics': {'damping': 1.0}}, "unknown key"),
    ({'load_time_function': {'type': 'table', 'values': [1.0, 1.0, 1.0]}}, "the table holds 3 values, the run needs 4"),
    ({'left': {'time_function': {'type': 'table', 'values': [1.0, 1.0, 1.0, 1.0]}}}, "the table holds 4 values, the run needs 5"),
    ({'transient_settings': {'time_step': 0.0}}, "do not make a run"),
    ({'initial_velocity': np.zeros(7)}, "holds 7 values"),
])
def test_refusals_raise_before_any_device_call(monkeypatch, extra, match):
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    solver = ElastodynamicsSolver(_case(**extra))
    with pytest.raises(SolverError, match=match):
        solver.solve()


def test_refusal_of_several_ranks(monkeypatch):
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    _no_device(monkeypatch)
    solver = ElastodynamicsSolver(_case())
    monkeypatch.setattr(parallel, "world", lambda: (0, 2, None))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve()


def test_refusal_of_periodic_spaces(monkeypatch):
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import SubDomain, VectorFunctionSpace, near

    class PeriodicY(SubDomain):
        def inside(self, x, on_boundary):
            return near(x[1], 0.0) and on_boundary

        def map(self, x, y):
            y[0], y[1], y[2] = x[0], x[1] - 1.0, x[2]
    _no_device(monkeypatch)
    s = _case()
    s['function_space'] = VectorFunctionSpace(s['function_space'].mesh(), "CG", 1, constrained_domain=PeriodicY())
    with pytest.raises(SolverError, match="ElastodynamicsSolver: periodic spaces"):
        ElastodynamicsSolver(s).solve()


def test_settings_are_read_on_the_host(monkeypatch):
    import importlib
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    _no_device(monkeypatch)
    main_mod = importlib.import_module('fenicssolver_amd.main')
    assert "ElastodynamicsSolver" in main_mod._SOLVERS
    ricker = {'type': 'ricker', 'frequency': 0.8, 'delay': 1.0}
    solver = ElastodynamicsSolver(_case(dynamics={'spectral_radius': 0.5, 'rayleigh_mass': 0.2, 'rayleigh_stiffness': 0.01, 'energy_freq': 2},
                                        load_time_function=ricker, left={'time_function': lambda t: 1.0 + t},
                                        initial_velocity=(0.0, "x[0]", 2.0), receivers=[(1.0, 1.0, 1.0), (0.02, 0.49, 0.0)]))
    assert solver.reference_load_sign is False
    p = solver.generalized_alpha_parameters()
    assert (p['alpha_m'], p['alpha_f'], p['beta'], p['gamma']) == er.parameters(0.5)
    assert (p['rayleigh_mass'], p['rayleigh_stiffness'], solver.energy_freq()) == (0.2, 0.01, 2)
    t = solver.time_points()
    assert np.array_equal(t, [0.0, 0.5, 1.0, 1.5, 2.0]) and np.array_equal(solver.step_lengths(), [0.5] * 4)
    sf, sg = solver.time_factors()
    from fenicssolver_amd.WaveSolver import ricker as ricker_fn
    # loads at t_n + (1 - alpha_f) dt; the homogeneous side with a time function sets the Dirichlet factor at the time points
    assert np.array_equal(sf, ricker_fn(t[:-1] + (1.0 - p['alpha_f']) * 0.5, 0.8, 1.0))
    assert np.array_equal(sg, 1.0 + t)
    u0, v0 = solver.initial_fields()
    co = solver.mesh.coordinates()
    assert not u0.any() and np.array_equal(v0.reshape(-1, 3), np.stack([np.zeros(len(co)), co[:, 0], np.full(len(co), 2.0)], axis=1))
    rv = solver.snap_receivers()
    assert np.allclose(co[rv], [(1.0, 1.0, 1.0), (0.0, 0.5, 0.0)])
    # a time series: the steps that start before the ending time
    s = _case(transient_settings={'time_step': None, 'time_series': [0.0, 0.1, 0.2, 0.4, 0.6], 'ending_time': 0.5})
    assert np.allclose(ElastodynamicsSolver(s).step_lengths(), [0.1, 0.1, 0.2, 0.2])


# ---- the reference marcher's own properties, on a random SPD pair ----------------------------------------------------------------
N_ = 12


def _spd_pair(seed=3):
    """(K, M, omega, Phi): random SPD K and M with moderate conditioning, the frequencies and M-orthonormal modes of the pair"""
    rng = np.random.default_rng(seed)
    Q1, _ = np.linalg.qr(rng.standard_normal((N_, N_)))
    Q2, _ = np.linalg.qr(rng.standard_normal((N_, N_)))
    K = Q1 @ np.diag(np.linspace(1.0, 30.0, N_)) @ Q1.T
    M = Q2 @ np.diag(np.linspace(0.5, 2.0, N_)) @ Q2.T
    K, M = 0.5 * (K + K.T), 0.5 * (M + M.T)
    lam, Phi = scipy.linalg.eigh(K, M)
    return K, M, np.sqrt(lam), Phi


def _roundoff_bound(K, M, par, dt, steps):
    """steps x n x eps x cond(A) with A the step matrix: every step solves with A once and adds n products' worth of rounding"""
    am, af, beta, gamma = par
    A = (1.0 - am) * M + (1.0 - af) * beta * dt * dt * K
    return steps * N_ * EPS * np.linalg.cond(A)


def test_reference_conserves_energy_for_the_trapezoidal_rule():
    K, M, om, Phi = _spd_pair()
    rng = np.random.default_rng(11)
    u0, v0 = rng.standard_normal(N_), rng.standard_normal(N_)
    dt, steps = 0.05, 200
    par = er.parameters(1.0)
    out = er.march(K, M, None, u0, v0, [dt] * steps, par)
    E = np.array([sum(er.energy(K, M, s['u'], s['v'])) for s in out])
    drift = np.abs(E - E[0]).max() / E[0]
    bound = _roundoff_bound(K, M, par, dt, steps)
    print("\nenergy drift over %d steps: %.2e (bound %.2e)" % (steps, drift, bound))
    assert drift <= bound
    # ... and a dissipative parameter set loses energy in every step
    out = er.march(K, M, None, u0, v0, [dt] * steps, er.parameters(0.5))
    E = np.array([sum(er.energy(K, M, s['u'], s['v'])) for s in out])
    assert E[-1] < 0.999 * E[0]


@pytest.mark.parametrize("k", [0, 5, N_ - 1])
def test_reference_marches_a_single_mode_at_the_discrete_frequency(k):
    K, M, om, Phi = _spd_pair()
    dt, steps = 0.07, 50
    par = er.parameters(1.0)
    out = er.march(K, M, None, Phi[:, k], np.zeros(N_), [dt] * steps, par)
    oh = er.discrete_frequency(om[k], dt)
    err = max(np.abs(s['u'] - Phi[:, k] * np.cos(oh * n * dt)).max() for n, s in enumerate(out)) / np.abs(Phi[:, k]).max()
    bound = _roundoff_bound(K, M, par, dt, steps)
    print("\nmode %d: largest deviation from phi cos(omega_h n dt): %.2e (bound %.2e)" % (k, err, bound))
    assert err <= bound


@pytest.mark.parametrize("rho_inf", [1.0, 0.8, 0.0])
def test_reference_is_second_order_for_a_forced_damped_run(rho_inf):
    K, M, om, Phi = _spd_pair()
    rng = np.random.default_rng(5)
    F, u0, v0 = rng.standard_normal(N_), rng.standard_normal(N_), rng.standard_normal(N_)
    par = er.parameters(rho_inf)
    T = 1.0

    def final(nsteps):
        dt = T / nsteps
        tm = dt * np.arange(nsteps) + (1.0 - par[1]) * dt
        return er.march(K, M, F, u0, v0, [dt] * nsteps, par, eta_m=0.3, eta_k=0.01, sf=np.cos(3.0 * tm), sf0=1.0)[-1]['u']
    us = [final(n) for n in (100, 200, 400, 800)]
    e = [np.abs(us[i] - us[i + 1]).max() for i in range(3)]
    ratios = [e[0] / e[1], e[1] / e[2]]
    print("\nrho_inf = %g: differences of successive halvings %s, ratios %s" % (rho_inf, ["%.2e" % x for x in e], ["%.3f" % r for r in ratios]))
    # second order: the difference of two successive halvings falls by 4; the next term of the expansion moves the ratio by O(dt)
    assert all(3.8 <= r <= 4.2 for r in ratios)


def test_reference_dirichlet_rows_follow_their_values_and_the_balance_holds():
    """the partitioned marcher against the balance equation it was written from, with a moving Dirichlet set"""
    K, M, om, Phi = _spd_pair()
    rng = np.random.default_rng(9)
    F, u0, v0 = rng.standard_normal(N_), rng.standard_normal(N_), rng.standard_normal(N_)
    par = am, af, beta, gamma = er.parameters(0.6)
    dofs, g = [2, 7, 2], [5.0, -0.4, 0.3]           # dof 2 named twice: the last value holds
    dt, steps = 0.1, 6
    sf, sg = 1.0 + 0.1 * np.arange(steps), np.cos(0.3 * np.arange(steps + 1))
    out = er.march(K, M, F, u0, v0, [dt] * steps, par, eta_m=0.2, eta_k=0.02, sf=sf, sf0=1.0, dofs=dofs, g=g, sg=sg)
    C = 0.2 * M + 0.02 * K
    free = np.setdiff1d(np.arange(N_), dofs)
    worst = 0.0
    for n in range(steps):
        s0, s1 = out[n], out[n + 1]
        assert s1['u'][2] == 0.3 * sg[n + 1] and s1['u'][7] == -0.4 * sg[n + 1]
        mid = {k: (1.0 - (am if k == 'a' else af)) * s1[k] + (am if k == 'a' else af) * s0[k] for k in 'uva'}
        res = M @ mid['a'] + C @ mid['v'] + K @ mid['u'] - sf[n] * F
        scale = np.abs(M @ mid['a']).max() + np.abs(K @ mid['u']).max()
        worst = max(worst, np.abs(res[free]).max() / scale)
        # the Newmark updates hold on every row
        ut = s0['u'] + dt * s0['v'] + dt * dt * (0.5 - beta) * s0['a']
        assert np.allclose(s1['u'], ut + beta * dt * dt * s1['a'], rtol=0, atol=1e-12 * np.abs(s1['u']).max())
    print("\nbalance residual on the free rows: %.2e" % worst)
    assert worst <= 100 * N_ * EPS
