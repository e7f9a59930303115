"""PlasticitySolver on the host side (no GPU): the numpy reference (tests/plasticity_reference.py) pinned by its own consistent
tangent against central differences, the yield surface and the uniaxial closed form; the refusals; the form; the main() dispatch."""
import copy
from collections import OrderedDict

import numpy as np
import pytest

import plasticity_reference as pr

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}


def _random_states(rng, n, d):
    """strains around the yield strain sy / (2 mu) ~ 2.6e-3 of the material below, with an admissible history"""
    eps = np.zeros((n, 3, 3))
    a = (1.6e-3 if d == 2 else 1.0e-3) * rng.standard_normal((n, d, d))
    eps[:, :d, :d] = 0.5 * (a + np.transpose(a, (0, 2, 1)))
    b = 5e-4 * rng.standard_normal((n, 3, 3))
    ep = 0.5 * (b + np.transpose(b, (0, 2, 1)))
    ep -= np.trace(ep, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3.0
    p = 2e-3 * rng.random(n)
    return eps, ep, p


MAT = (80.0, 120.0, 0.4, 15.0)          # mu, lambda, sigma_y, H


@pytest.mark.parametrize("d", [2, 3])
@pytest.mark.parametrize("H", [0.0, 15.0])
def test_consistent_tangent_matches_central_differences_of_the_stress(d, H):
    rng = np.random.default_rng(11 + d)
    mat = MAT[:3] + (H,)
    eps, ep, p = _random_states(rng, 40, d)
    sig, _, _, f, D = pr.return_map(eps, ep, p, *mat)
    keep = np.abs(f) > 1e-3 * mat[2]                 # away from the kink of sigma(eps) at f = 0
    assert (f[keep] > 0).sum() >= 5 and (f[keep] < 0).sum() >= 5
    h = 1e-7
    fd = np.zeros_like(D)
    for k in range(3):
        for l in range(3):
            de = np.zeros((3, 3))
            de[k, l] += 0.5 * h
            de[l, k] += 0.5 * h
            sp = pr.return_map(eps + de, ep, p, *mat, tangent=False)[0]
            sm = pr.return_map(eps - de, ep, p, *mat, tangent=False)[0]
            fd[:, :, :, k, l] = (sp - sm) / (2 * h)
    err = np.abs(fd - D)[keep].max() / np.abs(D).max()
    assert err < 1e-7, err


@pytest.mark.parametrize("H", [0.0, 15.0])
def test_returned_stress_lies_on_the_yield_surface(H):
    rng = np.random.default_rng(5)
    mat = MAT[:3] + (H,)
    eps, ep, p = _random_states(rng, 200, 3)
    sig, ep1, p1, f, _ = pr.return_map(eps, ep, p, *mat)
    y = f > 0
    assert y.sum() > 20 and (~y).sum() > 20
    q = pr.von_mises(sig)
    assert np.abs(q[y] - (mat[2] + H * p1[y])).max() < 1e-13 * mat[2]
    assert np.all(q[~y] <= mat[2] + H * p[~y])
    assert np.array_equal(ep1[~y], ep[~y]) and np.array_equal(p1[~y], p[~y])
    assert np.abs(np.trace(ep1, axis1=1, axis2=2)).max() < 1e-17 + 1e-15 * np.abs(ep1).max()
    assert np.all(p1 >= p)


def uniaxial_problem(d=3, n=(2, 2, 2), L=1.0):
    """box with roller planes on x = 0, y = 0 (, z = 0) and a prescribed u_x on x = L"""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point
    mesh = BoxMesh(Point(0, 0, 0), Point(L, L, L), *n) if d == 3 else RectangleMesh(Point(0, 0), Point(L, L), *n[:2])
    co = mesh.coordinates()[:, :d]
    fixed = [np.nonzero(np.abs(co[:, k]) < 1e-12)[0] * d + k for k in range(d)]
    pull = np.nonzero(np.abs(co[:, 0] - L) < 1e-12)[0] * d
    return mesh, co, np.concatenate(fixed + [pull]), sum(len(f) for f in fixed)


def test_reference_newton_follows_the_uniaxial_closed_form():
    E, nu, sy, H = 200.0, 0.3, 0.5, 20.0
    mu, lmbda = E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))
    mesh, co, dofs, nfix = uniaxial_problem()
    ey = sy / E
    path = [0.5 * ey, 1.5 * ey, 3.0 * ey, 2.5 * ey]                       # elastic, past yield, further, partial unloading
    loads = [(np.zeros(co.size), dofs, np.concatenate([np.zeros(nfix), np.full(len(dofs) - nfix, e)])) for e in path]
    steps = pr.solve_steps(co, mesh.cells(), (mu, lmbda, sy, H), loads, rtol=1e-12, atol=1e-14)
    exact = pr.uniaxial(path, E, nu, sy, H)
    Et = E * H / (E + H)
    assert abs(exact[2][0] - (sy + Et * (path[2] - ey))) < 1e-14 and exact[3][1] == exact[2][1]
    for st, (s, p, lat) in zip(steps, exact):
        sig = st["sigma"]
        assert np.abs(sig[:, 0, 0] - s).max() < 1e-11 * sy
        other = sig.copy()
        other[:, 0, 0] = 0.0
        assert np.abs(other).max() < 1e-11 * sy
        assert np.abs(st["p"] - p).max() < 1e-12
        eps = pr.strains(co, mesh.cells(), st["u"])[0]
        assert np.abs(eps[:, 1, 1] - lat).max() < 1e-12 and np.abs(eps[:, 2, 2] - lat).max() < 1e-12
        assert st["iterations"] <= 8


# ---- the solver class without a device ---------------------------------------------------------------------------------------
def _case(**extra):
    from fenicssolver_amd.fem import UnitCubeMesh, VectorFunctionSpace, CompiledSubDomain, Constant
    from fenicssolver_amd import SolverBase as SB
    mesh = UnitCubeMesh(3, 2, 2)
    bcs = OrderedDict()
    bcs["left"] = {'boundary': CompiledSubDomain("near(x[0], side) && on_boundary", side=0.0), 'boundary_id': 1,
                   'type': 'Dirichlet', 'value': Constant((0.0, 0.0, 0.0))}
    bcs["right"] = {'boundary': CompiledSubDomain("near(x[0], side) && on_boundary", side=1.0), 'boundary_id': 2,
                    'type': 'force', 'value': (0.1, 0.0, 0.0)}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': 200.0, 'poisson_ratio': 0.3, 'density': 800,
                     'thermal_expansion_coefficient': 2e-6, 'yield_stress': 0.5, 'hardening_modulus': 20.0}
    s['material'].update(extra.pop('material', {}))
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", extra.pop('degree', 1))
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
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
    ({'temperature_distribution': 350.0}, "temperature_distribution"),
    ({'point_source': {'value': 1.0}}, "point_source"),
    ({'surface_source': {'value': 1.0}}, "surface_source"),
    ({'material': {'yield_stress': None}}, "yield_stress' is required"),
    ({'material': {'yield_stress': 0.0}}, "yield_stress' must be positive"),
    ({'material': {'yield_stress': -1.0}}, "yield_stress' must be positive"),
    ({'material': {'hardening_modulus': -1.0}}, "hardening_modulus"),
    ({'material': {'poisson_ratio': 0.5}}, "poisson_ratio"),
])
def test_refusals_raise_before_any_device_call(monkeypatch, extra, match):
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    solver = PlasticitySolver(_case(**extra))
    with pytest.raises(SolverError, match=match):
        solver.solve()


def test_missing_yield_stress_key_is_refused(monkeypatch):
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    s = _case()
    del s['material']['yield_stress']
    with pytest.raises(SolverError, match="yield_stress' is required"):
        PlasticitySolver(s).solve()


def test_refusal_of_several_ranks(monkeypatch):
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    _no_device(monkeypatch)
    solver = PlasticitySolver(_case())
    monkeypatch.setattr(parallel, "world", lambda: (0, 2, None))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve()


def test_refusal_of_periodic_spaces(monkeypatch):
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
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
    with pytest.raises(SolverError, match="PlasticitySolver: periodic spaces"):
        PlasticitySolver(s).solve()


def test_form_carries_the_material_and_the_loads_with_their_physical_sign():
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.fem import Constant, MeshFunction
    from fenicssolver_amd import forms
    s = _case(body_source=Constant((0.0, -0.5, 0.0)))
    solver = PlasticitySolver(s)
    solver.init_solver()
    F, bcs = solver.generate_form(0, None, None, solver.w_current, solver.w_prev)
    assert isinstance(F, forms.PlasticForm) and F.describe()["type"] == "plasticity"
    assert F.body_force == (0.0, -0.5, 0.0) and np.allclose(F.tractions[0].g, (0.1, 0.0, 0.0))
    mu, lmbda = 200.0 / 2.6, 200.0 * 0.3 / (1.3 * 0.4)
    assert np.allclose(F.material_spec(), (mu, lmbda, 0.5, 20.0), rtol=1e-15) and not F.cellwise()
    # hardening defaults to 0; per-region values become per-cell arrays in the caller's cell order
    s2 = _case(material={'hardening_modulus': None,
                         'yield_stress': {'a': {'subdomain_id': 1, 'value': 0.5}, 'b': {'subdomain_id': 2, 'value': 0.8}}})
    solver2 = PlasticitySolver(s2)
    mesh = solver2.mesh
    sub = MeshFunction("size_t", mesh, 3)
    sub.array()[:] = np.where(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1)[:, 0] < 0.5, 1, 2)
    solver2.subdomains = sub
    solver2.init_solver()
    F2, _ = solver2.generate_form(0, None, None, solver2.w_current, solver2.w_prev)
    kind, arr = F2.material_spec()
    assert kind == "cell" and arr.shape == (mesh.num_cells(), 4)
    assert np.array_equal(arr[:, 2], np.where(sub.array() == 1, 0.5, 0.8)) and np.all(arr[:, 3] == 0.0) and np.all(arr[:, 0] == arr[0, 0])


def test_main_dispatches_to_the_plasticity_solver(monkeypatch):
    import importlib
    main_mod = importlib.import_module('fenicssolver_amd.main')
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    seen = []
    monkeypatch.setattr(PlasticitySolver, "solve", lambda self: seen.append(type(self).__name__))
    monkeypatch.setattr(PlasticitySolver, "plot", lambda self: None)
    s = _case()
    s['solver_name'] = 'PlasticitySolver'
    solver = main_mod.main(s)
    assert seen == ['PlasticitySolver'] and isinstance(solver, PlasticitySolver)
    assert "PlasticitySolver" in main_mod._SOLVERS
