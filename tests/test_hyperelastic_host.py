"""NonlinearElasticitySolver on the host side (no GPU): the numpy element against finite differences and the linear oracle, the
exact uniaxial state, the refusals, CompiledSubDomain and the main() dispatch."""
import copy
from collections import OrderedDict

import numpy as np
import pytest

import hyperelastic_reference as hr
from oracle import fem_oracle as fo

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}


def _random_cell(rng, d):
    X = np.eye(d + 1, d, -1) + 0.1 * rng.standard_normal((d + 1, d))
    U = 0.08 * rng.standard_normal((d + 1, d))
    return X, U


@pytest.mark.parametrize("d", [2, 3])
def test_element_derivatives_match_central_differences(d):
    rng = np.random.default_rng(7 + d)
    mu, lmbda = 1.3, 2.1
    for _ in range(5):
        X, U = _random_cell(rng, d)
        e0, f, K, J = hr.element(X, U, mu, lmbda)
        assert J > 0
        h = 1e-6
        fd_f = np.zeros_like(f)
        fd_K = np.zeros_like(K)
        for b in range(d + 1):
            for k in range(d):
                Up, Um = U.copy(), U.copy()
                Up[b, k] += h
                Um[b, k] -= h
                ep, fp, _, _ = hr.element(X, Up, mu, lmbda)
                em, fm, _, _ = hr.element(X, Um, mu, lmbda)
                fd_f[b, k] = (ep - em) / (2 * h)
                fd_K[:, :, b, k] = (fp - fm) / (2 * h)
        assert np.abs(fd_f - f).max() <= 1e-7 * np.abs(f).max()
        assert np.abs(fd_K - K).max() <= 1e-7 * np.abs(K).max()


def test_element_at_identity_is_the_linear_oracle():
    rng = np.random.default_rng(3)
    E, nu = 7.0, 0.3
    mu, lmbda = fo.lame(E, nu)
    for _ in range(4):
        X, _ = _random_cell(rng, 3)
        _, f, K, _ = hr.element(X, np.zeros((4, 3)), mu, lmbda)
        Ke = fo.p1_elasticity_local(X, np.arange(4)[None, :], E, nu)[0]
        assert np.abs(f).max() == 0.0
        assert np.allclose(K.reshape(12, 12), Ke, rtol=1e-13, atol=1e-13 * np.abs(Ke).max())


@pytest.mark.parametrize("d", [2, 3])
def test_exact_uniaxial_state_satisfies_the_discrete_equations(d):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point
    mu, lmbda = 1.0, 1.5
    L = 2.0
    mesh = BoxMesh(Point(0, 0, 0), Point(L, L, L), 3, 3, 3) if d == 3 else RectangleMesh(Point(0, 0), Point(L, L), 4, 4)
    co, ce = mesh.coordinates()[:, :d], mesh.cells()
    s = 1.3
    t = hr.exact_stretch_t(s, mu, lmbda, d)
    Fm = np.diag([s] + [t] * (d - 1))
    u = (co @ (Fm - np.eye(d)).T).ravel()
    _, f, _, J = hr.assemble(co, ce, u, mu, lmbda)
    f = f.reshape(-1, d)
    inner = np.all((co > 1e-12) & (co < L - 1e-12), axis=1)
    assert np.abs(f[inner]).max() < 1e-12
    # free lateral faces (y = L, z = L) carry no force normal to them; the x = L face carries P11 L^(d-1)
    right = np.abs(co[:, 0] - L) < 1e-12
    assert abs(f[right, 0].sum() - hr.first_pk_11(s, t, mu, lmbda, d) * L ** (d - 1)) < 1e-11
    top = np.abs(co[:, 1] - L) < 1e-12
    assert abs(f[top, 1].sum()) < 1e-11


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
    s['material'] = {'name': 'rubber', 'elastic_modulus': 10.0, 'poisson_ratio': 0.3, 'density': 800,
                     'thermal_expansion_coefficient': 2e-6}
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
])
def test_refusals_raise_before_any_device_call(monkeypatch, extra, match):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    solver = NonlinearElasticitySolver(_case(**extra))
    with pytest.raises(SolverError, match=match):
        solver.solve()


def test_refusal_of_several_ranks(monkeypatch):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    _no_device(monkeypatch)
    solver = NonlinearElasticitySolver(_case())
    monkeypatch.setattr(parallel, "world", lambda: (0, 2, None))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve()


def test_refusal_of_periodic_spaces(monkeypatch):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
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
    with pytest.raises(SolverError, match="NonlinearElasticitySolver: periodic spaces"):
        NonlinearElasticitySolver(s).solve()


def test_refusal_of_unsupported_boundary_type(monkeypatch):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    s = _case()
    s['boundary_conditions']['right']['type'] = 'symmetry'
    with pytest.raises(SolverError, match="symmetry"):
        NonlinearElasticitySolver(s).solve()


def test_form_loads_have_the_physical_sign_and_surface_source_semantics():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.fem import Constant
    from fenicssolver_amd import forms
    s = _case(body_source=Constant((0.0, -0.5, 0.0)), surface_source={'value': Constant(0.1), 'direction': Constant((1, 0, 0))})
    solver = NonlinearElasticitySolver(s)
    solver.init_solver()
    F, bcs = solver.generate_form(0, None, None, solver.w_current, solver.w_prev)
    assert isinstance(F, forms.HyperelasticForm)
    assert F.body_force == (0.0, -0.5, 0.0)
    assert [type(t).__name__ for t in F.tractions] == ['FacetLoad']          # the directed surface_source adds nothing
    assert np.allclose(F.tractions[0].g, (0.1, 0.0, 0.0))
    assert F.describe()["type"] == "hyperelasticity"
    # without a direction: the normal traction on the whole exterior boundary - zero net force on a closed surface
    solver2 = NonlinearElasticitySolver(_case(surface_source={'value': Constant(0.2)}))
    solver2.init_solver()
    F2, _ = solver2.generate_form(0, None, None, solver2.w_current, solver2.w_prev)
    ss = [t for t in F2.tractions if isinstance(t, forms.NodalLoad)]
    assert len(ss) == 1
    tot = np.zeros(3)
    np.add.at(tot, ss[0].dofs % 3, ss[0].values)
    assert np.abs(tot).max() < 1e-12 and np.abs(ss[0].values).sum() > 0.1
    # the linear class keeps refusing surface_source
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    lin = LinearElasticitySolver(_case(surface_source={'value': Constant(0.2)}))
    lin.init_solver()
    with pytest.raises(SolverError, match="surface_source"):
        lin.generate_form(0, None, None, lin.w_current, lin.w_prev)


def test_compiled_subdomain_marks_like_auto_subdomain():
    from fenicssolver_amd.fem import UnitCubeMesh, MeshFunction, CompiledSubDomain, AutoSubDomain, near
    mesh = UnitCubeMesh(4, 3, 3)
    a, b = MeshFunction("size_t", mesh, 2), MeshFunction("size_t", mesh, 2)
    a.array()[:] = 0
    b.array()[:] = 0
    CompiledSubDomain("near(x[0], side) && on_boundary", side=1.0).mark(a, 3)
    AutoSubDomain(lambda x, on_boundary: near(x[0], 1.0) and on_boundary).mark(b, 3)
    assert (a.array() == 3).sum() == 3 * 3 * 2          # the x = 1 face: 3 x 3 squares of two triangles
    assert np.array_equal(a.array(), b.array())
    c = CompiledSubDomain("near(x[0], side) && on_boundary", side=0.0)
    c.side = 1.0
    m = MeshFunction("size_t", mesh, 2)
    m.array()[:] = 0
    c.mark(m, 3)
    assert np.array_equal(m.array(), a.array())


def test_main_dispatches_to_the_nonlinear_solver(monkeypatch):
    import importlib
    main_mod = importlib.import_module('fenicssolver_amd.main')
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    seen = []
    monkeypatch.setattr(NonlinearElasticitySolver, "solve", lambda self: seen.append(type(self).__name__))
    monkeypatch.setattr(NonlinearElasticitySolver, "plot", lambda self: None)
    s = _case()
    s['solver_name'] = 'NonlinearElasticitySolver'
    solver = main_mod.main(s)
    assert seen == ['NonlinearElasticitySolver'] and isinstance(solver, NonlinearElasticitySolver)
