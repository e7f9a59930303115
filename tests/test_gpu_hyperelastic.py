"""NonlinearElasticitySolver and fs_assemble_hyperelastic on the MI355X: the tangent at u = 0 against the linear operator, the
kernels against the numpy reference (tests/hyperelastic_reference.py), exact finite-strain states (homogeneous stretch, rigid
rotation), the small-load limit, the reference example, the step cut-back and the configs[2] cantilever."""
import copy
import time
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sps

import hyperelastic_reference as hr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}


def _device(mesh, d):
    from fenicssolver_amd.fem import VectorFunctionSpace
    from fenicssolver_amd import backend
    backend.init()
    V = VectorFunctionSpace(mesh, "Lagrange", 1)
    return V, V.device()


def _csr(A):
    rp, ci, va, (nr, nc) = A.to_csr()
    return sps.csr_matrix((va, ci, rp), shape=(nr, nc))


def _box(n=(4, 3, 3), p1=(1.0, 0.8, 0.6)):
    from fenicssolver_amd.fem import BoxMesh, Point
    return BoxMesh(Point(0, 0, 0), Point(*p1), *n)


def _rect(n=(6, 5), p1=(1.0, 0.7)):
    from fenicssolver_amd.fem import RectangleMesh, Point
    return RectangleMesh(Point(0, 0), Point(*p1), *n)


def _smooth_u(co, d, amp=0.05):
    x = co[:, :d]
    u = np.stack([amp * np.sin(1.3 * x[:, 0] + 0.7 * x[:, 1]) + 0.3 * amp * x[:, 1] ** 2,
                  amp * np.cos(0.9 * x[:, 0] - 1.1 * x[:, 1])] + ([amp * x[:, 0] * x[:, 2] + 0.5 * amp * np.sin(2 * x[:, 2])] if d == 3 else []),
                 axis=1)
    return u.ravel()


@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("cellwise", [False, True])
def test_tangent_at_zero_is_the_linear_operator_bit_for_bit(d, cellwise):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh, d)
    nc = mesh.num_cells()
    mu, lmbda = 3.1, 4.7
    if cellwise:
        rng = np.random.default_rng(1)
        lame = ("cell", np.stack([mu * (1 + rng.random(nc)), lmbda * (1 + rng.random(nc))], axis=1))
    else:
        lame = (mu, lmbda)
    A = backend.DeviceMatrix(dV)
    A.assemble(lame=lame)
    K = backend.DeviceMatrix(dV)
    u = backend.DeviceVector(dV.n_local, np.zeros(dV.n_local))
    r = backend.DeviceVector(dV.n_owned)
    info = backend.assemble_hyperelastic(dV, u, lame, K=K, r=r, energy=True)
    assert info["n_inverted"] == 0 and info["first_inverted_cell"] == -1
    a, k = A.to_csr(), K.to_csr()
    assert np.array_equal(a[0], k[0]) and np.array_equal(a[1], k[1])
    assert np.array_equal(a[2], k[2])
    assert np.abs(r.get()).max() == 0.0
    area = mesh.coordinates().max(axis=0)[:d].prod()
    if d == 3:
        assert info["energy"] == 0.0
    elif not cellwise:                          # the reference's Identity(2) with "- 3": -mu/2 per unit area
        assert abs(info["energy"] + 0.5 * mu * area) < 1e-13 * mu * area


@pytest.mark.parametrize("d", [3, 2])
def test_per_cell_array_of_one_constant_gives_the_constant_bits(d):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh, d)
    u = backend.DeviceVector(dV.n_local, _smooth_u(mesh.coordinates(), d))
    mu, lmbda = 1.7, 2.9
    out = []
    for lame in ((mu, lmbda), ("cell", np.tile([mu, lmbda], (mesh.num_cells(), 1)))):
        K = backend.DeviceMatrix(dV)
        r = backend.DeviceVector(dV.n_owned)
        info = backend.assemble_hyperelastic(dV, u, lame, K=K, r=r, energy=True)
        out.append((K.to_csr()[2], r.get(), info["energy"]))
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1]) and out[0][2] == out[1][2]
    # per-cell pairs are checked like the constants
    bad = np.tile([mu, lmbda], (mesh.num_cells(), 1))
    bad[3, 0] = 0.0
    with pytest.raises(backend.BackendError, match="cell 3"):
        backend.assemble_hyperelastic(dV, u, ("cell", bad), r=backend.DeviceVector(dV.n_owned))


@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("cellwise", [False, True])
def test_add_accumulates_onto_the_target_bit_for_bit(d, cellwise):
    """Tangent and force with add=True equal y + x bit for bit (one fp64 addition per entry): y the target's content (the linear
    operator in the matrix, known values in the vector), x the result with add=False.  3 x 3 x 4 box: 216 cells, 80 nodes (a partial
    second slice); 5 x 4 square: 40 cells, 30 nodes."""
    from fenicssolver_amd import backend
    mesh = _box((3, 3, 4)) if d == 3 else _rect((5, 4))
    V, dV = _device(mesh, d)
    nc = mesh.num_cells()
    assert (nc, mesh.num_vertices()) == ((216, 80) if d == 3 else (40, 30))
    rng = np.random.default_rng(80 + d)
    lame = ("cell", np.stack([3.1 * (1 + rng.random(nc)), 4.7 * (1 + rng.random(nc))], axis=1)) if cellwise else (3.1, 4.7)
    u = backend.DeviceVector(dV.n_local, _smooth_u(mesh.coordinates(), d))
    K, r = backend.DeviceMatrix(dV), backend.DeviceVector(dV.n_owned)
    info = backend.assemble_hyperelastic(dV, u, lame, K=K, r=r)
    assert info["n_inverted"] == 0
    xk, xr = K.to_csr()[2], r.get()
    y = 0.37 + rng.standard_normal(dV.n_owned)
    Ka, ra = backend.DeviceMatrix(dV), backend.DeviceVector(dV.n_owned, y)
    Ka.assemble(lame=(3.1, 4.7))
    yk = Ka.to_csr()[2]
    backend.assemble_hyperelastic(dV, u, lame, K=Ka, r=ra, add=True)
    assert np.array_equal(Ka.to_csr()[2], yk + xk)
    assert np.array_equal(ra.get(), y + xr)


@pytest.mark.parametrize("d", [3, 2])
def test_kernels_match_the_host_reference_and_are_deterministic(d):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh, d)
    co, ce = mesh.coordinates(), mesh.cells()
    uh = _smooth_u(co, d)
    rng = np.random.default_rng(5)
    mu = 1.0 + rng.random(mesh.num_cells())
    lm = 2.0 + rng.random(mesh.num_cells())
    lame = ("cell", np.stack([mu, lm], axis=1))
    e_h, f_h, K_h, J_h = hr.assemble(co[:, :d], ce, uh, mu, lm)
    assert J_h.min() > 0.5
    u = backend.DeviceVector(dV.n_local, uh)
    outs = []
    for _ in range(2):
        K = backend.DeviceMatrix(dV)
        r = backend.DeviceVector(dV.n_owned)
        info = backend.assemble_hyperelastic(dV, u, lame, K=K, r=r, energy=True)
        outs.append((K.to_csr()[2], r.get(), info["energy"]))
        Kd = _csr(K)
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]
    assert abs(Kd - K_h).max() <= 1e-12 * abs(K_h).max()
    assert np.abs(outs[0][1] - f_h).max() <= 1e-12 * np.abs(f_h).max()
    assert abs(outs[0][2] - e_h) <= 1e-12 * abs(e_h)


def test_tangent_and_force_are_the_derivatives_of_the_device_energy():
    from fenicssolver_amd import backend
    mesh = _box((3, 3, 2))
    V, dV = _device(mesh, 3)
    uh = _smooth_u(mesh.coordinates(), 3, amp=0.1)
    lame = (1.7, 2.9)
    rng = np.random.default_rng(11)

    def state(x):
        K = backend.DeviceMatrix(dV)
        r = backend.DeviceVector(dV.n_owned)
        info = backend.assemble_hyperelastic(dV, backend.DeviceVector(dV.n_local, x), lame, K=K, r=r, energy=True)
        return _csr(K), r.get(), info["energy"]
    K, f, _ = state(uh)
    h = 1e-6
    for _ in range(3):
        w = rng.standard_normal(uh.size)
        _, fp, ep = state(uh + h * w)
        _, fm, em = state(uh - h * w)
        assert np.abs((fp - fm) / (2 * h) - K @ w).max() <= 1e-6 * np.abs(K @ w).max()
        assert abs((ep - em) / (2 * h) - f @ w) <= 1e-6 * abs(f @ w)


def _stretch_case(d, delta, L=1.0, n=None):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    mesh = BoxMesh(Point(0, 0, 0), Point(L, L, L), *(n or (4, 3, 3))) if d == 3 else RectangleMesh(Point(0, 0), Point(L, L), *(n or (6, 5)))
    free = [None] * d
    bcs = OrderedDict()
    def plane(k, v):
        return AutoSubDomain(lambda x: near(x[k], v))
    for k, name in enumerate("xyz"[:d]):
        val = list(free)
        val[k] = Constant(0.0)
        bcs["sym_" + name] = {'boundary': plane(k, 0.0), 'boundary_id': k + 1, 'type': 'Dirichlet', 'value': tuple(val)}
    val = list(free)
    val[0] = Constant(delta)
    bcs["pull"] = {'boundary': plane(0, L), 'boundary_id': 9, 'type': 'Dirichlet', 'value': tuple(val)}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'rubber', 'elastic_modulus': 10.0, 'poisson_ratio': 0.3, 'density': 1000,
                     'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-13, 'newton_solver': {'relative_tolerance': 1e-12}}
    return s, mesh


@pytest.mark.parametrize("d", [3, 2])
def test_exact_homogeneous_stretch(d):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd import backend
    L, delta = 1.0, 0.3
    s, mesh = _stretch_case(d, delta, L)
    solver = NonlinearElasticitySolver(s)
    u = solver.solve().vector()._values()
    mu, lmbda = solver.lame_parameters()
    sx = 1.0 + delta / L
    t = hr.exact_stretch_t(sx, mu, lmbda, d)
    co = mesh.coordinates()[:, :d]
    exact = (co @ (np.diag([sx] + [t] * (d - 1)) - np.eye(d)).T).ravel()
    assert np.abs(u - exact).max() < 1e-9
    assert solver.newton_iterations >= 2 and solver.newton_history[-1] < 1e-9 * solver.newton_history[0]
    dV = solver.function_space.device()
    r = backend.DeviceVector(dV.n_owned)
    backend.assemble_hyperelastic(dV, backend.DeviceVector(dV.n_local, exact), (mu, lmbda), r=r)
    f = r.get().reshape(-1, d)
    right = np.abs(co[:, 0] - L) < 1e-12
    assert abs(f[right, 0].sum() - hr.first_pk_11(sx, t, mu, lmbda, d) * L ** (d - 1)) < 1e-10


@pytest.mark.parametrize("ramp", ["sequence", "callable"])
def test_load_stepping_follows_the_exact_stretch_at_every_step(ramp):
    """transient settings = quasi-static load steps: the pull at x = L ramps 0.1, 0.2, 0.3, 0.4 over four steps (a per-step
    sequence, or a callable of time: step k runs at time start + (k - 1) dt, as in the reference's TimeGrid); each step starts from
    the previous solution and must reach that step's exact homogeneous stretch."""
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    s, mesh = _stretch_case(3, 0.0)
    pull = [0.1, 0.2, 0.3, 0.4] if ramp == "sequence" else (lambda t: 0.1 * (t + 2.0))
    s['boundary_conditions']['pull']['value'] = (pull, None, None)
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 1.0, 'ending_time': 4.0}
    solver = NonlinearElasticitySolver(s)
    mu, lmbda = solver.lame_parameters()
    co = mesh.coordinates()
    seen = []
    solve_form = solver.solve_form

    def checked(F, u_, bcs):
        start = u_.vector()._values().copy()
        out = solve_form(F, u_, bcs)
        delta = float(np.unique(bcs[-1].values)[0])
        t = hr.exact_stretch_t(1.0 + delta, mu, lmbda, 3)
        exact = (co @ (np.diag([1.0 + delta, t, t]) - np.eye(3)).T).ravel()
        seen.append((delta, np.abs(out.vector()._values() - exact).max(), np.abs(start).max()))
        return out
    solver.solve_form = checked
    solver.solve()
    assert [round(x[0], 12) for x in seen] == [0.1, 0.2, 0.3, 0.4]
    assert max(x[1] for x in seen) < 1e-9
    assert seen[0][2] == 0.0 and all(x[2] > 0.0 for x in seen[1:])          # later steps start from the previous solution


def test_rigid_rotation_is_reproduced_exactly():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.fem import UnitCubeMesh, VectorFunctionSpace, AutoSubDomain, Expression
    from fenicssolver_amd import SolverBase as SB, backend
    mesh = UnitCubeMesh(4, 4, 3)
    th = np.pi / 6
    code = ("0.0", "(x[1] - 0.5)*(cos(th) - 1) - (x[2] - 0.5)*sin(th)", "(x[1] - 0.5)*sin(th) + (x[2] - 0.5)*(cos(th) - 1)")
    bcs = OrderedDict()
    bcs["all"] = {'boundary': AutoSubDomain(lambda x, on_boundary: on_boundary), 'boundary_id': 1, 'type': 'Dirichlet',
                  'value': Expression(code, th=th, degree=1)}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'rubber', 'elastic_modulus': 10.0, 'poisson_ratio': 0.3, 'density': 1000, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-13, 'newton_solver': {'relative_tolerance': 1e-12}}
    solver = NonlinearElasticitySolver(s)
    co = mesh.coordinates()
    R = np.array([[1, 0, 0], [0, np.cos(th), -np.sin(th)], [0, np.sin(th), np.cos(th)]])
    exact = ((co - 0.5) @ (R - np.eye(3)).T).ravel()
    exact[0::3] = 0.0
    # the initial iterate (zero inside, the rotation on the boundary) has no inverted cell
    solver.init_solver()
    F, bc_list = solver.generate_form(0, None, None, solver.w_current, solver.w_prev)
    x0 = np.zeros(exact.size)
    dofs, vals = solver._bc_arrays(bc_list)
    x0[dofs] = vals
    assert hr.assemble(co, mesh.cells(), x0, *solver.lame_parameters())[3].min() > 0
    u = solver.solve().vector()._values()
    assert np.abs(u - exact).max() < 1e-9
    dV = solver.function_space.device()
    r = backend.DeviceVector(dV.n_owned)
    backend.assemble_hyperelastic(dV, backend.DeviceVector(dV.n_local, u), solver.lame_parameters(), r=r)
    assert np.abs(r.get()).max() < 1e-9


def _example_case(n, scale=1.0):
    """examples/test_nonlinear_elasticity.py through the drop-in API."""
    from fenicssolver_amd.fem import UnitCubeMesh, VectorFunctionSpace, CompiledSubDomain, Constant, Expression
    from fenicssolver_amd import SolverBase as SB
    mesh = UnitCubeMesh(*n)
    B = Constant((0.0, -0.5 * scale, 0.0))
    left = CompiledSubDomain("near(x[0], side) && on_boundary", side=0.0)
    right = CompiledSubDomain("near(x[0], side) && on_boundary", side=1.0)
    c = Constant((0.0, 0.0, 0.0))
    r = Expression(("scale*0.0",
                    "scale*(y0 + (x[1] - y0)*cos(theta) - (x[2] - z0)*sin(theta) - x[1])",
                    "scale*(z0 + (x[1] - y0)*sin(theta) + (x[2] - z0)*cos(theta) - x[2])"),
                   scale=0.5 * scale, y0=0.5, z0=0.5, theta=np.pi / 3, degree=2)
    bcs = OrderedDict()
    bcs["left"] = {'boundary': left, 'boundary_id': 1, 'type': 'Dirichlet', 'value': c}
    bcs["right"] = {'boundary': right, 'boundary_id': 2, 'type': 'Dirichlet', 'value': r}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'rubber', 'elastic_modulus': 10, 'poisson_ratio': 0.3, 'density': 800,
                     'thermal_expansion_coefficient': 2e-6}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['body_source'] = B
    s['surface_source'] = {'value': Constant(0.1), 'direction': Constant((1, 0.0, 0.0))}
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    return s, mesh


def test_reference_example_matches_the_host_newton():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    s, mesh = _example_case((8, 6, 6))
    solver = NonlinearElasticitySolver(s)
    u = solver.solve().vector()._values()
    mu, lmbda = solver.lame_parameters()
    co, ce = mesh.coordinates(), mesh.cells()
    # f_ext = int B.v dx: V/4 per cell and vertex
    vol = 1.0 / mesh.num_cells()
    f_ext = np.zeros(u.size)
    np.add.at(f_ext, (ce.astype(np.int64) * 3 + 1).ravel(), -0.5 * vol / 4.0)
    bcs = solver.generate_form(0, None, None, solver.w_prev, solver.w_prev)[1]
    dofs, vals = solver._bc_arrays(bcs)
    uh, hist = hr.newton(co, ce, mu, lmbda, f_ext, dofs, vals)
    assert np.abs(u - uh).max() <= 1e-9 * np.abs(uh).max()


def test_reference_example_converges_quadratically_with_full_steps():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    s, mesh = _example_case((24, 16, 16))
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-10}
    solver = NonlinearElasticitySolver(s)
    t0 = time.perf_counter()
    u = solver.solve().vector()._values()
    wall = time.perf_counter() - t0
    h = np.asarray(solver.newton_history) / solver.newton_history[0]
    print("\nreference example 24x16x16: %d Newton iterations, %.2f s, history %s, per-step (AMG set-up ms, solve ms) %s" % (
        solver.newton_iterations, wall, np.array2string(h, precision=2),
        [(round(x['amg_setup_ms'], 1), round(x['solve_ms'], 1)) for x in solver.newton_stats]))
    assert np.all(np.isfinite(u))
    assert all(step == 1.0 for step in solver.newton_steps)          # full Newton steps
    assert h[-1] < 1e-9
    for k in range(len(h) - 1):
        if h[k] < 1e-3:
            assert h[k + 1] <= 10.0 * h[k] ** 2 + 1e-10


def test_inverting_steps_are_cut_back_and_an_inverted_start_is_named():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    import scipy.sparse.linalg as spla
    # a soft cube clamped at x = 0 under a tip shear larger than half its modulus, in one load step: on the host, a full Newton
    # step inverts a cell (the same path the device takes from u = 0) and the halved steps converge
    T = 5.0
    mesh = BoxMesh(Point(0, 0, 0), Point(1, 1, 1), 4, 2, 2)
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'value': Constant((0.0, 0.0, 0.0))}
    bcs["shear"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 1.0)), 'boundary_id': 2, 'type': 'stress',
                    'value': Constant((0.0, 0.0, -T))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'rubber', 'elastic_modulus': 10.0, 'poisson_ratio': 0.3, 'density': 1000, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    solver = NonlinearElasticitySolver(s)
    mu, lmbda = solver.lame_parameters()
    co, ce = mesh.coordinates(), mesh.cells().astype(np.int64)
    fac = mesh.facets()[mesh.exterior_facets()].astype(np.int64)
    right = fac[np.all(np.abs(co[fac][:, :, 0] - 1.0) < 1e-12, axis=1)]
    p = co[right]
    area = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
    f_ext = np.zeros(co.size)
    np.add.at(f_ext, (right * 3 + 2).ravel(), np.repeat(-T * area / 3, 3))
    dofs = (np.nonzero(np.abs(co[:, 0]) < 1e-12)[0][:, None] * 3 + np.arange(3)).ravel()
    free = np.ones(co.size, dtype=bool)
    free[dofs] = False
    x, host_steps = np.zeros(co.size), []
    with np.errstate(invalid="ignore"):
        for _ in range(50):
            _, fi, K, _ = hr.assemble(co, ce, x, mu, lmbda)
            r = fi - f_ext
            r[~free] = 0.0
            if np.linalg.norm(r) < 1e-11 * np.linalg.norm(f_ext):
                break
            d = np.zeros(co.size)
            d[free] = -spla.spsolve(K[free][:, free].tocsc(), r[free])
            step = 1.0
            while hr.assemble(co, ce, x + step * d, mu, lmbda)[3].min() <= 0:
                step *= 0.5
            host_steps.append(step)
            x = x + step * d
    assert min(host_steps) < 1.0
    u = solver.solve().vector()._values()
    assert np.all(np.isfinite(u))
    assert min(solver.newton_steps) < 1.0                              # a step was cut back
    assert solver.newton_history[-1] < 1e-9 * solver.newton_history[0]
    assert np.abs(u - x).max() < 1e-8 * np.abs(x).max()
    # an initial iterate that is already inverted (the x = 1 face moved past the first cell layer): SolverError naming the cell
    s_bad, m_bad = _stretch_case(3, -0.8, n=(4, 2, 2))
    bad = NonlinearElasticitySolver(s_bad)
    with pytest.raises(SolverError, match=r"inverts \d+ cell\(s\), first cell \d+.*load in steps") as err:
        bad.solve()
    _assert_named_cell_inverted(str(err.value), bad, m_bad)


def _assert_named_cell_inverted(msg, solver, mesh):
    import re
    cell = int(re.search(r"first cell (\d+)", msg).group(1))
    dofs, vals = solver._bc_arrays(solver.generate_form(0, None, None, solver.w_prev, solver.w_prev)[1])
    x0 = np.zeros(mesh.num_vertices() * 3)
    x0[dofs] = vals
    with np.errstate(invalid="ignore"):
        J = hr.assemble(mesh.coordinates(), mesh.cells(), x0, *solver.lame_parameters())[3]
    assert J[cell] <= 0.0


def _xml_case(monkeypatch, renumber, pull=None):
    """tests/golden/data/mesh.xml (a 10 x 5 x 20 block) uploaded in file order or in locality order (FS_RENUMBER), E varying from cell
    to cell: clamped at z = 0, sheared at z = 20 (or pulled down by `pull`)."""
    import os
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.fem import Mesh, VectorFunctionSpace, AutoSubDomain, Constant, Expression, near
    from fenicssolver_amd import SolverBase as SB
    monkeypatch.setenv("FS_RENUMBER", "1" if renumber else "0")
    mesh = Mesh(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "mesh.xml"))
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'value': Constant((0.0, 0.0, 0.0))}
    if pull is None:
        bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 20.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': Constant((0.05, 0.0, 0.0))}
    else:
        bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 20.0)), 'boundary_id': 2, 'type': 'Dirichlet',
                      'value': Constant((0.0, 0.0, pull))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'rubber', 'elastic_modulus': Expression("10.0 + x[2]", degree=0), 'poisson_ratio': 0.3,
                     'density': 1000, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12, 'newton_solver': {'relative_tolerance': 1e-11}}
    return NonlinearElasticitySolver(s), mesh


def test_mesh_file_in_locality_order_gives_the_file_order_solution(monkeypatch):
    from fenicssolver_amd.SolverBase import SolverError
    out = []
    for renumber in (False, True):
        solver, mesh = _xml_case(monkeypatch, renumber)
        u = solver.solve().vector()._values().copy()
        assert (solver.function_space.localizer() is not None) == renumber
        out.append(u)
    assert np.abs(out[0]).max() > 1e-2
    assert np.abs(out[1] - out[0]).max() <= 1e-9 * np.abs(out[0]).max()
    # an inverted start on the renumbered mesh names the inverted cell in the FILE's numbering
    solver, mesh = _xml_case(monkeypatch, True, pull=-25.0)
    with pytest.raises(SolverError, match=r"first cell \d+") as err:
        solver.solve()
    assert solver.function_space.localizer() is not None
    _assert_named_cell_inverted(str(err.value), solver, mesh)


def test_per_region_material_matches_the_host_reference():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.fem import MeshFunction
    s, mesh = _example_case((6, 4, 4), scale=0.5)
    s['material']['elastic_modulus'] = {'soft': {'subdomain_id': 1, 'value': 5.0}, 'hard': {'subdomain_id': 2, 'value': 20.0}}
    solver = NonlinearElasticitySolver(s)
    co, ce = mesh.coordinates(), mesh.cells()
    sub = MeshFunction("size_t", mesh, 3)
    sub.array()[:] = np.where(co[ce.astype(np.int64)].mean(axis=1)[:, 0] < 0.5, 1, 2)
    solver.subdomains = sub
    u = solver.solve().vector()._values()
    mu, lmbda = solver.lame_parameters()
    vol = 1.0 / mesh.num_cells()
    f_ext = np.zeros(u.size)
    np.add.at(f_ext, (ce.astype(np.int64) * 3 + 1).ravel(), -0.25 * vol / 4.0)
    dofs, vals = solver._bc_arrays(solver.generate_form(0, None, None, solver.w_prev, solver.w_prev)[1])
    uh, _ = hr.newton(co, ce, mu, lmbda, f_ext, dofs, vals)
    assert np.abs(u - uh).max() <= 1e-9 * np.abs(uh).max()


def test_small_load_limit_is_the_linear_solution():
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    errs = []
    for sc in (1e-4, 1e-5):
        s, mesh = _example_case((6, 4, 4), scale=sc)
        s['surface_source'] = None
        nl = NonlinearElasticitySolver(copy.deepcopy(s)).solve().vector()._values()
        lin_solver = LinearElasticitySolver(s)
        lin_solver.reference_load_sign = False
        lin = lin_solver.solve().vector()._values()
        errs.append(np.abs(nl - lin).max() / np.abs(lin).max())
    assert errs[0] < 1e-3 and errs[1] < 0.2 * errs[0]


def test_configs2_cantilever_with_a_large_tip_load():
    """BASELINE configs[2]: 472 x 59 x 59 cantilever (5.11 M DOF), a tip load for a tip deflection of about 10 %."""
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    mesh = BoxMesh(Point(0, 0, 0), Point(8.0, 1.0, 1.0), 472, 59, 59)
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'value': Constant((0.0, 0.0, 0.0))}
    bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 8.0)), 'boundary_id': 2, 'type': 'stress',
                  'value': Constant((0.0, 0.0, -4.0e3))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'rubber', 'elastic_modulus': 1.0e7, 'poisson_ratio': 0.3, 'density': 1000, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-8, 'newton_solver': {'relative_tolerance': 1e-8}}
    s2 = copy.deepcopy(s)
    solver = NonlinearElasticitySolver(s)
    t0 = time.perf_counter()
    u = solver.solve().vector()._values().copy()
    wall, its, stats = time.perf_counter() - t0, solver.newton_iterations, solver.newton_stats
    again = NonlinearElasticitySolver(s2)
    u2 = again.solve().vector()._values()
    assert np.array_equal(u, u2) and again.newton_history == solver.newton_history      # the solve is deterministic
    tip = np.abs(u.reshape(-1, 3)[:, 2]).max()
    print("\nconfigs[2] cantilever: %d Newton iterations, %.2f s, tip deflection %.3f, per-step (Krylov its, AMG set-up ms, solve ms) %s" % (
        its, wall, tip, [(x['krylov_iterations'], round(x['amg_setup_ms'], 1), round(x['solve_ms'], 1)) for x in stats]))
    assert np.all(np.isfinite(u))
    assert 0.5 < tip < 1.0
