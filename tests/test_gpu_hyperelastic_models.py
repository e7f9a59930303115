"""St Venant-Kirchhoff, Mooney-Rivlin and Yeoh energies of NonlinearElasticitySolver on the MI355X (fs_hyper_models.hip): the kernels
against the numpy reference (tests/hyperelastic_models_reference.py, held to itself in test_hyperelastic_models_host.py), constant
against per-cell parameters, add, the device energy's derivatives, the rest and rigid states, and the solver on exact and reference
states; the Cauchy stress of all four energies (fs_hyper_stress).  Meshes, the smooth displacement and the tolerances are those of
test_gpu_hyperelastic.py."""
import copy
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sps

import hyperelastic_reference as hr
import hyperelastic_models_reference as mr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
CASES = [(m, d) for m in mr.MODELS for d in (3, 2)]

# one parameter row per model (p[4] of the reference) and the same material as the solver's settings
ROW = {
    "st_venant_kirchhoff": mr.row("st_venant_kirchhoff", mu=10.0 / 2.6, lmbda=10.0 * 0.3 / (1.3 * 0.4)),
    "mooney_rivlin": mr.row("mooney_rivlin", c10=1.2, c01=0.4, kappa=2.5),
    "yeoh": mr.row("yeoh", c10=1.5, c20=-0.1, c30=0.02, kappa=2.5),
}
MATERIAL = {
    "st_venant_kirchhoff": {'elastic_modulus': 10.0, 'poisson_ratio': 0.3, 'hyperelastic_model': 'st_venant_kirchhoff'},
    "mooney_rivlin": {'hyperelastic_model': {'type': 'mooney_rivlin', 'c10': 1.2, 'c01': 0.4, 'bulk_modulus': 2.5}},
    "yeoh": {'hyperelastic_model': {'type': 'yeoh', 'c10': 1.5, 'c20': -0.1, 'c30': 0.02, 'bulk_modulus': 2.5}},
}
# The cut-back case per (model, d): (coefficients that differ from MATERIAL, 'pull' = dead traction at x = 1 | 'move' = prescribed shear
# displacement of the x = 1 face, value), chosen on the host: the reference's Newton with the device loop's halving rule converges
# with a halved step, and every tangent on its path is positive definite (CG must not break down).  St Venant-Kirchhoff stiffens in
# tension, so a large dead pull overshoots laterally and recovers.  For Mooney-Rivlin and Yeoh most loads that force a cut also pass
# through an indefinite tangent (Ibar2 is not polyconvex, and neither is a Yeoh energy with c20 < 0); these are the loads found
# where the smallest eigenvalue on the path stays positive: 1.2e-3, 4.9e-3, 2.4e-4, 3.2e-4 of the largest, in the order below.
CUT_BACK = {("st_venant_kirchhoff", 3): ({}, "pull", 35.0), ("st_venant_kirchhoff", 2): ({}, "pull", 35.0),
            ("mooney_rivlin", 3): ({'c01': 0.1, 'bulk_modulus': 6.0}, "move", 0.8),
            ("mooney_rivlin", 2): ({'c01': 0.1, 'bulk_modulus': 6.0}, "move", 0.8),
            ("yeoh", 3): ({'bulk_modulus': 6.0}, "move", 0.8), ("yeoh", 2): ({'bulk_modulus': 10.0}, "move", 1.1)}
SMALL_LOAD = 0.02        # traction of the small-load case: strains of about 1e-2, differences to the linear solution of about 1e-4


def _device(mesh):
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


def _min_J(mesh, d, u):
    co, ce = mesh.coordinates()[:, :d], mesh.cells().astype(np.int64)
    E0 = np.swapaxes(co[ce][:, 1:] - co[ce][:, :1], 1, 2)
    U = u.reshape(-1, d)[ce]
    return (np.linalg.det(E0 + np.swapaxes(U[:, 1:] - U[:, :1], 1, 2)) / np.linalg.det(E0)).min()


def _random_rows(model, nc, seed):
    """per-cell parameter rows [nc, 4] inside every model's admissible range"""
    r = np.random.default_rng(seed).random((nc, 4))
    if model == "st_venant_kirchhoff":
        return np.stack([1.0 + r[:, 0], 2.0 + r[:, 1], 0 * r[:, 2], 0 * r[:, 3]], axis=1)
    if model == "mooney_rivlin":
        return np.stack([0.5 + 0.5 * r[:, 0], 0.2 + 0.2 * r[:, 1], 4.0 + r[:, 2], 0 * r[:, 3]], axis=1)
    return np.stack([0.6 + 0.4 * r[:, 0], -0.1 + 0.05 * r[:, 1], 0.03 + 0.02 * r[:, 2], 5.0 + r[:, 3]], axis=1)


def _args(model, rows):
    """keyword arguments of backend.assemble_hyperelastic / hyperelastic_stress for one row p[4] or per-cell rows [nc, 4]"""
    rows = np.asarray(rows, dtype=np.float64)
    cell = rows.ndim == 2
    if model in ("st_venant_kirchhoff", "neo_hookean"):
        return {"lame": ("cell", np.ascontiguousarray(rows[:, :2])) if cell else (float(rows[0]), float(rows[1])), "model": model}
    n = 3 if model == "mooney_rivlin" else 4
    return {"lame": None, "model": model, "params": ("cell", np.ascontiguousarray(rows[:, :n])) if cell else tuple(float(x) for x in rows[:n])}


def _assemble(dV, uh, model, rows, add=False, K=None, r=None):
    from fenicssolver_amd import backend
    K = backend.DeviceMatrix(dV) if K is None else K
    r = backend.DeviceVector(dV.n_owned) if r is None else r
    info = backend.assemble_hyperelastic(dV, backend.DeviceVector(dV.n_local, uh), K=K, r=r, energy=True, add=add, **_args(model, rows))
    return K, r, info


_HOST = {}


def _host(model, d):
    """the host reference on the 4 x 3 x 3 box / 6 x 5 rectangle at the smooth displacement with random per-cell rows: computed
    once, read by the tests that need it"""
    if (model, d) not in _HOST:
        mesh = _box() if d == 3 else _rect()
        uh = _smooth_u(mesh.coordinates(), d)
        rows = _random_rows(model, mesh.num_cells(), 5)
        _HOST[(model, d)] = (mesh, uh, rows) + mr.assemble(mesh.coordinates()[:, :d], mesh.cells(), uh, model, rows)
    return _HOST[(model, d)]


@pytest.mark.parametrize("model,d", CASES)
def test_kernels_match_the_host_reference_and_are_deterministic(model, d):
    from fenicssolver_amd import backend
    mesh, uh, rows, e_h, f_h, K_h, J_h, s_h = _host(model, d)
    assert J_h.min() > 0.5 and _min_J(mesh, d, uh) > 0.5
    V, dV = _device(mesh)
    outs = []
    for _ in range(2):
        K, r, info = _assemble(dV, uh, model, rows)
        sig = backend.hyperelastic_stress(dV, backend.DeviceVector(dV.n_local, uh), **_args(model, rows))
        assert info["n_inverted"] == 0 and info["first_inverted_cell"] == -1
        outs.append((K.to_csr()[2], r.get(), info["energy"], sig))
    Kd = _csr(K)
    errs = (abs(Kd - K_h).max() / abs(K_h).max(), np.abs(outs[0][1] - f_h).max() / np.abs(f_h).max(), abs(outs[0][2] - e_h) / abs(e_h),
            np.abs(outs[0][3] - s_h).max() / np.abs(s_h).max())
    print("\n%s d=%d: relative errors tangent %.2e force %.2e energy %.2e stress %.2e" % ((model, d) + errs))
    assert all(np.array_equal(a, b) for a, b in zip(outs[0], outs[1]))
    assert outs[0][3].shape == (mesh.num_cells(), 6 if d == 3 else 4)
    assert max(errs) <= 1e-12


@pytest.mark.parametrize("model,d", CASES)
def test_per_cell_rows_of_one_constant_give_the_constant_bits(model, d):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh)
    uh = _smooth_u(mesh.coordinates(), d)
    nc = mesh.num_cells()
    out = []
    for rows in (ROW[model], np.tile(ROW[model], (nc, 1))):
        K, r, info = _assemble(dV, uh, model, rows)
        sig = backend.hyperelastic_stress(dV, backend.DeviceVector(dV.n_local, uh), **_args(model, rows))
        out.append((K.to_csr()[2], r.get(), info["energy"], sig))
    assert all(np.array_equal(a, b) for a, b in zip(out[0], out[1]))
    # per-cell rows are checked like the constants, and the message names the cell
    bad = np.tile(ROW[model], (nc, 1))
    bad[3, 0] = -1.0
    with pytest.raises(backend.BackendError, match="cell 3"):
        _assemble(dV, uh, model, bad)
    bad[3, 0] = np.nan
    with pytest.raises(backend.BackendError, match="cell 3"):
        backend.hyperelastic_stress(dV, backend.DeviceVector(dV.n_local, uh), **_args(model, bad))
    row = ROW[model].copy()
    row[3 if model == "yeoh" else 2 if model == "mooney_rivlin" else 0] = 0.0          # kappa = 0, or mu = 0
    with pytest.raises(backend.BackendError, match="required"):
        _assemble(dV, uh, model, row)


@pytest.mark.parametrize("model,d", CASES)
def test_add_accumulates_onto_the_target_bit_for_bit(model, d):
    """3 x 3 x 4 box: 216 cells, 80 nodes (a partial second 64-row slice); 5 x 4 rectangle: 40 cells, 30 nodes"""
    from fenicssolver_amd import backend
    mesh = _box((3, 3, 4)) if d == 3 else _rect((5, 4))
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    assert (nc, mesh.num_vertices()) == ((216, 80) if d == 3 else (40, 30))
    uh = _smooth_u(mesh.coordinates(), d)
    assert _min_J(mesh, d, uh) > 0.5
    rng = np.random.default_rng(80 + d)
    for rows in (ROW[model], _random_rows(model, nc, 81)):
        K, r, info = _assemble(dV, uh, model, rows)
        assert info["n_inverted"] == 0
        xk, xr = K.to_csr()[2], r.get()
        y = 0.37 + rng.standard_normal(dV.n_owned)
        Ka, ra = backend.DeviceMatrix(dV), backend.DeviceVector(dV.n_owned, y)
        Ka.assemble(lame=(3.1, 4.7))
        yk = Ka.to_csr()[2]
        _assemble(dV, uh, model, rows, add=True, K=Ka, r=ra)
        assert np.array_equal(Ka.to_csr()[2], yk + xk)
        assert np.array_equal(ra.get(), y + xr)


@pytest.mark.parametrize("model,d", CASES)
def test_tangent_and_force_are_the_derivatives_of_the_device_energy(model, d):
    mesh = _box((3, 3, 2)) if d == 3 else _rect((5, 4))
    V, dV = _device(mesh)
    uh = _smooth_u(mesh.coordinates(), d, amp=0.1)
    assert _min_J(mesh, d, uh) > 0.5
    rng = np.random.default_rng(11)

    def state(x):
        K, r, info = _assemble(dV, x, model, ROW[model])
        return _csr(K), r.get(), info["energy"]
    K, f, _ = state(uh)
    h = 1e-6
    for _ in range(3):
        w = rng.standard_normal(uh.size)
        _, fp, ep = state(uh + h * w)
        _, fm, em = state(uh - h * w)
        assert np.abs((fp - fm) / (2 * h) - K @ w).max() <= 1e-6 * np.abs(K @ w).max()
        assert abs((ep - em) / (2 * h) - f @ w) <= 1e-6 * abs(f @ w)


@pytest.mark.parametrize("model,d", CASES)
def test_rest_state_is_the_linear_operator_and_a_rotation_costs_nothing(model, d):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    co = mesh.coordinates()[:, :d]
    for rows in (ROW[model], _random_rows(model, nc, 3)):
        rows2 = np.broadcast_to(rows, (nc, 4))
        mu0, lm0 = mr.small_strain_moduli(model, rows2.T)
        A = backend.DeviceMatrix(dV)
        A.assemble(lame=("cell", np.stack([mu0, lm0], axis=1)) if np.ndim(rows) == 2 else (float(mu0[0]), float(lm0[0])))
        K, r, info = _assemble(dV, np.zeros(dV.n_local), model, rows)
        a, k = A.to_csr(), K.to_csr()
        assert np.array_equal(a[0], k[0]) and np.array_equal(a[1], k[1])
        # to rounding, not bit for bit: the invariant form and the linear kernel are different expressions
        assert np.abs(a[2] - k[2]).max() <= 1e-12 * np.abs(a[2]).max()
        # F = I exactly: every term of P and of psi cancels within a few roundings of the moduli (<= 6), times V |g| <= 0.1 and the
        # handful of cells around a node
        assert np.abs(r.get()).max() <= 1e-13 and abs(info["energy"]) <= 1e-13
        assert info["n_inverted"] == 0
        # rigid rotation by 30 degrees (about x in 3-D): the rounding level of the existing rotation test
        th = np.pi / 6
        R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
        if d == 3:
            R = np.block([[np.eye(1), np.zeros((1, 2))], [np.zeros((2, 1)), R]])
        u = ((co - 0.5) @ (R - np.eye(d)).T).ravel()
        K, r, info = _assemble(dV, u, model, rows)
        assert np.abs(r.get()).max() < 1e-9 and abs(info["energy"]) < 1e-9 and info["n_inverted"] == 0


# ---- through the solver ----------------------------------------------------------------------------------------------------------
def _settings(mesh, material, bcs):
    from fenicssolver_amd.fem import VectorFunctionSpace
    from fenicssolver_amd import SolverBase as SB
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = dict({'name': 'rubber', 'density': 1000, 'thermal_expansion_coefficient': 0.0}, **copy.deepcopy(material))
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-13, 'newton_solver': {'relative_tolerance': 1e-12}}
    return s


def _plane(k, v):
    from fenicssolver_amd.fem import AutoSubDomain, near
    return AutoSubDomain(lambda x: near(x[k], v))


def _stretch_case(material, d, delta, L=1.0):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, Constant
    mesh = BoxMesh(Point(0, 0, 0), Point(L, L, L), 4, 3, 3) if d == 3 else RectangleMesh(Point(0, 0), Point(L, L), 6, 5)
    bcs = OrderedDict()
    for k, name in enumerate("xyz"[:d]):
        val = [None] * d
        val[k] = Constant(0.0)
        bcs["sym_" + name] = {'boundary': _plane(k, 0.0), 'boundary_id': k + 1, 'type': 'Dirichlet', 'value': tuple(val)}
    val = [None] * d
    val[0] = Constant(delta)
    bcs["pull"] = {'boundary': _plane(0, L), 'boundary_id': 9, 'type': 'Dirichlet', 'value': tuple(val)}
    return _settings(mesh, material, bcs), mesh


def _clamped_case(material, d, n, traction=None, move=None):
    """the unit cube / square clamped at x = 0; at x = 1 a dead traction ('stress') or a prescribed displacement"""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, Constant
    mesh = BoxMesh(Point(0, 0, 0), Point(1, 1, 1), *n) if d == 3 else RectangleMesh(Point(0, 0), Point(1, 1), *n)
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': _plane(0, 0.0), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0.0,) * d)}
    if traction is not None:
        bcs["load"] = {'boundary': _plane(0, 1.0), 'boundary_id': 2, 'type': 'stress', 'value': Constant(tuple(traction))}
    if move is not None:
        bcs["move"] = {'boundary': _plane(0, 1.0), 'boundary_id': 2, 'type': 'Dirichlet', 'value': Constant(tuple(move))}
    return _settings(mesh, material, bcs), mesh


def _traction_rhs(mesh, d, traction):
    """f_ext of the dead traction on the x = 1 face: |facet| / d per facet vertex"""
    co = mesh.coordinates()[:, :d]
    fac = mesh.facets()[mesh.exterior_facets()].astype(np.int64)
    right = fac[np.all(np.abs(co[fac][:, :, 0] - 1.0) < 1e-12, axis=1)]
    p = co[right]
    size = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1) if d == 3 else np.linalg.norm(p[:, 1] - p[:, 0], axis=1)
    f = np.zeros(co.size)
    for k in range(d):
        np.add.at(f, (right * d + k).ravel(), np.repeat(traction[k] * size / d, d))
    return f


def _rows_of(solver):
    """the reference's parameter rows of a solver's material: one row or [n_cells, 4]"""
    model, params = solver.hyperelastic_model()
    if params is not None:
        return model, np.asarray(params, dtype=np.float64)
    mu, lm = solver.lame_parameters()
    return model, np.array([mu, lm, 0.0, 0.0])


def _dirichlet(solver):
    return solver._bc_arrays(solver.generate_form(0, None, None, solver.w_prev, solver.w_prev)[1])


@pytest.mark.parametrize("model,d", CASES)
def test_exact_homogeneous_stretch(model, d):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    L, delta = 1.0, 0.3
    s, mesh = _stretch_case(MATERIAL[model], d, delta, L)
    solver = NonlinearElasticitySolver(s)
    u = solver.solve().vector()._values()
    _, p = _rows_of(solver)
    assert np.allclose(p, ROW[model], rtol=1e-14)
    sx = 1.0 + delta / L
    t = mr.exact_stretch_t(model, p, sx, d)
    co = mesh.coordinates()[:, :d]
    Fx = np.diag([sx] + [t] * (d - 1))
    exact = (co @ (Fx - np.eye(d)).T).ravel()
    assert np.abs(u - exact).max() < 1e-9
    assert solver.newton_iterations >= 2 and solver.newton_history[-1] < 1e-9 * solver.newton_history[0]
    dV = solver.function_space.device()
    K, r, info = _assemble(dV, exact, model, p)
    f = r.get().reshape(-1, d)
    right = np.abs(co[:, 0] - L) < 1e-12
    assert abs(f[right, 0].sum() - mr.first_pk_11(model, p, sx, t, d) * L ** (d - 1)) < 1e-10
    sig = solver.cauchy_stress()
    closed = mr.cauchy(model, p, Fx)
    assert sig.shape == (mesh.num_cells(), 6 if d == 3 else 4)
    assert np.abs(sig - closed[None, :]).max() < 1e-9
    assert abs(closed[1]) < 1e-12 and closed[0] > 0.1                       # free lateral faces, a pull
    vm = solver.von_Mises().vector()._values()
    assert np.abs(vm - mr.von_mises(closed)).max() < 1e-8 * mr.von_mises(closed)


@pytest.mark.parametrize("d", [3, 2])
def test_neo_hookean_cauchy_stress_on_the_homogeneous_stretch(d):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import Function
    s, mesh = _stretch_case({'elastic_modulus': 10.0, 'poisson_ratio': 0.3}, d, 0.3)
    solver = NonlinearElasticitySolver(s)
    solver.solve()
    mu, lmbda = solver.lame_parameters()
    sx = 1.3
    t = hr.exact_stretch_t(sx, mu, lmbda, d)
    J = sx * t ** (d - 1)
    s11 = hr.first_pk_11(sx, t, mu, lmbda, d) * sx / J                      # sigma = P F^T / J
    szz = 0.0 if d == 3 else lmbda * np.log(J) / J                          # plane strain: P_33 = lambda ln J with F33 = 1
    closed = np.array([s11, 0.0, szz, 0.0] + ([0.0, 0.0] if d == 3 else []))
    sig = solver.cauchy_stress()
    assert sig.shape == (mesh.num_cells(), 6 if d == 3 else 4)
    assert np.abs(sig - closed[None, :]).max() < 1e-9
    vm = solver.von_Mises().vector()._values()
    assert np.abs(vm - mr.von_mises(closed)).max() < 1e-8 * mr.von_mises(closed)
    # inverted cells are refused, not filled in: the x = 1 face pushed through the body
    bad = Function(solver.function_space)
    x0 = np.zeros(mesh.num_vertices() * d)
    x0[0::d] = -1.5 * mesh.coordinates()[:, 0]
    bad.vector().set_local(x0)
    with pytest.raises(SolverError, match=r"inverted.*first cell \d+"):
        solver.cauchy_stress(bad)
    with pytest.raises(SolverError, match="inverted"):
        solver.von_Mises(bad)


@pytest.mark.parametrize("model,d", CASES)
def test_small_load_limit_is_the_linear_solution(model, d):
    """the difference to the linear solution of the same small-strain moduli is quadratic in the load: halving it divides it by 4"""
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    n = (4, 3, 3) if d == 3 else (6, 5)
    diffs = []
    for q in (SMALL_LOAD, 0.5 * SMALL_LOAD):
        traction = [0.6 * q, -q] + ([0.3 * q] if d == 3 else [])
        s, mesh = _clamped_case(MATERIAL[model], d, n, traction=traction)
        nl_solver = NonlinearElasticitySolver(copy.deepcopy(s))
        nl = nl_solver.solve().vector()._values().copy()
        mu0, lm0 = nl_solver.small_strain_moduli()
        mu0, lm0 = float(mu0[0]), float(lm0[0])
        s['material'] = {'name': 'rubber', 'density': 1000, 'thermal_expansion_coefficient': 0.0,
                         'elastic_modulus': mu0 * (3 * lm0 + 2 * mu0) / (lm0 + mu0), 'poisson_ratio': lm0 / (2 * (lm0 + mu0))}
        lin_solver = LinearElasticitySolver(s)
        lin_solver.reference_load_sign = False
        lin = lin_solver.solve().vector()._values()
        assert np.abs(lin).max() > 1e-4
        diffs.append(np.abs(nl - lin).max())
    print("\n%s d=%d: |u_nl - u_lin| at q, q/2: %.3e %.3e, ratio %.3f" % (model, d, diffs[0], diffs[1], diffs[0] / diffs[1]))
    assert diffs[1] > 1e-8                                                 # far above the solver tolerances (1e-12, 1e-13)
    assert 3.0 <= diffs[0] / diffs[1] <= 5.0


@pytest.mark.parametrize("d", [3, 2])
def test_per_region_mooney_rivlin_matches_the_host_newton(d):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    from fenicssolver_amd.fem import MeshFunction
    material = {'hyperelastic_model': {'type': 'mooney_rivlin', 'c01': 0.4, 'bulk_modulus': 2.5,
                                       'c10': {'soft': {'subdomain_id': 1, 'value': 0.6}, 'hard': {'subdomain_id': 2, 'value': 2.4}}}}
    move = (0.1, -0.06, 0.03)[:d]
    s, mesh = _clamped_case(material, d, (4, 3, 3) if d == 3 else (6, 5), move=move)
    solver = NonlinearElasticitySolver(s)
    co, ce = mesh.coordinates()[:, :d], mesh.cells().astype(np.int64)
    sub = MeshFunction("size_t", mesh, d)
    sub.array()[:] = np.where(co[ce].mean(axis=1)[:, 0] < 0.5, 1, 2)
    solver.subdomains = sub
    u = solver.solve().vector()._values()
    model, rows = _rows_of(solver)
    assert model == "mooney_rivlin" and rows.shape == (len(ce), 4) and set(np.unique(rows[:, 0])) == {0.6, 2.4}
    dofs, vals = _dirichlet(solver)
    uh, hist, _ = mr.newton(co, ce, model, rows, np.zeros(co.size), dofs, vals)
    assert len(hist) >= 3 and np.abs(u - uh).max() <= 1e-9 * np.abs(uh).max()
    sig = solver.cauchy_stress()
    s_h = mr.assemble(co, ce, uh, model, rows)[4]
    assert np.abs(sig - s_h).max() <= 1e-8 * np.abs(s_h).max()


@pytest.mark.parametrize("model,d", CASES)
def test_a_step_too_large_is_cut_back_and_still_converges(model, d):
    from fenicssolver_amd.NonlinearElasticitySolver import NonlinearElasticitySolver
    other, kind, value = CUT_BACK[(model, d)]
    material = copy.deepcopy(MATERIAL[model])
    if other:
        material['hyperelastic_model'].update(other)
    traction = [value] + [0.0] * (d - 1) if kind == "pull" else None
    move = [0.0] * (d - 1) + [-value] if kind == "move" else None
    s, mesh = _clamped_case(material, d, (4, 2, 2) if d == 3 else (4, 2), traction=traction, move=move)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    solver = NonlinearElasticitySolver(s)
    solver.init_solver()
    co, ce = mesh.coordinates()[:, :d], mesh.cells().astype(np.int64)
    dofs, vals = _dirichlet(solver)
    _, p = _rows_of(solver)
    f_ext = _traction_rhs(mesh, d, traction) if traction is not None else np.zeros(co.size)
    with np.errstate(invalid="ignore", divide="ignore"):
        x, hist, host_steps = mr.newton(co, ce, model, p, f_ext, dofs, vals, rtol=1e-11, cut_back=True)
    assert min(host_steps) < 1.0
    u = solver.solve().vector()._values()
    assert np.all(np.isfinite(u))
    assert min(solver.newton_steps) < 1.0                              # a step was cut back
    assert solver.newton_history[-1] < 1e-9 * solver.newton_history[0]
    assert np.abs(u - x).max() < 1e-8 * np.abs(x).max()
