"""Linear buckling of LinearElasticitySolver on the host side (no GPU): buckling_settings defaults and range checks, the refusals
that must come before any device call, the ctypes structs of the buckling driver against the header, and the self-checks of the
host reference (tests/buckling_reference.py) the GPU tests compare against."""
import copy
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import buckling_reference as br
from oracle import fem_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}


def _solver(clamped=True, buckling=None, n=(4, 2, 2), degree=1, temperature=None, transient=False):
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(4, 1, 1), *n)
    bcs = OrderedDict()
    if clamped:
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0, 0, 0))}
    bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 4)), 'boundary_id': 2, 'type': 'pressure', 'value': 1e6}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': 2e11, 'poisson_ratio': 0.3, 'density': 7800,
                     'thermal_expansion_coefficient': 2e-6}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", degree)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['transient_settings']['transient'] = bool(transient)
    if buckling is not None:
        s['solver_settings']['buckling_settings'] = buckling
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = temperature
    return LinearElasticitySolver(s)


@pytest.fixture
def no_device(monkeypatch):
    """Every entry point that would reach the GPU fails the test."""
    from fenicssolver_amd import backend
    from fenicssolver_amd import fem

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    for name in ("DeviceMatrix", "DeviceVector", "DeviceSpace", "DeviceMesh", "AMG", "eigen_solve", "buckling_solve", "spmv_multi_pencil",
                 "krylov_solve", "synchronize", "init"):
        monkeypatch.setattr(backend, name, boom)
    monkeypatch.setattr(fem.FunctionSpace, "device", boom, raising=False)
    return boom


# ---- settings ------------------------------------------------------------------------------------------------------------------
def test_buckling_settings_defaults():
    assert _solver().buckling_settings() == {'number_of_modes': 4, 'tolerance': 1e-8, 'max_iterations': 500}
    bs = _solver(buckling={'number_of_modes': 7, 'max_iterations': 50}).buckling_settings()
    assert bs == {'number_of_modes': 7, 'tolerance': 1e-8, 'max_iterations': 50}


@pytest.mark.parametrize("bad", [{'number_of_modes': 0}, {'number_of_modes': 33}, {'number_of_modes': 2.5}, {'number_of_modes': True},
                                 {'tolerance': 0.0}, {'tolerance': -1e-8}, {'tolerance': 'fine'}, {'max_iterations': 0},
                                 {'max_iterations': True}, {'shift': 1.0}, {'modes': 4}])
def test_buckling_settings_range_checks(bad, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="buckling_settings"):
        _solver(buckling=bad).solve_buckling()


# ---- refusals, each before any device call ---------------------------------------------------------------------------------------
def test_p2_space_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="P2 displacement spaces are not supported.*quadrature kernel"):
        _solver(degree=2, n=(2, 1, 1)).solve_buckling()
    with pytest.raises(SolverError, match="P2"):
        _solver(degree=2, n=(2, 1, 1)).geometric_stiffness()


def test_several_ranks_are_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    solver = _solver()
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve_buckling()


def test_periodic_space_is_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver()
    monkeypatch.setattr(solver.function_space, "periodic_pairs", lambda: (np.array([0]), np.array([1])), raising=False)
    with pytest.raises(SolverError, match="periodic"):
        solver.solve_buckling()


def test_thermal_prestress_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="temperature_distribution"):
        _solver(temperature=350.0).solve_buckling()


def test_transient_case_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="transient"):
        _solver(transient=True).solve_buckling()


def test_no_displacement_bc_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="no displacement boundary condition"):
        _solver(clamped=False).solve_buckling()


# ---- the C interface -------------------------------------------------------------------------------------------------------------
def _header_struct(name):
    header = open(os.path.join(ROOT, "include", "fenicssolver_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    return [tuple(d.split()) for d in (x.strip() for x in body.split(";")) if d]


@pytest.mark.parametrize("name", ["fs_buckling_opts", "fs_buckling_stats"])
def test_buckling_structs_match_the_header(name):
    import ctypes as C
    from fenicssolver_amd import _lib
    ctype = {"int": C.c_int, "double": C.c_double, "uint64_t": C.c_uint64, "int64_t": C.c_int64}
    fields = _header_struct(name)
    py = getattr(_lib, name)._fields_
    assert [f[1] for f in fields] == [p[0] for p in py]
    assert [ctype[f[0]] for f in fields] == [p[1] for p in py]


def test_buckling_entry_points_are_bound():
    from fenicssolver_amd import _lib, backend
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    lib = _lib.load()
    for name in ("fs_assemble_geometric_stiffness", "fs_spmv_multi_pencil", "fs_spmv_multi_pencil_benchmark", "fs_buckling_solve"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert hasattr(backend.DeviceMatrix, "assemble_geometric") and hasattr(backend, "spmv_multi_pencil") and hasattr(backend, "buckling_solve")
    for name in ("geometric_stiffness", "buckling_settings", "solve_buckling"):
        assert hasattr(LinearElasticitySolver, name)


# ---- the host reference checks itself ----------------------------------------------------------------------------------------------
def _meshes():
    co, ce = fo.box_mesh((0.0, 0.0, 0.0), (1.5, 1.0, 0.7), 3, 2, 2)[:2]
    yield np.asarray(co, dtype=np.float64), np.asarray(ce)
    yield fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 5, 3)


def _smooth_u(co):
    d = co.shape[1]
    x, y = co[:, 0], co[:, 1]
    z = co[:, 2] if d == 3 else 0.3 * x
    u = np.stack([np.sin(x + 2.0 * y) + z, np.cos(y - z) * x, x * y + z * z][:d], axis=1)
    return 1e-3 * u.ravel()


@pytest.mark.parametrize("which", [0, 1])
def test_reference_is_symmetric_and_annihilates_translations(which):
    co, ce = list(_meshes())[which]
    d = co.shape[1]
    mu = 1.0 + 0.3 * np.sin(np.arange(len(ce)))
    KG = br.geometric_stiffness(co, ce, _smooth_u(co), mu, 1.5 * mu)
    scale = np.abs(KG).max()
    assert scale > 0.0
    assert np.abs(KG - KG.T).max() <= 1e-14 * scale
    assert np.abs(KG.sum(axis=1)).max() <= 1e-13 * scale           # the gradients of a cell sum to zero
    for i in range(d):
        t = np.zeros((co.shape[0], d))
        t[:, i] = 1.0
        assert np.abs(KG @ t.ravel()).max() <= 1e-13 * scale
    # every block is s I
    B = KG.reshape(co.shape[0], d, co.shape[0], d)
    for i in range(d):
        for j in range(d):
            assert np.array_equal(B[:, i, :, j], B[:, 0, :, 0] if i == j else np.zeros_like(B[:, 0, :, 0]))


@pytest.mark.parametrize("which", [0, 1])
def test_reference_reproduces_uniform_uniaxial_stress(which):
    """sigma_xx = -p in every cell: s_ab = -p sum_c |c| dN_a/dx dN_b/dx, assembled here cell by cell."""
    co, ce = list(_meshes())[which]
    d = co.shape[1]
    p = 3.5
    sig = np.zeros((len(ce), d, d))
    sig[:, 0, 0] = -p
    S = br.scalar_geometric(co, ce, sig).toarray()
    g, vol = br.geometry(co, ce)
    ref = np.zeros_like(S)
    for c, vt in enumerate(np.asarray(ce, dtype=np.int64)):
        ref[np.ix_(vt, vt)] += -p * vol[c] * np.outer(g[c, :, 0], g[c, :, 0])
    assert np.abs(S - ref).max() <= 1e-14 * np.abs(ref).max()
    KG = br.geometric_stiffness(co, ce, None, 0.0, 0.0, sigma=sig)
    assert np.array_equal(KG[::d, ::d], S) and np.array_equal(KG[1::d, 1::d], S)
    # compression: K_G is negative semidefinite
    assert np.linalg.eigvalsh(KG).max() <= 1e-12 * np.abs(KG).max()


def test_reference_cell_stress_of_a_uniform_strain():
    """u = (a x, 0, 0): eps_xx = a, sigma = (lambda a + 2 mu a, lambda a, lambda a, 0, 0, 0); plane strain records sigma_zz too."""
    a, mu, lm = 1e-3, 2.0, 3.0
    for which, rec_ref in ((0, [lm * a + 2 * mu * a, lm * a, lm * a, 0, 0, 0]), (1, [lm * a + 2 * mu * a, lm * a, lm * a, 0])):
        co, ce = list(_meshes())[which]
        u = np.zeros_like(co)
        u[:, 0] = a * co[:, 0]
        _, rec = br.cell_stress(co, ce, u.ravel(), mu, lm)
        assert np.abs(rec - np.asarray(rec_ref)[None, :]).max() <= 1e-15


def test_dense_pencil_orders_the_factors():
    K = np.diag([1.0, 2.0, 4.0])
    KG = -np.diag([0.5, 4.0, 1.0])
    nu, phi = br.dense_pencil(KG, K)
    assert np.allclose(nu, [-2.0, -0.5, -0.25]) and np.allclose(-1.0 / nu, [0.5, 2.0, 4.0])
    assert np.allclose(phi.T @ K @ phi, np.eye(3))
