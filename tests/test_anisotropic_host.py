"""Anisotropic materials of LinearElasticitySolver on the host side (no GPU): the identities the host reference
(tests/anisotropic_reference.py) rests on, the Voigt permutation, compliance -> stiffness, orientation parsing, every refusal (each
before any device call), the unchanged describe() of an isotropic form, and the struct against the header."""
import copy
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

import anisotropic_reference as ar
from oracle import fem_oracle as fo

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
EPS = np.finfo(np.float64).eps


def _solver(material, dim=3, degree=1, n=(2, 2, 2), bcs=None, regions=None, transient=False, temperature=None, cls=None):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, MeshFunction, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(1, 1, 2), *n) if dim == 3 else RectangleMesh(Point(0, 0), Point(2, 1), n[0], n[1])
    if bcs is None:
        bcs = OrderedDict()
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0,) * dim)}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = dict({'name': 'composite', 'density': 1600.0, 'thermal_expansion_coefficient': 2e-6}, **material)
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", degree)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['transient_settings']['transient'] = bool(transient)
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = temperature
    solver = (cls or LinearElasticitySolver)(s)
    if regions is not None:
        sub = MeshFunction("size_t", mesh, dim)
        sub.array()[:] = regions(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1))
        solver.subdomains = sub
    return solver


def _form(solver):
    return solver.generate_form(0, None, None, None, None)[0]


@pytest.fixture
def no_device(monkeypatch):
    """Every entry point that would reach the GPU fails the test."""
    from fenicssolver_amd import backend
    from fenicssolver_amd import fem

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    for name in ("DeviceMatrix", "DeviceVector", "DeviceSpace", "DeviceMesh", "AMG", "eigen_solve", "buckling_solve", "krylov_solve",
                 "synchronize", "init", "anisotropic_stress", "assemble_anisotropic_load"):
        monkeypatch.setattr(backend, name, boom)
    monkeypatch.setattr(fem.FunctionSpace, "device", boom, raising=False)
    return boom


CFRP_V = ar.orthotropic_voigt(**{k: ar.CFRP[v] for k, v in (('E', 'elastic_moduli'), ('nu', 'poisson_ratios'), ('G', 'shear_moduli'))})


# ---- the identities of the reference ---------------------------------------------------------------------------------------------
def test_cfrp_material_is_positive_definite():
    assert np.linalg.eigvalsh(CFRP_V).min() > 0.0
    assert np.abs(CFRP_V - CFRP_V.T).max() <= 1e-15 * np.abs(CFRP_V).max()


def test_isotropic_tensor_reproduces_the_lame_operator():
    co, ce = fo.box_mesh((0, 0, 0), (2.0, 1.0, 1.5), 3, 2, 2)
    E, nu = 2e11, 0.27
    D = np.broadcast_to(ar.to_library(ar.isotropic_voigt(E, nu)), (len(ce), 6, 6))
    Ka, Ko = ar.local_stiffness(co, ce, D), fo.p1_elasticity_local(co, ce, E, nu)
    assert np.abs(Ka - Ko).max() <= 1e-14 * np.abs(Ko).max()
    co2, ce2 = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 5, 3)
    D2 = np.broadcast_to(ar.to_library(ar.isotropic_voigt(3e3, 0.3)), (len(ce2), 6, 6))
    Kt = fo.tri_elasticity_local(co2, ce2, 3e3, 0.3)
    assert np.abs(ar.local_stiffness(co2, ce2, D2) - Kt).max() <= 1e-14 * np.abs(Kt).max()


def test_rotated_gradient_form_equals_the_rotated_tensor_form():
    """K_ab = R (V ghat_a . C . ghat_b) R^T with ghat = R^T g - what the kernels compute - against V B^T D' B with the rotated D'."""
    co, ce = fo.box_mesh((0, 0, 0), (1.0, 1.0, 1.0), 2, 1, 1)
    nc = len(ce)
    R = ar.random_rotations(nc, 5)
    D = ar.to_library(CFRP_V)
    Kref = ar.local_stiffness(co, ce, ar.global_D(D[None], None, R, nc))
    vol, g = ar.geometry(co, ce)
    C4 = ar.tensor4(D)
    gh = np.einsum('cki,cak->cai', R, g)
    Gm = np.einsum('cak,ikjl,cbl->cabij', gh, C4, gh)
    K = vol[:, None, None, None, None] * np.einsum('cim,cabmn,cjn->cabij', R, Gm, R)
    K = K.transpose(0, 1, 3, 2, 4).reshape(nc, 12, 12)
    assert np.abs(K - Kref).max() <= 1e-14 * np.abs(Kref).max()


def test_rotation_identity_of_the_rank_4_tensor():
    Q, R = ar.random_rotations(2, 11)
    C4 = ar.tensor4(ar.to_library(CFRP_V))
    both = ar.rotate4(ar.rotate4(C4, R), Q)
    assert np.abs(both - ar.rotate4(C4, Q @ R)).max() <= 1e-15 * np.abs(C4).max() * 16
    assert np.abs(ar.matrix6(ar.rotate4(ar.tensor4(ar.to_library(ar.isotropic_voigt(1.0, 0.3))), R)) -
                  ar.to_library(ar.isotropic_voigt(1.0, 0.3))).max() <= 1e-15


def test_thermal_load_balances_the_linear_field():
    """K u_lin = b_thermal on every row for u_lin = eps* x, and the stress of u_lin less the eigenstress is zero."""
    co, ce = fo.box_mesh((0, 0, 0), (2.0, 1.0, 1.5), 3, 2, 2)
    nc = len(ce)
    Dg = ar.global_D(ar.to_library(CFRP_V)[None], None, ar.random_rotations(nc, 3), nc)
    A = np.array([[1e-6, 2e-6, -1e-6], [2e-6, 3e-5, 4e-6], [-1e-6, 4e-6, 2e-5]]) * 50.0
    eig = np.tile([A[0, 0], A[1, 1], A[2, 2], A[0, 1], A[0, 2], A[1, 2]], (nc, 1))
    u = (co @ A.T).ravel()
    K = ar.assemble(len(co), ce, ar.local_stiffness(co, ce, Dg), 3)
    b = ar.eigenstress_load(len(co), co, ce, Dg, eig)
    assert np.abs(K @ u - b).max() <= 1e-13 * np.abs(b).max()
    s0 = ar.cell_stress(co, ce, None, Dg, -eig)
    assert np.abs(ar.cell_stress(co, ce, u, Dg, eig)).max() <= 1e-13 * np.abs(s0).max()


# ---- module-level helpers and the Voigt permutation ------------------------------------------------------------------------------
def test_voigt_permutation_and_helpers():
    from fenicssolver_amd import LinearElasticitySolver as LES
    assert LES.VOIGT_TO_LIBRARY == [0, 1, 2, 5, 4, 3] == ar.VOIGT_TO_LIBRARY
    Cv = LES.orthotropic_stiffness(ar.CFRP['elastic_moduli'], ar.CFRP['poisson_ratios'], ar.CFRP['shear_moduli'])
    assert np.abs(Cv - CFRP_V).max() <= 1e-14 * np.abs(CFRP_V).max()
    # compliance -> stiffness: S C = I, with S_12 = -nu12 / E1 and the shears at (23, 13, 12)
    S = ar.compliance_voigt(ar.CFRP['elastic_moduli'], ar.CFRP['poisson_ratios'], ar.CFRP['shear_moduli'])
    assert S[0, 1] == -0.3 / 140e9 and S[3, 3] == 1 / 3e9 and S[5, 5] == 1 / 5e9
    assert np.abs(S @ Cv - np.eye(6)).max() <= 1e-14
    assert (Cv[3, 3], Cv[4, 4], Cv[5, 5]) == pytest.approx((3e9, 4.5e9, 5e9), rel=1e-14)
    # the solver hands the library order to the device: G12 (Voigt 66) is the xy entry 3, G23 (Voigt 44) the yz entry 5
    table, index, frames = _solver({'elasticity_tensor': Cv}).stiffness_tensor()
    assert index is None and frames is None and table.shape == (1, 6, 6)
    assert np.array_equal(table[0], 0.5 * (Cv + Cv.T)[np.ix_([0, 1, 2, 5, 4, 3], [0, 1, 2, 5, 4, 3])])
    assert (table[0][3, 3], table[0][4, 4], table[0][5, 5]) == pytest.approx((5e9, 4.5e9, 3e9), rel=1e-14)
    t2 = _solver({'orthotropic': dict(ar.CFRP)}).stiffness_tensor()[0]
    assert np.array_equal(t2, table)
    # the rank-4 tensor of both orders is the same tensor
    assert np.abs(ar.tensor4(Cv, ar.VOIGT) - ar.tensor4(table[0], ar.LIB)).max() == 0.0


def test_isotropic_stiffness_against_the_lame_parameters():
    from fenicssolver_amd.LinearElasticitySolver import isotropic_stiffness
    E, nu = 2e11, 0.27
    mu, lm = fo.lame(E, nu)
    C = isotropic_stiffness(E, nu)
    ref = np.zeros((6, 6))
    ref[:3, :3] = lm
    ref[np.arange(3), np.arange(3)] = lm + 2 * mu
    ref[np.arange(3, 6), np.arange(3, 6)] = mu
    assert np.abs(C - ref).max() <= 4 * EPS * np.abs(ref).max()
    assert np.abs(C - ar.isotropic_voigt(E, nu)).max() <= 4 * EPS * np.abs(ref).max()


def test_regions_of_both_kinds_under_elasticity_tensor():
    from fenicssolver_amd.LinearElasticitySolver import isotropic_stiffness, orthotropic_stiffness
    Co = orthotropic_stiffness(ar.CFRP['elastic_moduli'], ar.CFRP['poisson_ratios'], ar.CFRP['shear_moduli'])
    mat = {'elasticity_tensor': {'ply': {'subdomain_id': 1, 'value': Co}, 'resin': {'subdomain_id': 2, 'value': isotropic_stiffness(3e9, 0.35)}}}
    solver = _solver(mat, regions=lambda cen: np.where(cen[:, 2] < 1.0, 1, 2))
    table, index, frames = solver.stiffness_tensor()
    assert table.shape == (2, 6, 6) and frames is None
    assert np.array_equal(index, np.where(solver.subdomains.array() == 1, 0, 1))
    assert 0 < index.sum() < len(index)
    d = _form(solver).describe()
    assert d['mu'] is None and d['anisotropic']['materials'] == 2 and d['anisotropic']['per_cell_index']


# ---- orientation -------------------------------------------------------------------------------------------------------------------
def test_orientation_parsing_and_orthonormalisation():
    from fenicssolver_amd.fem import UserExpression
    R0 = ar.rotation_about([1.0, 2.0, -1.0], np.pi / 6)
    base = {'orthotropic': dict(ar.CFRP)}
    fr = _solver(dict(base, material_orientation=R0)).stiffness_tensor()[2]
    assert fr.shape == (48, 3, 3) and np.array_equal(fr, np.broadcast_to(R0, fr.shape))
    # two skew axes: e1 = v / |v|, e2 = w less its part along e1, e3 = e1 x e2
    v, w = np.array([2.0, 0.0, 0.0]), np.array([1.0, 3.0, 0.0])
    fr = _solver(dict(base, material_orientation={'axis_1': v, 'axis_2': w})).stiffness_tensor()[2]
    assert np.abs(fr[0] - np.eye(3)).max() <= 2 * EPS
    v, w = np.array([1.0, 1.0, 0.0]), np.array([0.0, 1.0, 1.0])
    R = _solver(dict(base, material_orientation={'axis_1': v, 'axis_2': w})).stiffness_tensor()[2][0]
    assert np.abs(R.T @ R - np.eye(3)).max() <= 4 * EPS and np.linalg.det(R) > 0
    assert np.abs(R[:, 0] - v / np.sqrt(2)).max() <= 2 * EPS and abs(R[:, 1] @ v) <= 4 * EPS and R[:, 1] @ w > 0
    # per region, either kind
    per = {'a': {'subdomain_id': 1, 'value': R0}, 'b': {'subdomain_id': 2, 'axis_1': [0, 1, 0], 'axis_2': [-1, 0, 0]}}
    s = _solver(dict(base, material_orientation=per), regions=lambda cen: np.where(cen[:, 2] < 1.0, 1, 2))
    fr = s.stiffness_tensor()[2]
    ids = s.subdomains.array()
    assert np.array_equal(fr[ids == 1], np.broadcast_to(R0, (int((ids == 1).sum()), 3, 3)))
    assert np.abs(fr[ids == 2] - np.array([[0, -1, 0], [1, 0, 0], [0, 0, 1.0]])).max() == 0.0

    class Cylindrical(UserExpression):           # radial, hoop, axial about the z axis through (0.5, 0.5)
        def value_shape(self):
            return (9,)

        def eval(self, value, x):
            t = np.arctan2(x[1] - 0.5, x[0] - 0.5)
            value[:] = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]]).ravel()
    s = _solver(dict(base, material_orientation=Cylindrical(degree=0)))
    fr = s.stiffness_tensor()[2]
    cen = s.mesh.coordinates()[s.mesh.cells().astype(np.int64)].mean(axis=1)
    radial = (cen[:, :2] - 0.5) / np.linalg.norm(cen[:, :2] - 0.5, axis=1)[:, None]
    assert np.abs(fr[:, :2, 0] - radial).max() <= 1e-14 and len(np.unique(np.round(fr[:, 0, 0], 12))) > 2


@pytest.mark.parametrize("bad,match", [
    (np.diag([1.0, 1.0, -1.0]), "not a proper rotation"),                       # a reflection: det < 0
    (np.eye(3) + 1e-9 * np.ones((3, 3)), "not a proper rotation"),              # max|R^T R - I| > 1e-10
    (2.0 * np.eye(3), "not a proper rotation"),
    ({'axis_1': [1, 0, 0], 'axis_2': [2, 0, 0]}, "parallel"),
    ({'axis_1': [0, 0, 0], 'axis_2': [0, 1, 0]}, "zero vector"),
    (np.eye(4), "3x3 rotation"),
])
def test_bad_orientations_are_refused(bad, match, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match=match):
        _form(_solver({'orthotropic': dict(ar.CFRP), 'material_orientation': bad}))


def test_a_rotation_within_the_tolerance_is_taken(no_device):
    R = ar.rotation_about([0, 0, 1.0], 0.3) + 1e-12
    assert _form(_solver({'orthotropic': dict(ar.CFRP), 'material_orientation': R})).anisotropic.frames is not None


# ---- refusals of the material ----------------------------------------------------------------------------------------------------------
def test_a_material_that_is_not_positive_definite_names_its_region(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    bad = CFRP_V.copy()
    bad[0, 1] = bad[1, 0] = 2.0 * np.sqrt(bad[0, 0] * bad[1, 1])
    with pytest.raises(SolverError, match="'elasticity_tensor'.*not positive definite"):
        _form(_solver({'elasticity_tensor': bad}))
    mat = {'elasticity_tensor': {'good': {'subdomain_id': 1, 'value': CFRP_V}, 'broken': {'subdomain_id': 2, 'value': bad}}}
    with pytest.raises(SolverError, match="region 'broken'.*not positive definite"):
        _form(_solver(mat, regions=lambda cen: np.where(cen[:, 2] < 1.0, 1, 2)))
    skew = CFRP_V.copy()
    skew[0, 1] *= 1.001
    with pytest.raises(SolverError, match="not symmetric"):
        _form(_solver({'elasticity_tensor': skew}))
    with pytest.raises(SolverError, match="6x6"):
        _form(_solver({'elasticity_tensor': np.eye(3)}))
    # nu12 too large for E1 / E2: the compliance is indefinite
    ortho = dict(ar.CFRP, poisson_ratios=[4.5, 0.25, 0.4])
    with pytest.raises(SolverError, match="'orthotropic'.*not positive definite"):
        _form(_solver({'orthotropic': ortho}))
    with pytest.raises(SolverError, match="elastic_moduli"):
        _form(_solver({'orthotropic': {'elastic_moduli': [1, 1, 1]}}))
    with pytest.raises(SolverError, match="does not cover"):
        _form(_solver({'elasticity_tensor': {'only': {'subdomain_id': 1, 'value': CFRP_V}}},
                      regions=lambda cen: np.where(cen[:, 2] < 1.0, 1, 2)))


@pytest.mark.parametrize("extra", [{'elastic_modulus': 2e11}, {'poisson_ratio': 0.3}, {'elastic_modulus': 2e11, 'poisson_ratio': 0.3},
                                   {'orthotropic': dict(ar.CFRP)}])
def test_both_key_families_are_refused(extra, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="given together with"):
        _form(_solver(dict({'elasticity_tensor': CFRP_V}, **extra)))


def test_plane_strain_needs_a_monoclinic_material_and_frames_about_z(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    tilted = ar.matrix6(ar.rotate4(ar.tensor4(CFRP_V, ar.VOIGT), ar.rotation_about([1.0, 0.0, 0.0], 0.4)), ar.VOIGT)
    with pytest.raises(SolverError, match="monoclinic about z"):
        _form(_solver({'elasticity_tensor': tilted}, dim=2))
    with pytest.raises(SolverError, match="rotations about z"):
        _form(_solver({'orthotropic': dict(ar.CFRP), 'material_orientation': ar.rotation_about([1.0, 0.0, 0.0], 0.4)}, dim=2))
    about_z = ar.matrix6(ar.rotate4(ar.tensor4(CFRP_V, ar.VOIGT), ar.rotation_about([0.0, 0.0, 1.0], 0.4)), ar.VOIGT)
    F = _form(_solver({'elasticity_tensor': about_z, 'material_orientation': ar.rotation_about([0.0, 0.0, 1.0], -0.4)}, dim=2))
    assert F.anisotropic.table.shape == (1, 6, 6) and F.anisotropic.frames.shape[1:] == (3, 3)


# ---- refusals of the case, each before any device call ---------------------------------------------------------------------------
ANISO = {'orthotropic': dict(ar.CFRP)}


def test_p2_space_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="anisotropic material: P2 displacement spaces are not supported"):
        _solver(ANISO, degree=2, n=(1, 1, 1)).solve()


def test_several_ranks_are_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    solver = _solver(ANISO)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(SolverError, match="anisotropic material runs on one rank"):
        _form(solver)


def test_periodic_space_is_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver(ANISO)
    monkeypatch.setattr(solver.function_space, "periodic_pairs", lambda: (np.array([0]), np.array([1])), raising=False)
    with pytest.raises(SolverError, match="periodic"):
        _form(solver)


@pytest.mark.parametrize("btype", ["contact", "sliding"])
def test_constraint_sides_are_refused_before_any_device_call(btype, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0, 0, 0))}
    bcs["floor"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0)), 'boundary_id': 2, 'type': btype, 'value': 0.0}
    with pytest.raises(SolverError, match="'contact' / 'sliding' boundary conditions \\(floor\\) are not supported"):
        _solver(ANISO, bcs=bcs).solve()


def test_solving_dynamics_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver(ANISO, transient=True)
    solver.solving_dynamics = True
    with pytest.raises(SolverError, match="solving_dynamics"):
        _form(solver)


def test_buckling_and_lame_parameters_are_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver(ANISO)
    with pytest.raises(SolverError, match="solve_buckling.*does not take an anisotropic material"):
        solver.solve_buckling()
    with pytest.raises(SolverError, match="LinearElasticitySolver: lame_parameters.*does not take an anisotropic material"):
        solver.lame_parameters()
    with pytest.raises(SolverError, match="anisotropic"):
        solver.geometric_stiffness()
    with pytest.raises(SolverError, match="isotropic"):
        _solver({'elastic_modulus': 2e11, 'poisson_ratio': 0.3}).stiffness_tensor()


@pytest.mark.parametrize("module,name", [("PlasticitySolver", "PlasticitySolver"), ("ViscoelasticitySolver", "ViscoelasticitySolver"),
                                         ("NonlinearElasticitySolver", "NonlinearElasticitySolver"),
                                         ("ElastodynamicsSolver", "ElastodynamicsSolver"), ("LargeDeformationSolver", "LargeDeformationSolver")])
def test_the_other_solid_solvers_refuse_an_anisotropic_material(module, name, no_device):
    import importlib
    from fenicssolver_amd.SolverBase import SolverError
    cls = getattr(importlib.import_module("fenicssolver_amd." + module), name)
    with pytest.raises(SolverError, match=name + ": .*does not take an anisotropic material"):
        solver = _solver(ANISO, cls=cls, transient=name in ("ElastodynamicsSolver", "LargeDeformationSolver"))
        solver.solve()


# ---- wiring ------------------------------------------------------------------------------------------------------------------------
def test_describe_of_an_isotropic_form_is_unchanged():
    F = _form(_solver({'elastic_modulus': 2e11, 'poisson_ratio': 0.3}, temperature=343.0))
    d = F.describe()
    assert F.anisotropic is None
    assert set(d) == {"type", "mu", "lambda", "body_force", "tractions", "thermal", "load_sign"}
    assert d["mu"] == pytest.approx(fo.lame(2e11, 0.3)[0]) and d["thermal"] is not None


def test_anisotropic_thermal_eigenstrain_is_rotated_into_the_global_axes():
    Rz = ar.rotation_about([0.0, 0.0, 1.0], np.pi / 2)
    mat = {'orthotropic': dict(ar.CFRP), 'material_orientation': Rz, 'thermal_expansion_coefficient': [1e-6, 3e-5, 2e-5]}
    F = _form(_solver(mat, temperature=343.0))
    eps1, T, T_ref = F.anisotropic.thermal
    assert F.thermal is None and (T, T_ref) == (343.0, 293.0)
    # axis 1 points along y: the x expansion is the material's second principal value
    assert np.abs(eps1 - np.array([3e-5, 1e-6, 2e-5, 0, 0, 0])).max() <= 1e-20
    full = {'orthotropic': dict(ar.CFRP), 'thermal_expansion_coefficient': [[1e-6, 2e-6, 0], [2e-6, 3e-5, 0], [0, 0, 2e-5]]}
    assert np.abs(_form(_solver(full, temperature=343.0)).anisotropic.thermal[0][0] - [1e-6, 3e-5, 2e-5, 2e-6, 0, 0]).max() == 0.0
    iso = {'orthotropic': dict(ar.CFRP), 'thermal_expansion_coefficient': 2e-6}
    assert np.abs(_form(_solver(iso, dim=2, n=(3, 2), temperature=343.0)).anisotropic.thermal[0] - [2e-6, 2e-6, 2e-6, 0]).max() == 0.0
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="thermal_expansion_coefficient"):
        _form(_solver(dict(iso, thermal_expansion_coefficient=[1.0, 2.0]), temperature=343.0))


def test_amg_operator_key_digests_the_material():
    s1, s2 = _solver(ANISO), _solver({'orthotropic': dict(ar.CFRP, shear_moduli=[5e9, 4.5e9, 3.5e9])})
    F1, F2 = _form(s1), _form(s2)
    k1, k1b = s1._amg_operator_key(F1, []), s1._amg_operator_key(_form(s1), [])
    assert k1 == k1b and k1[2] == 'anisotropic'
    assert s2._amg_operator_key(F2, [])[3] != k1[3]
    s3 = _solver(dict(ANISO, material_orientation=ar.rotation_about([0, 0, 1.0], 0.1)))
    assert s3._amg_operator_key(_form(s3), [])[3] != k1[3]


# ---- the C interface ---------------------------------------------------------------------------------------------------------------
def test_struct_and_prototypes_match_the_header():
    import ctypes as C
    from fenicssolver_amd import _lib as L
    header = open(os.path.join(ROOT, "include", "fenicssolver_amd.h")).read()
    body = re.search(r"typedef struct fs_aniso_material \{(.*?)\} fs_aniso_material;", header, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = [m.group(1) for m in re.finditer(r"(\w+)\s*;", body)]
    assert names == [f[0] for f in L.fs_aniso_material._fields_] == ["n_materials", "stiffness", "material_of_cell", "frame"]
    assert C.sizeof(L.fs_aniso_material) == 32
    for fn, nargs in (("fs_assemble_anisotropic", 4), ("fs_anisotropic_stress", 7), ("fs_assemble_anisotropic_load", 5)):
        proto = re.search(r"int %s\((.*?)\);" % fn, header, re.S).group(1)
        assert len(proto.split(",")) == nargs == len(L.SIGNATURES[fn][1])
    src = open(os.path.join(ROOT, "fenicssolver_amd", "csrc", "Makefile")).read()
    assert "fs_anisotropic.hip" in src
