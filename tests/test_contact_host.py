"""Frictionless contact and sliding supports of LinearElasticitySolver on the host side (no GPU): the self-checks of the host
reference (tests/contact_reference.py) the GPU tests compare against, the conditions its four fixtures must meet, contact_settings,
the refusals that must come before any device call, the entry points against the header, and the candidate nodes and averaged normals
the solver hands to the device.

What the reference gives on the fixtures (active counts per active set; min active lambda / max lambda; min open gap / max gap):
  strip         18 -> 15 -> 12       0.247   0.134    sum lambda = 1.02777e7 N = 3 * 7.8e3 * 9.81 * 50 - 1.2e6
  oblique       20 -> 16 -> 12 -> 8  0.343   0.0503
  punch         81 -> 9 -> 5         0.0466  0.0262
  plane strain  9 -> 8 -> 7 -> 6     0.177   0.151
"""
import importlib
import os
import re

import numpy as np
import pytest
import scipy.sparse as sp

import contact_reference as cr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EPS = np.finfo(np.float64).eps


# ---- the reference checks itself ---------------------------------------------------------------------------------------------------
def _normals(d):
    rng = np.random.default_rng(7 + d)
    ek = np.zeros(d)
    ek[d - 1] = 1.0
    tilt = np.zeros(d)
    tilt[0] = 1e-9
    generic = rng.standard_normal((40, d))
    zero_k = rng.standard_normal((3, d))
    zero_k[:, d - 1] = 0.0                      # sgn(0) = +1
    return np.concatenate([[ek, -ek, ek + tilt, -ek + tilt, ek - tilt, -ek - tilt], zero_k, generic])


@pytest.mark.parametrize("d", [2, 3])
def test_frames_are_symmetric_orthogonal_and_map_the_normal_onto_the_last_axis(d):
    nrm = _normals(d)
    H, sigma, n = cr.frames(nrm)
    eye = np.eye(d)[None]
    assert np.abs(H - np.transpose(H, (0, 2, 1))).max() == 0.0
    assert np.abs(np.einsum("aij,ajk->aik", H, H) - eye).max() <= 8 * EPS
    assert np.all(np.abs(sigma) == 1.0) and np.array_equal(sigma, np.where(n[:, d - 1] < 0.0, 1.0, -1.0))
    assert sigma[0] == -1.0 and sigma[1] == 1.0 and np.all(sigma[6:9] == -1.0)
    # H e_k = sigma n, hence (H u)_k = sigma n . u for every u
    assert np.abs(H[:, :, d - 1] - sigma[:, None] * n).max() <= 4 * EPS
    u = np.random.default_rng(1).standard_normal((len(n), d))
    hu = np.einsum("aij,aj->ai", H, u)
    assert np.abs(hu[:, d - 1] - sigma * np.einsum("ai,ai->a", n, u)).max() <= 8 * EPS * np.abs(u).max()
    # +-e_k exactly: a reflection of the last axis alone, the other axes untouched
    for a in (0, 1):
        ref = np.eye(d)
        ref[d - 1, d - 1] = -1.0
        assert np.array_equal(H[a], ref)


@pytest.mark.parametrize("d", [2, 3])
def test_rotated_matrix_and_vector_of_the_reference(d):
    rng = np.random.default_rng(d)
    nn = 9
    A = rng.standard_normal((d * nn, d * nn))
    A = A + A.T
    nodes = np.array([0, 3, 8])
    H, _, _ = cr.frames(rng.standard_normal((3, d)))
    Hs = cr.frame_matrix(nn, nodes, H).toarray()
    assert np.abs(Hs @ Hs - np.eye(d * nn)).max() <= 8 * EPS
    Ap = cr.rotate_matrix(sp.csr_matrix(A), nodes, H).toarray()
    assert np.abs(Ap - Hs @ A @ Hs).max() <= 1e-14 * np.abs(A).max()
    assert np.abs(Ap - Ap.T).max() <= 1e-14 * np.abs(A).max()
    v = rng.standard_normal(d * nn)
    assert np.abs(cr.rotate_vector(v, nodes, H) - Hs @ v).max() <= 8 * EPS * np.abs(v).max()
    untouched = np.setdiff1d(np.arange(nn), nodes)
    idx = (d * untouched[:, None] + np.arange(d)).ravel()
    assert np.array_equal(Ap[np.ix_(idx, idx)], A[np.ix_(idx, idx)])


@pytest.fixture(scope="module")
def references():
    return {name: (make(), make().reference()) for name, make in cr.FIXTURES.items()}


@pytest.mark.parametrize("name", list(cr.FIXTURES))
def test_reference_satisfies_the_kkt_conditions_to_rounding(references, name):
    fx, ref = references[name]
    k = cr.kkt(ref["K"], ref["b"], fx.dim, ref["u"], ref["nodes"], ref["normals"], ref["gaps"], ref["active"], ref["dir_dofs"])
    scale = (abs(ref["K"]) @ np.abs(ref["u"])).max()
    print(name, ref["history"], {a: k[a] for a in ("free_residual", "min_lambda", "min_gap", "max_complementarity")}, "scale", scale)
    assert k["free_residual"] <= 1e-12 * scale
    assert k["min_lambda"] > 0.0 and k["min_gap"] > 0.0
    # active nodes sit on the obstacle to rounding, open nodes carry no force at all
    assert k["max_complementarity"] <= 16 * EPS * np.abs(ref["u"]).max() * k["lambda"].max()
    # the multipliers of the loop are the normal components of the residual
    assert np.abs(ref["lam"][ref["active"]] - k["lambda"][ref["active"]]).max() <= 1e-12 * scale
    assert ref["K"].shape[0] <= 729


@pytest.mark.parametrize("name", list(cr.FIXTURES))
def test_fixture_conditions(references, name):
    """Conditions on the fixtures, not measurements: a case with every or no node in contact, or with a node that sits on the fence,
    would not tell a right active set from a wrong one."""
    fx, ref = references[name]
    n_active, n_cand, lam_margin, gap_margin = cr.fixture_margins(ref)
    print(name, ref["history"], n_active, n_cand, lam_margin, gap_margin)
    assert 0 < n_active < n_cand
    assert lam_margin >= 1e-2 and gap_margin >= 1e-2
    assert 3 <= ref["iterations"] <= 5


def test_strip_carries_the_applied_normal_load(references):
    fx, ref = references["strip"]
    load = 3.0 * cr.BODY - cr.STRIP_LIFT               # weight of the 3 x 1 x 1 strip less the lift on its 1 x 1 end face, N
    assert abs(ref["lam"][ref["active"]].sum() - load) <= 1e-7 * load


def test_expected_histories(references):
    assert references["strip"][1]["history"] == [18, 15, 12]
    assert references["punch"][1]["history"] == [81, 9, 5]
    assert len(references["oblique"][1]["nodes"]) == 20


# ---- settings ----------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def no_device(monkeypatch):
    """Every entry point that would reach the GPU fails the test."""
    from fenicssolver_amd import backend
    from fenicssolver_amd import fem

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    for name in ("DeviceMatrix", "DeviceVector", "DeviceSpace", "DeviceMesh", "AMG", "ContactFrames", "contact_update", "eigen_solve",
                 "buckling_solve", "krylov_solve", "synchronize", "init"):
        monkeypatch.setattr(backend, name, boom)
    monkeypatch.setattr(fem.FunctionSpace, "device", boom, raising=False)
    return boom


def test_contact_settings_defaults():
    assert cr.make_solver(cr.strip()).contact_settings() == {'max_iterations': 30, 'initial_active': 'all'}
    cs = cr.make_solver(cr.strip(), contact_settings={'max_iterations': 7, 'initial_active': 'none'}).contact_settings()
    assert cs == {'max_iterations': 7, 'initial_active': 'none'}


@pytest.mark.parametrize("bad", [{'max_iterations': 0}, {'max_iterations': -3}, {'max_iterations': 2.5}, {'max_iterations': True},
                                 {'max_iterations': '30'}, {'initial_active': 'some'}, {'initial_active': True}, {'tolerance': 1e-8},
                                 {'iterations': 3}])
def test_contact_settings_range_checks(bad, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="contact_settings"):
        cr.make_solver(cr.strip(), contact_settings=bad).solve()


# ---- refusals, each before any device call -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["contact", "sliding"])
def test_p2_space_is_refused_before_any_device_call(no_device, kind):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="P2 displacement spaces are not supported"):
        cr.make_solver(cr.strip(), degree=2, contact_type=kind).solve()


def test_several_ranks_are_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    solver = cr.make_solver(cr.strip())
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve()


def test_periodic_space_is_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = cr.make_solver(cr.strip())
    monkeypatch.setattr(solver.function_space, "periodic_pairs", lambda: (np.array([0]), np.array([1])), raising=False)
    with pytest.raises(SolverError, match="periodic"):
        solver.solve()


def test_transient_case_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="transient"):
        cr.make_solver(cr.strip(), transient=True).solve()


@pytest.mark.parametrize("kind", ["contact", "sliding"])
def test_modal_and_buckling_with_a_constraint_side_are_refused(no_device, kind):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="solve_modal: contact / sliding boundary conditions \\(base\\) are not supported"):
        cr.make_solver(cr.strip(), contact_type=kind).solve_modal()
    with pytest.raises(SolverError, match="solve_buckling: contact / sliding boundary conditions \\(base\\) are not supported"):
        cr.make_solver(cr.strip(), contact_type=kind).solve_buckling()


@pytest.mark.parametrize("normal", [(0.0, 0.0, 0.0), (0.0, 0.0), (np.nan, 0.0, 1.0)])
def test_zero_or_ill_shaped_normal_is_refused(no_device, normal):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="normal"):
        cr.make_solver(cr.strip(), normal=normal).solve()


def test_a_marker_without_facets_is_refused(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    fx = cr.strip()
    fx.on_contact = lambda x: np.zeros(len(x), dtype=bool)
    with pytest.raises(SolverError, match="no facet carries marker"):
        cr.make_solver(fx).solve()


def test_a_side_without_a_candidate_left_is_refused(no_device):
    """One hexahedron held on its faces x = 0 and x = 1: every vertex of the face z = 0 carries a displacement BC, and Dirichlet wins."""
    from fenicssolver_amd.SolverBase import SolverError
    from oracle import fem_oracle as fo
    co, ce = fo.box_mesh((0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 1, 1, 1)
    fx = cr.Fixture("cube", 3, co, ce, None, [(lambda x: (np.abs(x[:, 0]) < 1e-9) | (np.abs(x[:, 0] - 1.0) < 1e-9), (0.0, 0.0, 0.0))],
                    lambda x: np.abs(x[:, 2]) < 1e-9, (0.0, 0.0, -1.0), lambda x: 0.0 * x[:, 0], (0.0, 0.0, 0.0), None, None)
    with pytest.raises(SolverError, match="no candidate node is left"):
        cr.make_solver(fx).solve()


def test_bad_value_is_refused(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = cr.make_solver(cr.strip())
    solver.boundary_conditions["base"]["value"] = [1.0, 2.0]
    with pytest.raises(SolverError, match="value must be"):
        solver.solve()


@pytest.mark.parametrize("module", ["NonlinearElasticitySolver", "PlasticitySolver", "ViscoelasticitySolver", "ElastodynamicsSolver",
                                    "LargeDeformationSolver"])
@pytest.mark.parametrize("kind", ["contact", "sliding"])
def test_the_other_solid_solvers_keep_refusing_both_types(no_device, module, kind):
    from fenicssolver_amd.SolverBase import SolverError
    cls = getattr(importlib.import_module("fenicssolver_amd." + module), module)
    solver = cr.make_solver(cr.strip(), cls=cls, contact_type=kind)
    with pytest.raises(SolverError, match="boundary type`%s` is not supported" % kind):
        solver.update_boundary_conditions(0, None, None, None)


def test_results_are_refused_before_a_solve():
    from fenicssolver_amd.SolverBase import SolverError
    solver = cr.make_solver(cr.strip())
    for call in (solver.contact_forces, solver.contact_pressure, solver.contact_status):
        with pytest.raises(SolverError, match="no contact result"):
            call()


# ---- the C interface -----------------------------------------------------------------------------------------------------------------
def _header_prototype(name):
    header = open(os.path.join(ROOT, "include", "fenicssolver_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    m = re.search(r"\bint\s+%s\s*\((.*?)\)\s*;" % name, header, flags=re.S)
    assert m, name
    return [a.strip() for a in m.group(1).split(",")]


def test_contact_entry_points_are_bound_as_the_header_declares_them():
    import ctypes as C
    from fenicssolver_amd import _lib, backend
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    lib = _lib.load()
    handle = ("fs_space_t", "fs_matrix_t", "fs_vector_t", "fs_contact_t")

    def ctype(decl):
        t = decl.rsplit(" ", 1)[0].replace("const ", "").strip()
        if t in handle:
            return C.c_void_p
        return {"int64_t": C.c_int64, "int32_t*": _lib.c_i32p, "double*": _lib.c_f64p, "fs_contact_t*": C.POINTER(C.c_void_p)}[t]
    for name in ("fs_contact_create", "fs_contact_destroy", "fs_contact_get", "fs_matrix_rotate_nodes",
                 "fs_vector_rotate_nodes", "fs_contact_update"):
        assert name in _lib.SIGNATURES and hasattr(lib, name), name
        res, args = _lib.SIGNATURES[name]
        assert res is C.c_int
        assert [ctype(a) for a in _header_prototype(name)] == args, name
    assert hasattr(backend, "ContactFrames") and hasattr(backend, "contact_update")
    assert hasattr(backend.DeviceMatrix, "rotate_nodes") and hasattr(backend.DeviceVector, "rotate_nodes")
    for name in ("solve_contact", "contact_settings", "contact_forces", "contact_pressure", "contact_status"):
        assert hasattr(LinearElasticitySolver, name)
    src = open(os.path.join(ROOT, "fenicssolver_amd", "csrc", "Makefile")).read()
    assert "fs_contact.hip" in src


# ---- what the solver hands to the device -----------------------------------------------------------------------------------------------
def _setup(solver):
    solver.init_solver()
    F, bcs = solver.generate_form(0, None, None, solver.w_current, solver.w_prev)
    return solver._contact, bcs


@pytest.mark.parametrize("name", list(cr.FIXTURES))
def test_candidates_normals_and_gaps_of_the_fixtures(no_device, name):
    """Candidates: the vertices of the marked facets less those with a displacement BC.  The oblique fixture gives no normal: the
    area-weighted mean of the facet normals is the rotated (0, 0, -1) at every node of the flat face, to rounding."""
    fx = cr.FIXTURES[name]()
    K, b, dofs, vals, cand, normals, gaps = fx.system()
    C_, bcs = _setup(cr.make_solver(fx))
    assert np.array_equal(C_["nodes"], cand)
    assert np.abs(np.linalg.norm(C_["normals"], axis=1) - 1.0).max() <= 4 * EPS
    assert np.abs(C_["normals"] - normals).max() <= 8 * EPS
    assert np.abs(C_["values"] - gaps).max() <= 4 * EPS * np.abs(gaps).max()
    assert not C_["bilateral"].any()
    bf = fx.facets_on(fx.on_contact)
    assert np.abs(C_["area"] - cr.lumped_areas(fx.coords, bf)[cand]).max() <= 8 * EPS
    # the user's Dirichlet dofs are the reference's
    got = np.unique(np.concatenate([bc.dofs for bc in bcs]))
    assert np.array_equal(got, np.unique(dofs))


def test_averaged_normals_on_a_box_face_and_on_a_rotated_box(no_device):
    """Omitted normals: outward, unit, area-weighted.  On the z = 0 face of the axis-aligned punch box they are (0, 0, -1) exactly
    up to the sign of zero; on the rotated box R (0, 0, -1)."""
    fx = cr.punch()
    C_, _ = _setup(cr.make_solver(fx, normal=None))
    assert np.array_equal(C_["normals"], np.tile([0.0, 0.0, -1.0], (len(C_["nodes"]), 1)))
    fo_ = cr.oblique()
    C2, _ = _setup(cr.make_solver(fo_))
    assert np.abs(C2["normals"] - (fo_.R @ np.array([0.0, 0.0, -1.0]))[None, :]).max() <= 8 * EPS
    # a side that bends round an edge of the box: the mean of the two face normals on the edge, each face's own elsewhere
    fx3 = cr.punch()
    fx3.dirichlet = [(lambda x: np.abs(x[:, 2] - 0.25) < 1e-9, (0.0, 0.0, 0.0))]
    fx3.on_contact = lambda x: (np.abs(x[:, 2]) < 1e-9) | (np.abs(x[:, 0]) < 1e-9)
    C3, _ = _setup(cr.make_solver(fx3, normal=None))
    co = fx3.coords[C3["nodes"]]
    edge = (np.abs(co[:, 2]) < 1e-9) & (np.abs(co[:, 0]) < 1e-9)
    assert edge.sum() == 9
    assert np.abs(C3["normals"][edge] - np.array([-1.0, 0.0, -1.0]) / np.sqrt(2.0)).max() <= 4 * EPS
    assert np.array_equal(C3["normals"][~edge & (np.abs(co[:, 2]) < 1e-9)], np.tile([0.0, 0.0, -1.0], ((~edge & (np.abs(co[:, 2]) < 1e-9)).sum(), 1)))


def test_dirichlet_wins_and_an_earlier_side_keeps_shared_nodes(no_device):
    from fenicssolver_amd.fem import AutoSubDomain
    fx = cr.punch()
    wall = {'boundary': AutoSubDomain(lambda x: abs(x[0]) < 1e-9), 'boundary_id': 9, 'type': 'sliding', 'normal': (-1.0, 0.0, 0.0),
            'value': 1e-4}
    C_, _ = _setup(cr.make_solver(fx, extra_bcs={'wall': wall}))
    co = fx.coords
    base = np.flatnonzero(np.abs(co[:, 2]) < 1e-9)
    on_wall = np.flatnonzero((np.abs(co[:, 0]) < 1e-9) & (np.abs(co[:, 2]) > 1e-9) & (np.abs(co[:, 2] - 0.25) > 1e-9))
    assert np.array_equal(C_["nodes"], np.union1d(base, on_wall))
    is_wall = np.isin(C_["nodes"], on_wall)
    assert np.array_equal(C_["bilateral"], is_wall)
    assert np.all(C_["values"][is_wall] == 1e-4) and np.all(C_["normals"][is_wall] == np.array([-1.0, 0.0, 0.0]))
    assert C_["names"] == ["base", "wall"]
