"""ScalarTransportDGSolver on the host side (no GPU): the numpy restatement of the DG form against an exact linear state, the '+'
rule, the DG1 dof layout, the refusals and the main() dispatch."""
import copy
import os

import numpy as np
import pytest

import dg_reference as dr

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _xml_mesh():
    from fenicssolver_amd.fem import Mesh
    return Mesh(os.path.join(ROOT, "tests", "golden", "data", "mesh.xml"))


def _rect_mesh():
    from fenicssolver_amd.fem import RectangleMesh, Point
    return RectangleMesh(Point(0.0, 0.0), Point(2.0, 1.0), 12, 7)


def _linear_state(mesh, rng):
    d = mesh.geometry().dim()
    a = rng.uniform(0.5, 1.5, d)
    t0 = 1.7
    co = mesh.coordinates()[mesh.cells().ravel()]
    return a, t0, co @ a + t0


@pytest.mark.parametrize("which", ["xml3d", "rect2d"])
@pytest.mark.parametrize("transient", [False, True])
def test_exact_linear_state_satisfies_the_restated_system(which, transient):
    mesh = _xml_mesh() if which == "xml3d" else _rect_mesh()
    rng = np.random.default_rng(5)
    d = mesh.geometry().dim()
    a, t0, Tstar = _linear_state(mesh, rng)
    k, c = 0.3, 2.0
    beta = rng.uniform(-1.0, 1.0, d)
    alpha = 500.0 if d == 3 else 5.0
    nl = d + 1
    src = np.full(mesh.num_cells() * nl, c * float(beta @ a))
    dt = 0.05
    op, mass = (0.5, c / dt) if transient else (1.0, 0.0)
    A, b = dr.assemble(mesh, k, c, beta, alpha, op=op, mass=mass, source=src)
    if transient:
        B, _ = dr.assemble(mesh, k, c, beta, alpha, op=-0.5, mass=c / dt)
        b = b + B @ Tstar
    dofs = dr.geometric_dirichlet_dofs(mesh, np.nonzero(mesh.exterior_facets())[0])
    assert 0 < len(dofs) < len(Tstar)
    A, b = dr.apply_dirichlet(A, b, dofs, Tstar[dofs])
    res = A @ Tstar - b
    scale = abs(A) @ np.abs(Tstar)
    assert np.max(np.abs(res) / scale) <= 1e-12


def test_plus_rule_moves_the_matrix_only_where_h_differs():
    """Swapping the '+' side of every interior facet changes the penalty h+ and nothing else: the difference of the two matrices
    lives exactly in the blocks of the facets whose two cells have different h; a marker difference across a facet picks '+'."""
    mesh = _xml_mesh()
    nc = mesh.num_cells()
    args = (0.4, 1.3, np.array([0.3, -0.2, 0.5]), 500.0)
    A0, _ = dr.assemble(mesh, *args)
    A1, _ = dr.assemble(mesh, *args, key=np.arange(nc))          # the higher number is '+' everywhere
    D = (A1 - A0).tocoo()
    X = mesh.coordinates()[mesh.cells()]
    h = dr.circum_h(X)
    pairs, _ = mesh.interior_facet_cells()
    differ = np.abs(h[pairs[:, 0]] - h[pairs[:, 1]]) > 1e-12 * h.max()
    assert differ.any() and (~differ).any()
    touched = set()
    for p, q in pairs[differ]:
        touched.update([(int(p), int(q)), (int(q), int(p)), (int(p), int(p)), (int(q), int(q))])
    big = np.abs(D.data) > 1e-12 * abs(A0).max()
    cells_hit = set(zip((D.row[big] // 4).tolist(), (D.col[big] // 4).tolist()))
    assert cells_hit and cells_hit <= touched
    # cross blocks of a facet whose cells have equal h do not move
    for p, q in pairs[~differ][:50]:
        assert np.abs((A1 - A0)[p * 4:(p + 1) * 4, q * 4:(q + 1) * 4].toarray()).max() <= 1e-12 * abs(A0).max()
    # markers: the cell with the larger marker is '+', whatever the numbering
    mk = np.zeros(nc, dtype=np.int64)
    mk[pairs[differ][0, 1]] = 1
    key_mk = mk * nc - np.arange(nc)
    A2, _ = dr.assemble(mesh, *args, key=key_mk)
    p, q = pairs[differ][0]
    blk = lambda A: A[p * 4:(p + 1) * 4, q * 4:(q + 1) * 4].toarray()     # noqa: E731
    assert np.abs(blk(A2) - blk(A1)).max() <= 1e-12 * abs(A0).max()
    assert np.abs(blk(A2) - blk(A0)).max() > 1e-9 * abs(A0).max()


def test_dg_space_layout_and_node_coordinates():
    from fenicssolver_amd.fem import FunctionSpace, Function, Expression, interpolate, DGFunctionSpace
    mesh = _rect_mesh()
    V = FunctionSpace(mesh, "DG", 1)
    assert isinstance(V, DGFunctionSpace)
    assert isinstance(FunctionSpace(mesh, "Discontinuous Lagrange", 1), DGFunctionSpace)
    assert V.dim() == 3 * mesh.num_cells()
    assert V.ufl_element().family() == "Discontinuous Lagrange"
    cells = mesh.cells()
    assert np.array_equal(V.node_coordinates(), mesh.coordinates()[cells.ravel()])
    assert np.array_equal(V.cell_nodes(), np.arange(V.dim()).reshape(-1, 3))
    f = interpolate(Expression("x[0] + 2*x[1]", degree=1), V)
    co = V.node_coordinates()
    assert np.allclose(f.vector().get_local(), co[:, 0] + 2 * co[:, 1], rtol=0, atol=1e-14)
    assert Function(V).vector().size() == V.dim()
    # geometric rule: every dof of a vertex on the marked facets
    ext = np.nonzero(mesh.exterior_facets())[0]
    dofs = V.facet_nodes(ext)
    bverts = set(np.unique(mesh.facets()[ext]).tolist())
    assert set(cells.ravel()[dofs].tolist()) == bverts
    assert all(cells.ravel()[i] not in bverts for i in np.setdiff1d(np.arange(V.dim()), dofs))


@pytest.mark.parametrize("family, degree", [("DG", 2), ("DG", 0)])
def test_dg_degrees_other_than_one_are_refused(family, degree):
    from fenicssolver_amd.fem import FunctionSpace
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="DG1 only"):
        FunctionSpace(_rect_mesh(), family, degree)


def _case(**over):
    from fenicssolver_amd.fem import UnitSquareMesh, AutoSubDomain
    s = {
        "solver_name": "ScalarTransportDGSolver", "scalar_name": "temperature", "case_name": "dg", "case_folder": "/tmp/",
        "mesh": UnitSquareMesh(4, 4), "fe_degree": 1, "fe_family": "DG", "periodic_boundary": None,
        "boundary_conditions": {"all": {"boundary_id": 1, "type": "Dirichlet", "value": 1.0,
                                        "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary)}},
        "body_source": None, "surface_source": None, "initial_values": {},
        "material": {"density": 1.0, "specific_heat_capacity": 2.0, "thermal_conductivity": 0.5},
        "convective_velocity": (1.0, 0.5),
        "solver_settings": {"transient_settings": {"transient": False, "starting_time": 0, "time_step": 0.1, "ending_time": 0.3},
                            "reference_values": {}, "solver_parameters": {}},
        "report_settings": dict(QUIET),
    }
    s.update(over)
    return s


def _no_device(monkeypatch):
    from fenicssolver_amd import backend, _lib

    def refuse(*a, **k):
        raise AssertionError("a device call was made")
    monkeypatch.setattr(_lib, "load", refuse)
    monkeypatch.setattr(backend.DeviceMatrix, "__init__", refuse)
    monkeypatch.setattr(backend.DeviceDGSpace, "__init__", refuse)


@pytest.mark.parametrize("over, match", [
    ({"fe_degree": 2}, "fe_degree 2"),
    ({"convective_velocity": None}, "convective_velocity is required"),
    ({"convective_velocity": ("x[0]", "0")}, "constant vector"),
    ({"material": {"density": 1.0, "specific_heat_capacity": 2.0, "thermal_conductivity": lambda T: 1 + T}}, "conductivity"),
    ({"material": {"density": 1.0, "specific_heat_capacity": 2.0, "thermal_conductivity": [[1, 0], [0, 2]]}}, "conductivity"),
    ({"material": {"density": 1.0, "specific_heat_capacity": 2.0,
                   "thermal_conductivity": {"a": {"subdomain_id": 0, "value": 1.0}}}}, "conductivity"),
    ({"material": {"capacity": lambda T: 1 + T, "thermal_conductivity": 0.5}}, "capacity"),
    ({"point_source": [((0.5, 0.5), 1.0)]}, "point_source"),
    ({"surface_source": {"value": 1.0}}, "surface_source"),
    ({"radiation_settings": {"ambient_temperature": 300.0}}, "radiation_settings"),
    ({"advection_settings": {"stabilization_method": "SPUG", "Pe": 1.0}}, "stabilisation"),
])
def test_refusals_raise_before_any_device_call(monkeypatch, over, match):
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    with pytest.raises(SolverError, match=match):
        ScalarTransportDGSolver(_case(**over)).solve()


def test_refusal_of_several_ranks_and_vector_spaces(monkeypatch):
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    _no_device(monkeypatch)
    solver = ScalarTransportDGSolver(_case())
    monkeypatch.setattr(parallel, "world", lambda: (0, 2, None))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve()
    monkeypatch.undo()
    _no_device(monkeypatch)
    s = _case()
    s.pop("scalar_name")
    s["vector_name"] = "displacement"
    with pytest.raises(SolverError, match="vector-valued"):
        ScalarTransportDGSolver(s)


def test_refusal_of_periodic_spaces(monkeypatch):
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import SubDomain, near

    class PeriodicY(SubDomain):
        def inside(self, x, on_boundary):
            return near(x[1], 0.0) and on_boundary

        def map(self, x, y):
            y[0], y[1] = x[0], x[1] - 1.0
    _no_device(monkeypatch)
    with pytest.raises(SolverError, match="periodic"):
        ScalarTransportDGSolver(_case(periodic_boundary=PeriodicY())).solve()


def test_main_dispatches_to_the_dg_solver(monkeypatch):
    import importlib
    M = importlib.import_module("fenicssolver_amd.main")
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    assert "ScalarTransportDGSolver" in M._SOLVERS
    seen = []
    monkeypatch.setattr(ScalarTransportDGSolver, "solve", lambda self: seen.append(type(self).__name__))
    monkeypatch.setattr(ScalarTransportDGSolver, "plot", lambda self: None)
    solver = M.main(copy.deepcopy(_case()))
    assert seen == ["ScalarTransportDGSolver"] and isinstance(solver, ScalarTransportDGSolver)
    assert type(solver.function_space).__name__ == "DGFunctionSpace"
    assert solver.function_space_CG.ufl_element().family() == "Lagrange"


def test_varying_boundary_data_is_taken_at_the_mesh_vertices():
    """Neumann / flux / HTC-ambient values that vary: the value at every facet vertex, whether given as an Expression or as an
    expression string (which the settings turn into a Function on the DG space)."""
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    from fenicssolver_amd.fem import Expression
    solver = ScalarTransportDGSolver(_case())
    mesh = solver.mesh
    tri = mesh.facets()[solver.boundary_facets.where(1)].astype(np.int64)
    co = mesh.coordinates()
    want = co[tri][..., 0] + 10.0 * co[tri][..., 1]
    got = solver._facet_value(Expression("x[0] + 10*x[1]", degree=1), 1, "flux")
    assert np.abs(got - want).max() <= 1e-13
    got = solver._facet_value(solver.translate_value("x[0] + 10*x[1]"), 1, "flux")
    assert np.abs(got - want).max() <= 1e-13


@pytest.mark.parametrize("pc", ["petsc_amg", "amg", "hypre_amg"])
def test_amg_preconditioner_is_refused(monkeypatch, pc):
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    from fenicssolver_amd.SolverBase import SolverError
    _no_device(monkeypatch)
    s = _case()
    s["solver_settings"]["solver_parameters"] = {"preconditioner": pc}
    with pytest.raises(SolverError, match="no AMG for DG"):
        ScalarTransportDGSolver(s).solve()
