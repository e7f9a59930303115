"""ScalarTransportDGSolver on the MI355X: the DG1 cell-block assembly against the numpy restatement (tests/dg_reference.py), the
block product, block-Jacobi BiCGStab, the exact linear state through solve(), an advection-dominated case end to end and a full-size
box."""
import os
import time

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.linalg import spsolve

import dg_reference as dr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DATA = os.path.join(ROOT, "tests", "golden", "data")


@pytest.fixture(scope="module", autouse=True)
def _device():
    from fenicssolver_amd import backend
    backend.init(0)


def _xml_mesh():
    from fenicssolver_amd.fem import Mesh, MeshFunction
    mesh = Mesh(os.path.join(DATA, "mesh.xml"))
    regions = np.asarray(MeshFunction("size_t", mesh, os.path.join(DATA, "mesh_physical_region.xml")).array(), dtype=np.int64)
    # the file holds one region: a second one (cells right of the median centroid) makes the markers differ across facets
    cx = mesh.coordinates()[mesh.cells()].mean(axis=1)[:, 0]
    return mesh, regions + (cx > np.median(cx))


def _meshes():
    from fenicssolver_amd.fem import UnitCubeMesh, RectangleMesh, Point
    xml, regions = _xml_mesh()
    return {"xml": (xml, regions), "cube": (UnitCubeMesh(5, 4, 3), None),
            "rect": (RectangleMesh(Point(0.0, 0.0), Point(2.0, 1.0), 11, 6), None)}


def _inputs(mesh, rng):
    """facet lists (flux / Neumann loads on one half of the boundary, HTC on the other), a per-dof body source"""
    nc, nl = mesh.cells().shape
    cf = mesh.cell_facets().astype(np.int64)
    bc, bl = np.nonzero(mesh.exterior_facets()[cf])
    half = len(bc) // 2
    h = np.concatenate([np.zeros(half), rng.uniform(0.5, 2.0, len(bc) - half)])
    g = rng.uniform(-1.0, 1.0, (len(bc), nl))
    src = rng.uniform(0.0, 2.0, nc * nl)
    return bc, bl, h, g, src


def _device_system(V, rec, params, bc, bl, h, g, src):
    """(A, b) assembled on the device, exported and permuted to the API dof order"""
    from fenicssolver_amd import backend
    n = V.dim()
    cell_a2d = np.empty(len(rec.cell_order), dtype=np.int64)
    cell_a2d[rec.cell_order.astype(np.int64)] = np.arange(len(rec.cell_order))
    A = backend.DeviceDGMatrix(rec.space)
    b = backend.DeviceVector(n)
    A.assemble_transport(b, facet_cell=cell_a2d[bc], facet_local=bl, facet_h=h, facet_g=g, source=src[rec.device_to_dof], **params)
    rp, ci, va, _ = A.to_csr()
    Ad = sp.csr_matrix((va, ci, rp), shape=(n, n))
    P = rec.dof_to_device
    return Ad[P][:, P], b.get(n)[P], A, b


PARAMS = dict(conductivity=0.7, capacity=1.9, velocity=(0.4, -0.3, 0.25), operator_scale=1.0, mass_scale=0.0)


@pytest.mark.parametrize("name", ["xml", "cube", "rect"])
@pytest.mark.parametrize("transient", [False, True])
def test_assembly_matches_the_host_restatement(name, transient):
    from fenicssolver_amd.fem import FunctionSpace
    mesh, regions = _meshes()[name]
    d = mesh.geometry().dim()
    rng = np.random.default_rng(11)
    bc, bl, h, g, src = _inputs(mesh, rng)
    params = dict(PARAMS, alpha=500.0 if d == 3 else 5.0)
    if transient:
        params.update(operator_scale=0.5, mass_scale=1.9 / 0.02)
    V = FunctionSpace(mesh, "DG", 1)
    if regions is not None:
        V.set_cell_markers(regions)
    rec = V.device()
    A, b, _, _ = _device_system(V, rec, params, bc, bl, h, g, src)
    key = V.plus_key()
    Ah, bh = dr.assemble(mesh, params["conductivity"], params["capacity"], params["velocity"], params["alpha"],
                         op=params["operator_scale"], mass=params["mass_scale"], facet_cell=bc, facet_local=bl, facet_h=h,
                         facet_g=g, source=src, key=key)
    scale = abs(Ah).max()
    diff = (A - Ah).tocoo()
    assert A.nnz >= Ah.nnz - (Ah.data == 0).sum()
    assert np.abs(diff.data).max(initial=0.0) <= 1e-12 * scale
    assert np.abs(b - bh).max() <= 1e-12 * np.abs(bh).max()
    if regions is not None:
        assert len(np.unique(regions)) > 1


def test_file_order_and_locality_order_give_the_same_values():
    from fenicssolver_amd.fem import FunctionSpace
    mesh, regions = _xml_mesh()
    rng = np.random.default_rng(3)
    bc, bl, h, g, src = _inputs(mesh, rng)
    params = dict(PARAMS, alpha=500.0)
    out = []
    for renumber in (False, True):
        V = FunctionSpace(mesh, "DG", 1)
        V.set_cell_markers(regions)
        rec = V.device(renumber=renumber)
        assert renumber == (not np.array_equal(rec.cell_order, np.arange(mesh.num_cells())))
        A, b, _, _ = _device_system(V, rec, params, bc, bl, h, g, src)
        out.append((A, b))
    scale = abs(out[0][0]).max()
    assert abs(out[0][0] - out[1][0]).max() <= 1e-14 * scale
    assert np.abs(out[0][1] - out[1][1]).max() <= 1e-14 * np.abs(out[0][1]).max()


def test_assembly_is_deterministic_and_the_product_matches_the_host():
    from fenicssolver_amd import backend
    from fenicssolver_amd.fem import FunctionSpace, UnitCubeMesh
    mesh = UnitCubeMesh(9, 8, 7)
    rng = np.random.default_rng(2)
    bc, bl, h, g, src = _inputs(mesh, rng)
    V = FunctionSpace(mesh, "DG", 1)
    rec = V.device()
    params = dict(PARAMS, alpha=500.0)
    _, _, A1, b1 = _device_system(V, rec, params, bc, bl, h, g, src)
    _, _, A2, b2 = _device_system(V, rec, params, bc, bl, h, g, src)
    v1, v2 = A1.to_csr()[2], A2.to_csr()[2]
    assert np.array_equal(v1.view(np.uint64), v2.view(np.uint64))
    assert np.array_equal(b1.get().view(np.uint64), b2.get().view(np.uint64))
    n = V.dim()
    rp, ci, va, _ = A1.to_csr()
    Ad = sp.csr_matrix((va, ci, rp), shape=(n, n))
    x = rng.standard_normal(n)
    xd = backend.DeviceVector(n + 256, np.concatenate([x, np.full(256, np.nan)]))    # poisoned tail behind n
    y = backend.DeviceVector(n)
    A1.spmv(xd, y)
    ref = Ad @ x
    assert np.isfinite(y.get()).all()
    assert np.abs(y.get() - ref).max() <= 1e-14 * (abs(Ad) @ np.abs(x)).max()
    assert backend.last_product_kind() == 6


@pytest.mark.parametrize("name", ["xml", "rect"])
def test_block_jacobi_bicgstab_matches_a_direct_solve(name):
    from fenicssolver_amd import backend
    from fenicssolver_amd.fem import FunctionSpace
    mesh, regions = _meshes()[name]
    d = mesh.geometry().dim()
    rng = np.random.default_rng(4)
    bc, bl, h, g, src = _inputs(mesh, rng)
    params = dict(PARAMS, alpha=500.0 if d == 3 else 5.0)
    V = FunctionSpace(mesh, "DG", 1)
    rec = V.device()
    _, _, A, b = _device_system(V, rec, params, bc, bl, h, g, src)
    dofs = dr.geometric_dirichlet_dofs(mesh, np.nonzero(mesh.exterior_facets())[0])[::3]
    vals = rng.uniform(-1.0, 1.0, len(dofs))
    A.apply_dirichlet(b, rec.dof_to_device[dofs], vals)
    Ah, bh = dr.assemble(mesh, params["conductivity"], params["capacity"], params["velocity"], params["alpha"], facet_cell=bc,
                         facet_local=bl, facet_h=h, facet_g=g, source=src, key=V.plus_key())
    Ah, bh = dr.apply_dirichlet(Ah, bh, dofs, vals)
    xh = spsolve(Ah.tocsc(), bh)
    n = V.dim()
    sols = []
    for pc in ("block_jacobi", "jacobi"):
        x = backend.DeviceVector(n)
        st = backend.dg_krylov_solve(A, b, x, rtol=1e-12, max_iter=20000, precond=pc)
        assert st["converged"] == 1 and st["true_rel_residual"] <= 1e-10, st
        assert st["product_kind"] == 6 and st["spmv_bytes"] > 0
        xs = x.get(n)[rec.dof_to_device]
        assert np.abs(xs - xh).max() <= 1e-9 * np.abs(xh).max()
        sols.append((xs, st["iterations"]))
    print("iterations block-Jacobi %d, point Jacobi %d" % (sols[0][1], sols[1][1]))


def _case(mesh, d, transient=False, kappa=0.5, beta=None, a=None, t0=2.0, bcs=None, source=True):
    from fenicssolver_amd.fem import AutoSubDomain, Expression
    beta = np.asarray(beta if beta is not None else ([0.6, -0.4, 0.3][:d]), dtype=np.float64)
    a = np.asarray(a if a is not None else ([0.8, 1.3, -0.6][:d]), dtype=np.float64)
    c = 2.0 * 1.5
    expr = "+".join("%r*x[%d]" % (float(a[i]), i) for i in range(d)) + "+%r" % t0
    if bcs is None:
        bcs = {"all": {"boundary_id": 1, "type": "Dirichlet", "value": Expression(expr, degree=1),
                       "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary)}}
    s = {
        "solver_name": "ScalarTransportDGSolver", "scalar_name": "temperature", "case_name": "dg", "case_folder": "/tmp/",
        "mesh": mesh, "fe_degree": 1, "fe_family": "DG", "periodic_boundary": None, "boundary_conditions": bcs,
        "body_source": c * float(beta @ a) if source else None, "surface_source": None,
        "initial_values": {"temperature": expr} if transient else {},
        "material": {"density": 2.0, "specific_heat_capacity": 1.5, "thermal_conductivity": kappa * c},
        "convective_velocity": tuple(float(v) for v in beta),
        "solver_settings": {"transient_settings": {"transient": transient, "starting_time": 0, "time_step": 0.05, "ending_time": 0.15},
                            "reference_values": {}, "solver_parameters": {}},
        "report_settings": dict(QUIET),
    }
    return s, a, t0


@pytest.mark.parametrize("dim", [2, 3])
@pytest.mark.parametrize("transient", [False, True])
def test_exact_linear_state_through_solve(dim, transient):
    from fenicssolver_amd.fem import UnitCubeMesh, UnitSquareMesh
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    mesh = UnitCubeMesh(6, 5, 4) if dim == 3 else UnitSquareMesh(12, 9)
    s, a, t0 = _case(mesh, dim, transient=transient)
    solver = ScalarTransportDGSolver(s)
    P = solver.solve()
    if transient:
        assert solver.current_step == 3
    V = solver.function_space
    Tstar = V.node_coordinates() @ a + t0
    T = solver.w_current.vector().get_local()
    assert np.abs(T - Tstar).max() <= 1e-10 * np.abs(Tstar).max()
    Pstar = mesh.coordinates() @ a + t0
    assert np.abs(P.vector().get_local() - Pstar).max() <= 1e-10 * np.abs(Pstar).max()
    assert P.function_space() is solver.function_space_CG


def test_advection_dominated_case_end_to_end(tmp_path):
    from fenicssolver_amd.fem import UnitCubeMesh, AutoSubDomain, near
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    mesh = UnitCubeMesh(8, 7, 6)
    beta = np.array([1.0, 0.4, 0.2])
    hmin = mesh.hmin()
    kappa = 1e-3 * np.linalg.norm(beta) * hmin
    bcs = {"inlet": {"boundary_id": 1, "type": "Dirichlet", "value": 1.0,
                     "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary and near(x[0], 0.0))},
           "cooled": {"boundary_id": 2, "type": "HTC", "value": 3.0, "ambient": 0.2,
                      "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary and near(x[1], 1.0))}}
    s, _, _ = _case(mesh, 3, kappa=kappa, beta=beta, bcs=bcs, source=False)
    s["body_source"] = 0.5
    s["report_settings"] = dict(QUIET, result_filename=str(tmp_path / "dg.pvd"))
    solver = ScalarTransportDGSolver(s)
    P = solver.solve()
    # host pipeline: the restated system, a direct solve, the host L2 projection
    F, bcs_ = solver.generate_form(0, None, None, solver.w_current, solver.w_prev)
    fc, fl, fh, fg, src = solver.system_arrays(F)
    V = solver.function_space
    Ah, bh = dr.assemble(mesh, F.conductivity, F.capacity, F.velocity, F.alpha, facet_cell=fc, facet_local=fl, facet_h=fh,
                         facet_g=fg, source=src, key=V.plus_key())
    dofs, vals = solver._bc_arrays(bcs_)
    Ah, bh = dr.apply_dirichlet(Ah, bh, dofs, vals)
    Th = spsolve(Ah.tocsc(), bh)
    T = solver.w_current.vector().get_local()
    assert np.abs(T - Th).max() <= 1e-9 * np.abs(Th).max()
    Ph = dr.cg1_projection(mesh, Th)
    assert np.abs(P.vector().get_local() - Ph).max() <= 1e-9 * np.abs(Ph).max()
    st = solver.last_solve_stats
    print("advection-dominated: %d iterations, %.3f ms per product" % (st["iterations"], st["spmv_ms"]))
    solver.save(str(tmp_path / "dg.pvd"))
    vtu = list(tmp_path.glob("dg*.vtu"))
    assert vtu and os.path.getsize(vtu[0]) > 0


def test_full_size_box_reproduces_the_exact_linear_state():
    """BoxMesh of 1.5 M cells (6.1 M DOF): the exact linear state to 1e-9, advection-dominated (kappa = 1e-4, |beta| ~ 1.1).
    With kappa = 0.01 the solve meets its test (true residual 9e-14) and the state is off by 2.3e-8: that operator's condition
    number, not the stopping test, bounds the error there."""
    from fenicssolver_amd.fem import BoxMesh, Point
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    n = (64, 64, 62)
    mesh = BoxMesh(Point(0.0, 0.0, 0.0), Point(1.0, 1.0, 1.0), *n)
    assert mesh.num_cells() >= 1500000
    s, a, t0 = _case(mesh, 3, kappa=1e-4, beta=[1.0, 0.5, 0.25])
    solver = ScalarTransportDGSolver(s)
    t = time.perf_counter()
    P = solver.solve()
    wall = time.perf_counter() - t
    st = solver.last_solve_stats
    Tstar = solver.function_space.node_coordinates() @ a + t0
    T = solver.w_current.vector().get_local()
    print("full size: %d DOF, %d iterations, %.3f ms per iteration (solve %.0f ms), %.1f s wall, true residual %.2e" % (
        len(T), st["iterations"], st["solve_ms"] / max(st["iterations"], 1), st["solve_ms"], wall, st["true_rel_residual"]))
    assert st["converged"] == 1 and st["true_rel_residual"] <= 1e-12
    assert np.abs(T - Tstar).max() <= 1e-9 * np.abs(Tstar).max()
    Pstar = mesh.coordinates() @ a + t0
    assert np.abs(P.vector().get_local() - Pstar).max() <= 1e-9 * np.abs(Pstar).max()


def test_varying_flux_and_htc_ambient_end_to_end():
    """Expression-valued flux and HTC ambient temperature: the solver's DG solution against a host system whose facet lists and
    vertex values are built here from the mesh coordinates (not from the solver's arrays)."""
    from fenicssolver_amd.fem import UnitCubeMesh, AutoSubDomain, Expression, near
    from fenicssolver_amd.ScalarTransportDGSolver import ScalarTransportDGSolver
    mesh = UnitCubeMesh(6, 5, 4)
    beta = np.array([0.7, 0.2, -0.1])
    flux = lambda X: X[..., 0] + 2.0 * X[..., 1] * X[..., 2] + 0.5      # noqa: E731
    amb = lambda X: 1.0 + X[..., 0] * X[..., 2]                           # noqa: E731
    bcs = {"inlet": {"boundary_id": 1, "type": "Dirichlet", "value": 1.0,
                     "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary and near(x[0], 0.0))},
           "heated": {"boundary_id": 2, "type": "heat_flux", "value": Expression("x[0] + 2*x[1]*x[2] + 0.5", degree=1),
                      "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary and near(x[1], 0.0))},
           "cooled": {"boundary_id": 3, "type": "HTC", "value": 3.0, "ambient": "1 + x[0]*x[2]",
                      "boundary": AutoSubDomain(lambda x, on_boundary: on_boundary and near(x[1], 1.0))}}
    s, _, _ = _case(mesh, 3, kappa=0.05, beta=beta, bcs=bcs, source=False)
    solver = ScalarTransportDGSolver(s)
    solver.solve()
    T = solver.w_current.vector().get_local()
    c = 2.0 * 1.5
    k = 0.05 * c
    # host system from the mesh alone
    co, cells = mesh.coordinates(), mesh.cells().astype(np.int64)
    nc, nl = cells.shape
    cf = mesh.cell_facets().astype(np.int64)
    fc, fl = np.nonzero(mesh.exterior_facets()[cf])
    X = co[cells[fc]]                                                         # [n, 4, 3] the cells behind the boundary facets
    on = np.arange(nl)[None, :] != fl[:, None]
    fx = np.stack([X[i][on[i]] for i in range(len(fc))])                      # the facets' vertices
    at_y0 = np.all(np.abs(fx[..., 1]) < 1e-12, axis=1)
    at_y1 = np.all(np.abs(fx[..., 1] - 1.0) < 1e-12, axis=1)
    at_x0 = np.all(np.abs(fx[..., 0]) < 1e-12, axis=1)
    sel = at_y0 | at_y1
    h = np.where(at_y1, 3.0 / c, 0.0)[sel]
    g = np.where(at_y0[:, None], flux(X) / c, (3.0 / c) * amb(X))[sel]
    Ah, bh = dr.assemble(mesh, k, c, beta, 500.0, facet_cell=fc[sel], facet_local=fl[sel], facet_h=h, facet_g=g,
                         key=-np.arange(nc))
    inlet_verts = np.unique(fx[at_x0].reshape(-1, 3) @ np.array([1e6, 1e3, 1.0]))
    vkey = co @ np.array([1e6, 1e3, 1.0])
    on_inlet = np.isin(np.round(vkey, 6), np.round(inlet_verts, 6))
    dofs = np.nonzero(on_inlet[cells.ravel()])[0]
    Ah, bh = dr.apply_dirichlet(Ah, bh, dofs, np.ones(len(dofs)))
    Th = spsolve(Ah.tocsc(), bh)
    assert np.abs(T - Th).max() <= 1e-9 * np.abs(Th).max()
