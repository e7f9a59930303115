"""Isotropic elasticity with E, nu (and alpha) varying from cell to cell: FS_COEF_CELL_LAME through fs_assemble_matrix, the
per-cell von Mises load (fs_assemble_von_mises_cells), the per-cell thermal load and LinearElasticitySolver with per-region
materials - on one GPU and on several ranks sharing it (tests/materials_gpu_worker.py).  References: the oracle's element
matrices evaluated once per material, picked cell by cell by region."""
import copy
import os
import subprocess
import sys
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E1, NU1, E2, NU2 = 2e11, 0.27, 1e10, 0.35          # E ratio 20, different nu


def _csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


def _pairs(region):
    """(mu, lambda) per cell: material 1 where region is True, material 2 elsewhere."""
    m1, m2 = np.array(fo.lame(E1, NU1)), np.array(fo.lame(E2, NU2))
    return np.where(np.asarray(region)[:, None], m1[None, :], m2[None, :])


def _by_region(K1, K2, region):
    return np.where(np.asarray(region)[:, None, None], K1, K2)


def _vm_rhs(gpu, dV, dP, n_local, lame, seed=3):
    u = gpu.DeviceVector(n_local, np.random.default_rng(seed).standard_normal(n_local))
    b = gpu.DeviceVector(dP.n_owned)
    if isinstance(lame, tuple) and isinstance(lame[0], str):
        gpu.assemble_von_mises(dV, u, lame, None, dP, b)
    else:
        gpu.assemble_von_mises(dV, u, lame[0], lame[1], dP, b)
    return b.get()


def _meshes_3d(gpu, data_dir):
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(data_dir, "mesh.xml"))
    yield "file", gpu.DeviceMesh(co, ce), len(co), len(ce)
    nx, ny, nz = 5, 3, 4
    yield "box", gpu.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), (2.0, 1.0, 1.5)), (nx + 1) * (ny + 1) * (nz + 1), 6 * nx * ny * nz


# ---------------------------------------------------------------------------------------------- 1. uniform per-cell == constant
@pytest.mark.parametrize("degree", [1, 2])
def test_uniform_per_cell_material_gives_the_constant_operator_bit_for_bit(gpu, data_dir, degree):
    mu, lm = fo.lame(E1, NU1)
    for name, mesh, nv, nc in _meshes_3d(gpu, data_dir):
        V = gpu.DeviceSpace(mesh, 3, degree=degree)
        pairs = np.tile([mu, lm], (nc, 1))
        Ac, Ak = gpu.DeviceMatrix(V), gpu.DeviceMatrix(V)
        Ac.assemble(lame=(mu, lm))
        Ak.assemble(lame=("cell", pairs))
        vc, vk = Ac.to_csr()[2], Ak.to_csr()[2]
        assert np.array_equal(vc.view(np.uint64), vk.view(np.uint64)), name
        # the add form and a mass term on top
        Ac.assemble(lame=(mu, lm), mass=7800.0, add=True)
        Ak.assemble(lame=("cell", pairs), mass=7800.0, add=True)
        assert np.array_equal(Ac.to_csr()[2].view(np.uint64), Ak.to_csr()[2].view(np.uint64)), name
        P = gpu.DeviceSpace(mesh, 1)
        rc = _vm_rhs(gpu, V, P, V.n_local, (mu, lm))
        rk = _vm_rhs(gpu, V, P, V.n_local, ("cell", pairs))
        assert np.array_equal(rc.view(np.uint64), rk.view(np.uint64)), name


@pytest.mark.parametrize("degree", [1, 2])
def test_uniform_per_cell_material_on_triangles_bit_for_bit(gpu, degree):
    co, ce = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 9, 4)
    mu, lm = fo.lame(3.0e3, 0.3)
    mesh = gpu.DeviceMesh(co, ce)
    V = gpu.DeviceSpace(mesh, ncomp=2, degree=degree)
    pairs = np.tile([mu, lm], (len(ce), 1))
    Ac, Ak = gpu.DeviceMatrix(V), gpu.DeviceMatrix(V)
    Ac.assemble(lame=(mu, lm), mass=2.0)
    Ak.assemble(lame=("cell", pairs), mass=2.0)
    assert np.array_equal(Ac.to_csr()[2].view(np.uint64), Ak.to_csr()[2].view(np.uint64))
    P = gpu.DeviceSpace(mesh, 1)
    rc = _vm_rhs(gpu, V, P, V.n_local, (mu, lm))
    rk = _vm_rhs(gpu, V, P, V.n_local, ("cell", pairs))
    assert np.array_equal(rc.view(np.uint64), rk.view(np.uint64))


def test_per_cell_arrays_of_the_wrong_length_are_refused(gpu):
    co, ce = fo.box_mesh((0, 0, 0), (1.0, 1.0, 1.0), 2, 2, 2)
    mesh = gpu.DeviceMesh(co, ce)
    V = gpu.DeviceSpace(mesh, 3)
    A = gpu.DeviceMatrix(V)
    with pytest.raises(gpu.BackendError):
        A.assemble(lame=("cell", np.ones((len(ce) - 1, 2))))
    S = gpu.DeviceSpace(mesh, 1)
    with pytest.raises(gpu.BackendError):          # per-cell Lame pairs on a scalar space
        gpu.DeviceMatrix(S).assemble(lame=("cell", np.ones((len(ce), 2))))


# ---------------------------------------------------------------------------------------------- 2. two regions against the oracle
def _check_against(M, R):
    assert M.shape == R.shape
    assert np.array_equal(M.indptr, R.indptr) and np.array_equal(M.indices, R.indices)
    assert abs(M - R).max() <= 1e-12 * abs(R).max()


def test_two_region_p1_operator_matches_the_oracle(gpu, data_dir):
    for co, ce in (fo.read_dolfin_xml_mesh(os.path.join(data_dir, "mesh.xml")), fo.box_mesh((0, 0, 0), (2.0, 1.0, 1.0), 6, 3, 3)):
        cen = co[ce.astype(np.int64)].mean(axis=1)
        region = cen[:, 0] < 0.5 * (co[:, 0].min() + co[:, 0].max())
        assert region.any() and not region.all()
        Ke = _by_region(fo.p1_elasticity_local(co, ce, E1, NU1), fo.p1_elasticity_local(co, ce, E2, NU2), region)
        dofs = (ce.astype(np.int64)[:, :, None] * 3 + np.arange(3)).reshape(len(ce), 12)
        R = fo.assemble_generic(3 * len(co), dofs, Ke).tocsr()
        R.sort_indices()
        # uploaded in locality order: device vertex k = file vertex vo[k], device cell c = file cell cord[c]
        mesh, vo, cord = gpu.DeviceMesh.renumbered(co, ce)
        V = gpu.DeviceSpace(mesh, 3)
        A = gpu.DeviceMatrix(V)
        A.assemble(lame=("cell", _pairs(region)[cord]))
        p = (vo.astype(np.int64)[:, None] * 3 + np.arange(3)).ravel()
        Rp = R[p][:, p].tocsr()
        Rp.sort_indices()
        _check_against(_csr(A), Rp)


def test_two_region_p1_box_operator_matches_the_oracle_and_its_product(gpu):
    """A device-generated box (snapped geometry): the assembled values, and the product through the form the library selects
    (row dictionary / block rows check every row against its class and stream the rest)."""
    nx, ny, nz = 8, 5, 6
    mesh = gpu.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), (2.0, 1.0, 1.5))
    co, ce, _ = mesh.get()                  # the reference on the device's own vertices and cells
    cen = co[ce.astype(np.int64)].mean(axis=1)
    region = cen[:, 2] < 0.75
    Ke = _by_region(fo.p1_elasticity_local(co, ce, E1, NU1), fo.p1_elasticity_local(co, ce, E2, NU2), region)
    dofs = (ce.astype(np.int64)[:, :, None] * 3 + np.arange(3)).reshape(len(ce), 12)
    R = fo.assemble_generic(3 * len(co), dofs, Ke).tocsr()
    R.sort_indices()
    V = gpu.DeviceSpace(mesh, 3)
    A = gpu.DeviceMatrix(V)
    A.assemble(lame=("cell", _pairs(region)))
    _check_against(_csr(A), R)
    xv = np.random.default_rng(1).standard_normal(V.n_local)
    x, y = gpu.DeviceVector(V.n_local, xv), gpu.DeviceVector(V.n_owned)
    yr = R @ xv[:V.n_owned]
    for product in (A.spmv, A.spmv_dictionary):
        product(x, y)
        assert np.abs(y.get() - yr).max() <= 1e-12 * np.abs(yr).max()


def test_two_region_p2_operator_matches_the_oracle(gpu, data_dir):
    for co, ce in (fo.read_dolfin_xml_mesh(os.path.join(data_dir, "mesh.xml")), fo.box_mesh((0, 0, 0), (2.0, 1.0, 1.0), 4, 2, 2)):
        cen = co[ce.astype(np.int64)].mean(axis=1)
        region = cen[:, 1] < 0.5 * (co[:, 1].min() + co[:, 1].max())
        mesh = gpu.DeviceMesh(co, ce)
        V = gpu.DeviceSpace(mesh, 3, degree=2)
        cd, edges = fo.p2_cell_dofs(len(co), ce)
        assert np.array_equal(V.edges(), edges)
        Ke = _by_region(fo.p2_elasticity_local(co, ce, E1, NU1), fo.p2_elasticity_local(co, ce, E2, NU2), region)
        R = fo.assemble_generic(3 * (len(co) + len(edges)), fo.p2_vector_cell_dofs(cd), Ke).tocsr()
        R.sort_indices()
        A = gpu.DeviceMatrix(V)
        A.assemble(lame=("cell", _pairs(region)))
        _check_against(_csr(A), R)


def test_two_region_triangle_operator_matches_the_oracle(gpu):
    co, ce = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 9, 4)
    cen = co[ce.astype(np.int64)].mean(axis=1)
    region = cen[:, 0] < 1.0
    Ke = _by_region(fo.tri_elasticity_local(co, ce, E1, NU1), fo.tri_elasticity_local(co, ce, E2, NU2), region)
    R = fo.assemble_generic(2 * len(co), fo.tri_vector_cell_dofs(ce), Ke).tocsr()
    R.sort_indices()
    mesh = gpu.DeviceMesh(co, ce)
    V = gpu.DeviceSpace(mesh, ncomp=2)
    A = gpu.DeviceMatrix(V)
    A.assemble(lame=("cell", _pairs(region)))
    _check_against(_csr(A), R)


# ---------------------------------------------------------------------------------------------- solver cases
def _bar_solver(nz=8, degree=1, dim=3, material=None, bcs=None, **extra):
    """The bar [0,1]^2 x [0,2] (3-D, along z) / [0,2] x [0,1] (2-D, along x) in two regions: subdomain 1 before the mesh plane
    at 3/4 of its length, subdomain 2 after."""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, MeshFunction, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    L, ax = 2.0, (2 if dim == 3 else 0)
    if dim == 3:
        mesh = BoxMesh(Point(0, 0, 0), Point(1, 1, L), 2, 2, nz)
    else:
        mesh = RectangleMesh(Point(0, 0), Point(L, 1), nz, 2)
    if bcs is None:
        bcs = OrderedDict()
        bcs["clamp"] = {'boundary': AutoSubDomain(lambda x: near(x[ax], 0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0,) * dim)}
        bcs["pull"] = {'boundary': AutoSubDomain(lambda x: near(x[ax], L)), 'boundary_id': 2, 'type': 'stress',
                       'value': Constant(tuple(0.0 if i != ax else 3e7 for i in range(dim)))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = material or {'name': 'bimaterial', 'density': 7800, 'thermal_expansion_coefficient': 1.2e-5,
                                 'elastic_modulus': {'low': {'subdomain_id': 1, 'value': E1}, 'high': {'subdomain_id': 2, 'value': E2}},
                                 'poisson_ratio': {'low': {'subdomain_id': 1, 'value': 0.0}, 'high': {'subdomain_id': 2, 'value': 0.0}}}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", degree)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    s['report_settings'] = dict(QUIET)
    s.update(extra)
    solver = LinearElasticitySolver(s)
    solver.reference_load_sign = False
    co, ce = mesh.coordinates(), mesh.cells()
    sub = MeshFunction("size_t", mesh, dim)
    sub.array()[:] = np.where(co[ce.astype(np.int64)].mean(axis=1)[:, ax] < 0.75 * L, 1, 2)
    solver.subdomains = sub
    return solver


@pytest.mark.parametrize("dim,degree", [(3, 1), (3, 2), (2, 1), (2, 2)])
def test_bimaterial_bar_is_exact(gpu, dim, degree):
    """nu = 0, clamp at 0, traction T at L: u along the bar is piecewise linear, u(L) = T (L1/E1 + L2/E2); the von Mises stress
    is |T| everywhere (2-D: the reference's deviator keeps the 1/3 of three dimensions, sqrt(5/6) |T|)."""
    T, L1, L2 = 3e7, 1.5, 0.5
    solver = _bar_solver(degree=degree, dim=dim)
    u = solver.solve()
    ax = 2 if dim == 3 else 0
    X = solver.function_space.node_coordinates()
    z = X[:, ax]
    exact = np.where(z < L1, T * z / E1, T * (L1 / E1 + (z - L1) / E2))
    U = u.node_values()
    assert np.abs(U[:, ax] - exact).max() <= 1e-8 * exact.max()
    assert np.abs(np.delete(U, ax, axis=1)).max() <= 1e-8 * exact.max()
    if dim == 3 and degree == 1:
        assert solver.last_solve_stats.get('amg_levels', 0) >= 1                 # solve_amg with the AMG preconditioner
    vm = solver.von_Mises(u).vector().get_local()
    expect = T if dim == 3 else np.sqrt(5.0 / 6.0) * T
    assert np.abs(vm - expect).max() <= 1e-8 * expect


@pytest.mark.parametrize("degree", [1, 2])
def test_thermal_expansion_of_two_materials_is_stress_free(gpu, degree):
    """Uniform alpha and dT, regions that differ in E and nu, rollers on x = 0, y = 0, z = 0: u = alpha dT x, which holds only if
    the per-cell thermal factor E alpha / (1 - 2 nu) matches the per-cell stiffness."""
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    def plane(i):
        return AutoSubDomain(lambda x: near(x[i], 0))

    bcs = OrderedDict()
    for i, name in enumerate("xyz"):
        val = [None, None, None]
        val[i] = Constant(0.0)
        bcs["roller_" + name] = {'boundary': plane(i), 'boundary_id': i + 1, 'type': 'Dirichlet', 'value': tuple(val)}
    material = {'name': 'two', 'density': 7800, 'thermal_expansion_coefficient': 1.2e-5,
                'elastic_modulus': {'a': {'subdomain_id': 1, 'value': E1}, 'b': {'subdomain_id': 2, 'value': E2}},
                'poisson_ratio': {'a': {'subdomain_id': 1, 'value': NU1}, 'b': {'subdomain_id': 2, 'value': NU2}}}
    solver = _bar_solver(nz=6, degree=degree, material=material, bcs=bcs, temperature_distribution=343.0)
    u = solver.solve()
    X = solver.function_space.node_coordinates()
    exact = 1.2e-5 * 50.0 * X
    assert np.abs(u.node_values() - exact).max() <= 1e-9 * np.abs(exact).max()


def _cantilever(n=(24, 4, 4), contrast=100.0, preconditioner=None, E=None, rtol=1e-11):
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, MeshFunction, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(10, 1, 1), *n)
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0, 0, 0))}
    bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 10)), 'boundary_id': 2, 'type': 'stress', 'value': Constant((0, 0, -1e6))}
    s = copy.deepcopy(SB.default_case_settings)
    E = E or (2e11, 2e11 / contrast)
    s['material'] = {'name': 'two', 'density': 7800, 'thermal_expansion_coefficient': 1.2e-5,
                     'elastic_modulus': {'stiff': {'subdomain_id': 1, 'value': E[0]}, 'soft': {'subdomain_id': 2, 'value': E[1]}},
                     'poisson_ratio': {'stiff': {'subdomain_id': 1, 'value': 0.27}, 'soft': {'subdomain_id': 2, 'value': 0.33}}}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    # (stopping test on the unpreconditioned residual: what 'true residual <= 10 rtol' asks of the contrast case)
    sp_ = {'krylov_relative_tolerance': rtol, 'maximum_iterations': 200000, 'norm_type': 'unpreconditioned'}
    if preconditioner:
        sp_['preconditioner'] = preconditioner
    s['solver_settings']['solver_parameters'] = sp_
    s['report_settings'] = dict(QUIET)
    solver = LinearElasticitySolver(s)
    co, ce = mesh.coordinates(), mesh.cells()
    sub = MeshFunction("size_t", mesh, 3)
    sub.array()[:] = np.where(co[ce.astype(np.int64)].mean(axis=1)[:, 0] < 5.0, 1, 2)
    solver.subdomains = sub
    return solver


@pytest.mark.parametrize("n,rtol", [((24, 4, 4), 1e-11), ((120, 64, 64), 1e-9)])
def test_contrast_100_with_amg_matches_jacobi_cg(gpu, n, rtol):
    """E ratio 100 across x = 5: solve_amg converges, its true residual is within 10 rtol, the field is Jacobi-CG's.  The second
    size has more than 1.5 M rows: the two-material operator also goes through the library's product-form selection (its true
    residual stops near 1e-9 in fp64: the tolerance there is 1e-9)."""
    amg = _cantilever(n, rtol=rtol)
    u = amg.solve().vector().get_local()
    st = amg.last_solve_stats
    assert st['converged'] == 1 and st['true_rel_residual'] <= 10 * rtol, st
    assert st.get('amg_levels', 0) >= 1
    if n[0] > 100:
        assert 3 * (n[0] + 1) * (n[1] + 1) * (n[2] + 1) > 1.5e6
    ref = _cantilever(n, preconditioner='jacobi', rtol=rtol).solve().vector().get_local()
    assert np.abs(u - ref).max() <= 1e-6 * np.abs(ref).max()


def test_material_changed_between_solves(gpu):
    """A solver whose material changes between solves does not reuse the old AMG hierarchy under the old key."""
    s1 = _cantilever()
    s1.solve()
    s1.material['elastic_modulus'] = {'stiff': {'subdomain_id': 1, 'value': 7e10}, 'soft': {'subdomain_id': 2, 'value': 3e9}}
    again = s1.solve().vector().get_local()
    assert s1.last_solve_stats.get('amg_reused') is False
    fresh = _cantilever(E=(7e10, 3e9)).solve().vector().get_local()
    assert np.abs(again - fresh).max() <= 1e-10 * np.abs(fresh).max()


# ---------------------------------------------------------------------------------------------- 7. several ranks
def _run(world, case, tmp_path):
    out = str(tmp_path / ("%s_%d.npz" % (case, world)))
    shim = os.path.join(ROOT, "tests", "shim", "libfakerccl.so")
    assert os.path.exists(shim), "build tests/shim first (make -C tests/shim; __graft_entry__.build() does it)"
    env = dict(os.environ, FS_RCCL_PATH=shim)
    port = 29800 + 10 * world + (os.getpid() % 97) * 20
    cmd = [sys.executable, "-m", "fenicssolver_amd.launch", "--nproc", str(world), "--devices", ",".join(["0"] * world),
           "--master-port", str(port), os.path.join(ROOT, "tests", "materials_gpu_worker.py"), out, case]
    p = subprocess.run(cmd, env=env, cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=600)
    assert p.returncode == 0, p.stdout.decode()[-3000:]
    return np.load(out)


@pytest.mark.parametrize("world", [2, 3])
def test_two_region_cantilever_on_several_ranks_equals_one_gpu(gpu, tmp_path, world):
    """The two-region P1 case on a replicated mesh: AMG with a distributed fine level and the replicated levels assembled from
    the GLOBAL per-cell array; the von Mises projection on the decomposed P1 space."""
    single = _cantilever(n=(36, 6, 6))
    u1 = single.solve()
    vm1 = single.von_Mises(u1).vector().get_local()
    r = _run(world, "cantilever", tmp_path)
    assert str(r["amg_decomposition"]) == "distributed"
    x1 = u1.vector().get_local()
    assert np.abs(r["x"] - x1).max() <= 1e-8 * np.abs(x1).max()
    assert np.abs(r["von_mises"] - vm1).max() <= 1e-8 * np.abs(vm1).max()
