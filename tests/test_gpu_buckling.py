"""Linear buckling on the GPU: the geometric stiffness (fs_assemble_geometric_stiffness) against the host reference, the fused
pencil product (fs_spmv_multi_pencil) against the block products it replaces, and fs_buckling_solve through
LinearElasticitySolver.solve_buckling against the dense pencil K_G phi = nu K phi built on the host from the device's own K and K_G
restricted to the free dofs."""
import copy
import os
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sp

import buckling_reference as br
from oracle import fem_oracle as fo
from spmv_reference import _poison, _vector_from_cache

pytestmark = pytest.mark.gpu
QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E, NU = 2e11, 0.3
TOL = 1e-8                       # the default tolerance of buckling_settings


def _csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ fixtures
def _fixtures(gpu, data_dir):
    """(name, coords [n, d], cells, DeviceSpace): the column, the unstructured mesh, plane strain, the box of 45 nodes."""
    for name, (nx, ny, nz), p1 in (("column", (10, 2, 2), (1.0, 0.1, 0.06)), ("odd box", (4, 2, 2), (2.0, 1.0, 1.0))):
        mesh = gpu.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), p1)
        xyz, cells, _ = mesh.get()
        yield name, xyz, cells, gpu.DeviceSpace(mesh, 3, 1)
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(data_dir, "mesh.xml"))
    yield "mesh.xml", co, ce, gpu.DeviceSpace(gpu.DeviceMesh(co, ce), 3, 1)
    co2, ce2 = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 9, 4)
    yield "plane strain", co2, ce2, gpu.DeviceSpace(gpu.DeviceMesh(co2, ce2), 2, 1)


def _smooth_u(co):
    d = co.shape[1]
    x, y = co[:, 0], co[:, 1]
    z = co[:, 2] if d == 3 else 0.3 * x
    u = np.stack([np.sin(x + 2.0 * y) + z, np.cos(y - z) * x, x * y + z * z][:d], axis=1)
    return 1e-3 * u.ravel()


# ------------------------------------------------------------------------------------------------ 1. assembly against the host
@pytest.mark.parametrize("material", ["constant", "per cell"])
def test_geometric_stiffness_matches_the_host_reference(gpu, data_dir, material):
    mu0, lm0 = fo.lame(E, NU)
    for name, co, ce, V in _fixtures(gpu, data_dir):
        d = co.shape[1]
        nc = len(ce)
        if material == "constant":
            mu, lm, spec = mu0, lm0, (mu0, lm0)
        else:
            mu = mu0 * (1.0 + 0.5 * np.sin(np.arange(nc)))
            lm = lm0 * (1.0 + 0.3 * np.cos(0.7 * np.arange(nc)))
            spec = ("cell", np.stack([mu, lm], axis=1))
        uh = _smooth_u(co)
        u = gpu.DeviceVector(V.n_local, uh)
        KG = gpu.DeviceMatrix(V)
        sig = KG.assemble_geometric(spec, u, cell_stress=True)
        rp, ci, va, shape = KG.to_csr()
        _, rec = br.cell_stress(co, ce, uh, mu, lm)
        ref = br.geometric_stiffness_csr(co, ce, uh, mu, lm)
        assert shape == ref.shape, name
        assert np.array_equal(rp, ref.indptr) and np.array_equal(ci, ref.indices), (name, "pattern")
        scale = np.abs(ref.data).max()
        assert scale > 0.0
        err = np.abs(va - ref.data).max()
        print("%s / %s: max|K_G - ref| / max|K_G| = %.3e" % (name, material, err / scale))
        assert err <= 1e-12 * scale, (name, err / scale)
        rows = np.repeat(np.arange(shape[0]), np.diff(rp))
        assert np.all(va[(rows % d) != (ci % d)] == 0.0), (name, "off-diagonal block entries")
        assert sig.shape == rec.shape
        serr = np.abs(sig - rec).max() / np.abs(rec).max()
        print("%s / %s: max|sigma - ref| / max|sigma| = %.3e" % (name, material, serr))
        assert serr <= 1e-12, (name, serr)
        KG2 = gpu.DeviceMatrix(V)
        sig2 = KG2.assemble_geometric(spec, u, cell_stress=True)
        assert np.array_equal(_bits(KG2.to_csr()[2]), _bits(va)) and np.array_equal(_bits(sig2), _bits(sig)), (name, "bits")
        assert KG.assemble_geometric(spec, u) is None


def test_geometric_stiffness_is_an_ordinary_matrix(gpu, data_dir):
    """spmv and apply_dirichlet take K_G as they take any matrix of the space; the pencil product refuses it once a Dirichlet row
    has made a block something else than s I."""
    mu, lm = fo.lame(E, NU)
    name, co, ce, V = next(_fixtures(gpu, data_dir))
    uh = _smooth_u(co)
    KG = gpu.DeviceMatrix(V)
    KG.assemble_geometric((mu, lm), gpu.DeviceVector(V.n_local, uh))
    rng = np.random.default_rng(3)
    xv = rng.standard_normal(V.n_local)
    y = gpu.DeviceVector(V.n_owned)
    KG.spmv(gpu.DeviceVector(V.n_local, xv), y)
    ref = br.geometric_stiffness_csr(co, ce, uh, mu, lm)
    assert np.abs(y.get() - ref @ xv).max() <= 1e-12 * (abs(ref) @ np.abs(xv)).max()
    K = gpu.DeviceMatrix(V)
    K.assemble(lame=(mu, lm))
    KG.apply_dirichlet(None, np.array([4], dtype=np.int32), np.zeros(1), symmetric=True)
    X = [gpu.DeviceVector(V.n_local, xv)]
    with pytest.raises(gpu.BackendError, match="multiple of the identity"):
        gpu.spmv_multi_pencil(K, KG, X, [gpu.DeviceVector(V.n_owned)], [gpu.DeviceVector(V.n_owned)])


# ------------------------------------------------------------------------------------------------ 2. fused product
@pytest.mark.parametrize("m", [1, 3, 8, 13])
def test_pencil_product_equals_the_two_block_products(gpu, data_dir, m):
    """Y_K bit for bit; Y_G as numbers (np.array_equal: the block product of K_G adds exact zeros, which can turn a -0 into +0).
    X comes out of a block cache that held NaN, so the entry behind the end of every column is a NaN."""
    mu, lm = fo.lame(E, NU)
    rng = np.random.default_rng(m)
    for name, co, ce, V in _fixtures(gpu, data_dir):
        K, KG = gpu.DeviceMatrix(V), gpu.DeviceMatrix(V)
        K.assemble(lame=(mu, lm))
        KG.assemble_geometric((mu, lm), gpu.DeviceVector(V.n_local, _smooth_u(co)))
        _poison(gpu, (V.n_local + 1, V.n_local + 2), "nan", seed=m)
        X = []
        for _ in range(m):
            x = _vector_from_cache(gpu, V.n_local)
            x.set(rng.standard_normal(V.n_local))
            X.append(x)
        YK, YG, RK, RG = ([gpu.DeviceVector(V.n_owned) for _ in range(m)] for _ in range(4))
        gpu.spmv_multi_pencil(K, KG, X, YK, YG)
        gpu.spmv_multi(K, X, RK)
        gpu.spmv_multi(KG, X, RG)
        for j in range(m):
            yk, yg = YK[j].get(), YG[j].get()
            assert np.all(np.isfinite(yk)) and np.all(np.isfinite(yg)), (name, j)
            assert np.array_equal(_bits(yk), _bits(RK[j].get())), (name, j, "K half")
            assert np.array_equal(yg, RG[j].get()), (name, j, "K_G half")
            assert np.abs(yg).max() > 0.0
        for x in X:
            x.close()


def test_pencil_benchmark_and_the_two_pass_driver(gpu, data_dir):
    """The timing entry point runs both forms, and fs_buckling_solve with two block products (two_pass) finds the factors of the
    fused form: the K halves agree bit for bit, the K_G halves as numbers, so at most the sign of a zero differs on the way."""
    mu, lm = fo.lame(E, NU)
    name, co, ce, V = next(_fixtures(gpu, data_dir))
    K, KG = gpu.DeviceMatrix(V), gpu.DeviceMatrix(V)
    K.assemble(lame=(mu, lm))
    u = np.zeros_like(co)
    u[:, 0] = -1e-3 * co[:, 0]                                            # uniform compression along the column
    KG.assemble_geometric((mu, lm), gpu.DeviceVector(V.n_local, u.ravel()))
    fused_ms, two_pass_ms = gpu.spmv_multi_pencil_benchmark(K, KG, m=8, reps=2)
    assert fused_ms > 0.0 and two_pass_ms > 0.0
    cons = np.flatnonzero(np.repeat(co[:, 0] == 0.0, 3)).astype(np.int32)
    K.apply_dirichlet(None, cons, np.zeros(cons.size), symmetric=True)
    amg = gpu.AMG(K, nullspace="rigid_body", coarse_size=36)
    a, _, sa = gpu.buckling_solve(K, KG, 3, amg=amg, constrained=cons)
    b, _, sb = gpu.buckling_solve(K, KG, 3, amg=amg, constrained=cons, two_pass=True)
    amg.close()
    assert sa['n_converged'] == sb['n_converged'] == 3 and sa['iterations'] == sb['iterations']
    assert np.all(np.abs(a - b) <= 1e-12 * a), (a, b)


# ------------------------------------------------------------------------------------------------ the solver class
def _near_faces(axis, lo, hi):
    from fenicssolver_amd.fem import AutoSubDomain, near
    return AutoSubDomain(lambda x: near(x[axis], lo) or near(x[axis], hi))


def _solver(load=None, far=None, rollers=False, modulus=E, buckling=None, dim=3, p1=(1.0, 0.1, 0.06), n=(10, 2, 2)):
    """The column clamped at x = 0.  load: pressure on the far face (> 0 compresses); far: prescribed u_x of the far face, all its
    other components held; rollers: u_y = 0 on the y faces and u_z = 0 on the z faces."""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    L = p1[0]
    mesh = BoxMesh(Point(0, 0, 0), Point(*p1), *n) if dim == 3 else RectangleMesh(Point(0.0, 0.0), Point(*p1[:2]), *n[:2])
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'value': Constant((0.0,) * dim)}
    if load is not None:
        bcs["end"] = {'boundary': AutoSubDomain(lambda x: near(x[0], L)), 'boundary_id': 2, 'type': 'pressure', 'value': load}
    if far is not None:
        bcs["end"] = {'boundary': AutoSubDomain(lambda x: near(x[0], L)), 'boundary_id': 2, 'type': 'Dirichlet',
                      'value': Constant((far,) + (0.0,) * (dim - 1))}
    if rollers:
        bcs["y"] = {'boundary': _near_faces(1, 0.0, p1[1]), 'boundary_id': 3, 'type': 'Dirichlet', 'value': (None, Constant(0.0), None)}
        bcs["z"] = {'boundary': _near_faces(2, 0.0, p1[2]), 'boundary_id': 4, 'type': 'Dirichlet', 'value': (None, None, Constant(0.0))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': modulus, 'poisson_ratio': NU, 'density': 7800.0, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['buckling_settings'] = dict(buckling or {})
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = None
    return LinearElasticitySolver(s)


def _host_pencil(gpu, solver):
    """K and K_G - assembled by the device from the device's own static displacement - on the host, restricted to the free dofs,
    and the dense pencil on them."""
    F, bcs = solver.generate_form(0, None, None, solver.w_current, solver.w_prev)
    V = F.space.device()
    K = gpu.DeviceMatrix(V)
    K.assemble(lame=F.lame_spec())
    KG = solver.geometric_stiffness(solver.w_current)
    cons = np.unique(solver._bc_arrays(bcs)[0])
    free = np.setdiff1d(np.arange(V.n_owned), cons)
    Kf = _csr(K)[free][:, free].toarray()
    Gf = _csr(KG)[free][:, free].toarray()
    nu, phi = br.dense_pencil(Gf, Kf)
    return Kf, Gf, free, cons, nu, phi


def _check_against_dense(gpu, solver, nm, tol=TOL):
    Kf, Gf, free, cons, nu, _ = _host_pencil(gpu, solver)
    # preconditions of the case, not properties of the code under test
    assert np.sum(nu < 0.0) >= nm, ("the dense pencil has too few negative nu", nu[:nm + 2])
    lam_ref = -1.0 / nu[:nm]
    lam = solver.buckling_factors
    assert lam.shape == (nm,) and np.all(lam > 0.0) and np.all(np.diff(lam) >= 0.0), lam
    # B-norm eigenvalue bound for a 2-norm residual of tol, with a factor 10 for the recomputed products
    bound = 10.0 * tol * np.sqrt(np.linalg.cond(Kf))
    rel = np.abs(lam - lam_ref) / lam_ref
    print("factors", lam, "dense", lam_ref, "rel. error", rel, "bound", bound, "stats", solver.buckling_stats)
    assert np.all(rel <= bound), (lam, lam_ref, bound)
    Phi = np.stack([f.vector().get_local() for f in solver.buckling_modes], axis=1)
    assert np.all(Phi[cons] == 0.0)
    assert np.all(np.abs(Phi).max(axis=0) == 1.0)
    P = Phi[free]
    for j in range(nm):
        kx = Kf @ P[:, j]
        r = Gf @ P[:, j] + kx / lam[j]                      # K_G x - nu K x with nu = -1 / lambda
        assert np.linalg.norm(r) <= 1e-8 / lam[j] * np.linalg.norm(kx), (j, np.linalg.norm(r) * lam[j] / np.linalg.norm(kx))
    G = P.T @ (Kf @ P)
    dg = np.sqrt(np.diag(G))
    C = G / np.outer(dg, dg)
    assert np.abs(C - np.eye(nm)).max() <= 1e-8, np.abs(C - np.eye(nm)).max()
    return lam_ref


PRESSURE = 1e6


def test_column_under_a_compressive_end_load(gpu):
    solver = _solver(load=PRESSURE)
    mode = solver.solve_buckling()
    assert mode is solver.buckling_modes[0] and len(solver.buckling_modes) == 4
    st = solver.buckling_stats
    assert st['n_converged'] == 4 and st['n_negative'] >= 4 and st['max_rel_residual'] <= TOL
    lam_ref = _check_against_dense(gpu, solver, 4)
    assert lam_ref[1] > 1.01 * lam_ref[0], lam_ref                       # precondition: the rectangular section keeps them apart
    # the static displacement is where solve() leaves it, and the prestress is its stress: compression along x
    u0 = solver.w_current.vector().get_local()
    assert solver.result is solver.w_current and np.abs(u0).max() > 0.0
    co, ce = solver.mesh.coordinates(), solver.mesh.cells()
    mu, lm = fo.lame(E, NU)
    _, rec = br.cell_stress(co, ce, u0, mu, lm)
    assert solver.prestress.shape == rec.shape == (len(ce), 6)
    assert np.abs(solver.prestress - rec).max() <= 1e-12 * np.abs(rec).max()
    assert np.all(rec[:, 0] < 0.0)
    # Euler's load of the clamped-free column about its weak axis, as an order of magnitude: P1 tetrahedra in bending lock
    b, h, L = 0.1, 0.06, 1.0
    euler = np.pi ** 2 * E * (b * h ** 3 / 12.0) / (4.0 * L ** 2) / (PRESSURE * b * h)
    assert euler <= solver.buckling_factors[0] <= 30.0 * euler, (solver.buckling_factors, euler)


def test_exact_scalings_of_the_factors(gpu):
    base = _solver(load=PRESSURE)
    base.solve_buckling()
    twice_load = _solver(load=2.0 * PRESSURE)
    twice_load.solve_buckling()
    twice_modulus = _solver(load=PRESSURE, modulus=2.0 * E)
    twice_modulus.solve_buckling()
    f = base.buckling_factors
    print(f, twice_load.buckling_factors, twice_modulus.buckling_factors)
    assert np.all(np.abs(2.0 * twice_load.buckling_factors - f) <= 1e-6 * f)
    assert np.all(np.abs(0.5 * twice_modulus.buckling_factors - f) <= 1e-6 * f)


def test_displacement_controlled_compression(gpu):
    solver = _solver(far=-1e-4)
    solver.solve_buckling()
    _check_against_dense(gpu, solver, 4)
    x = solver.mesh.coordinates()[:, 0]
    Phi = np.stack([f.vector().get_local() for f in solver.buckling_modes], axis=1).reshape(len(x), 3, 4)
    assert np.all(Phi[(x == 0.0) | (x == 1.0)] == 0.0)


def test_plane_strain_with_the_jacobi_preconditioner(gpu):
    """bs = 2, no V-cycle: diag(K)^-1.  max_iterations stays at its default of 500: Jacobi needs 127 iterations here."""
    solver = _solver(load=PRESSURE, dim=2, p1=(2.0, 0.5), n=(9, 4))
    solver.solve_buckling()
    print("plane strain iterations", solver.buckling_stats['iterations'])
    _check_against_dense(gpu, solver, 4)
    assert solver.prestress.shape == (solver.mesh.num_cells(), 4)


def test_nothing_buckles_under_tension(gpu):
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver(far=+1e-4, rollers=True)
    solver.solve()
    nu = _host_pencil(gpu, solver)[4]
    assert nu[0] > 0.0, nu[:4]                                           # precondition: the dense pencil has no negative nu
    with pytest.raises(SolverError, match="only 0 buckling mode"):
        solver.solve_buckling()


def test_identical_calls_give_identical_factor_bits(gpu):
    solver = _solver(load=PRESSURE)
    solver.solve_buckling()
    a = solver.buckling_factors.copy()
    solver.solve_buckling()
    assert np.array_equal(_bits(a), _bits(solver.buckling_factors))
    other = _solver(load=PRESSURE)
    other.solve_buckling()
    assert np.array_equal(_bits(a), _bits(other.buckling_factors))
