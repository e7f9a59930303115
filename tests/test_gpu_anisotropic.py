"""Anisotropic linear elasticity on the GPU: fs_assemble_anisotropic, fs_anisotropic_stress and fs_assemble_anisotropic_load against
the dense numpy reference (tests/anisotropic_reference.py, which rotates the rank-4 tensor where the kernels rotate the gradients),
and LinearElasticitySolver with 'elasticity_tensor' / 'orthotropic' / 'material_orientation' against exact solutions.

Operator comparisons: identical CSR structure and <= 1e-12 max|ref|, the bound of tests/test_gpu_elasticity_materials.py."""
import copy
import os
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import anisotropic_reference as ar
from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu
QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E_ISO, NU_ISO = 2e11, 0.27
CFRP_V = ar.orthotropic_voigt(ar.CFRP['elastic_moduli'], ar.CFRP['poisson_ratios'], ar.CFRP['shear_moduli'])
CFRP_S = ar.compliance_voigt(ar.CFRP['elastic_moduli'], ar.CFRP['poisson_ratios'], ar.CFRP['shear_moduli'])
# three regions with different D (library order): the CFRP, a glass-fibre-like orthotropic material, an isotropic resin
GFRP_V = ar.orthotropic_voigt([40e9, 12e9, 9e9], [0.28, 0.3, 0.42], [4e9, 3.5e9, 3.2e9])
TABLE3 = np.stack([ar.to_library(CFRP_V), ar.to_library(GFRP_V), ar.to_library(ar.isotropic_voigt(3.5e9, 0.35))])
TABLE3 = 0.5 * (TABLE3 + np.transpose(TABLE3, (0, 2, 1)))


def _csr(A):
    rp, ci, va, shape = A.to_csr()
    M = sp.csr_matrix((va, ci, rp), shape=shape)
    M.sort_indices()
    return M


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _check_against(M, R):
    assert M.shape == R.shape
    assert np.array_equal(M.indptr, R.indptr) and np.array_equal(M.indices, R.indices)
    err, scale = abs(M - R).max(), abs(R).max()
    print("operator error / max|ref| = %.3e" % (err / scale))
    assert err <= 1e-12 * scale


def _meshes(gpu, data_dir):
    """(name, DeviceMesh, coordinates, cells, dimension): the unstructured file mesh, a device box, a rectangle of triangles - with
    corner, edge and interior rows whose source counts are not multiples of the prefetch group of four."""
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(data_dir, "mesh.xml"))
    yield "file", gpu.DeviceMesh(co, ce), co, ce, 3
    box = gpu.DeviceMesh.box(5, 3, 4, (0.0, 0.0, 0.0), (2.0, 1.0, 1.5))
    cb, eb, _ = box.get()
    yield "box", box, cb, eb, 3
    c2, e2 = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 9, 4)
    yield "triangles", gpu.DeviceMesh(c2, e2), c2, e2, 2


def _three_regions(co, ce, d):
    cen = co[ce.astype(np.int64)][:, :d + 1].mean(axis=1)
    x = (cen[:, 0] - co[:, 0].min()) / (co[:, 0].max() - co[:, 0].min())
    idx = np.minimum((3 * x).astype(np.int32), 2)
    assert len(np.unique(idx)) == 3
    return idx


def _space(gpu, mesh, d):
    return gpu.DeviceSpace(mesh, 3) if d == 3 else gpu.DeviceSpace(mesh, ncomp=2)


def _reference_operator(co, ce, d, Dg, rho=None):
    Ke = ar.local_stiffness(co, ce, Dg)
    if rho is not None:
        Ke = Ke + ar.local_mass(co, ce, rho)
    return ar.assemble(len(co), ce, Ke, d)


# ---------------------------------------------------------------------------------------------- 1. isotropic D == the Lame operator
def test_isotropic_tensor_gives_the_lame_operator(gpu, data_dir):
    mu, lm = fo.lame(E_ISO, NU_ISO)
    D = ar.to_library(ar.isotropic_voigt(E_ISO, NU_ISO))
    for name, mesh, co, ce, d in _meshes(gpu, data_dir):
        V = _space(gpu, mesh, d)
        Aa, Ai = gpu.DeviceMatrix(V), gpu.DeviceMatrix(V)
        Aa.assemble_anisotropic((D[None], None, None))
        Ai.assemble(lame=(mu, lm))
        print(name, end=" ")
        _check_against(_csr(Aa), _csr(Ai))
        # a mass term, and on top of what is there (add=True): K + (K + rho M)
        rho = np.linspace(1000.0, 8000.0, len(ce))
        Aa.assemble_anisotropic((D[None], None, None), mass=('cell', rho), add=True)
        Ai.assemble(lame=(mu, lm), mass=('cell', rho), add=True)
        _check_against(_csr(Aa), _csr(Ai))
        Aa.assemble_anisotropic((D[None], None, None), mass=7800.0)
        Ai.assemble(lame=(mu, lm), mass=7800.0)
        _check_against(_csr(Aa), _csr(Ai))


# ---------------------------------------------------------------------------------------------- 2. regions and per-cell frames
@pytest.fixture(scope="module")
def region_cases(gpu, data_dir):
    """Per mesh: three regions with different D and per-cell random frames (about z in plane strain), the device matrix of the
    state and the numpy reference's per-cell global D - computed once, left unchanged."""
    out = {}
    for k, (name, mesh, co, ce, d) in enumerate(_meshes(gpu, data_dir)):
        idx = _three_regions(co, ce, d)
        R = ar.random_rotations(len(ce), 20 + k, about_z=(d == 2))
        V = _space(gpu, mesh, d)
        out[name] = dict(mesh=mesh, co=co, ce=ce, d=d, idx=idx, R=R, V=V, Dg=ar.global_D(TABLE3, idx, R, len(ce)))
    return out


@pytest.mark.parametrize("name", ["file", "box", "triangles"])
def test_three_regions_with_per_cell_frames_match_the_reference(gpu, region_cases, name):
    c = region_cases[name]
    A = gpu.DeviceMatrix(c['V'])
    A.assemble_anisotropic((TABLE3, c['idx'], c['R']))
    _check_against(_csr(A), _reference_operator(c['co'], c['ce'], c['d'], c['Dg']))
    # without frames, and with the consistent mass
    A.assemble_anisotropic((TABLE3, c['idx'], None), mass=1600.0)
    _check_against(_csr(A), _reference_operator(c['co'], c['ce'], c['d'], TABLE3[c['idx']], rho=1600.0))


# ---------------------------------------------------------------------------------------------- 3. the three ways to one material
@pytest.mark.parametrize("name", ["file", "box", "triangles"])
def test_index_forms_and_repeated_assemblies_give_the_same_bits(gpu, region_cases, name):
    c = region_cases[name]
    nc = len(c['ce'])
    D = TABLE3[:1]
    vals = []
    for material in ((D, None, c['R']), (D, np.zeros(nc, dtype=np.int32), c['R']), (np.repeat(D, nc, axis=0), None, c['R']),
                     (D, None, c['R']), gpu.AnisotropicMaterial(D[0], frames=c['R'].reshape(nc, 9))):
        A = gpu.DeviceMatrix(c['V'])
        A.assemble_anisotropic(material)
        vals.append(A.to_csr()[2])
    assert np.abs(vals[0]).max() > 0.0
    for v in vals[1:]:
        assert np.array_equal(_bits(v), _bits(vals[0]))
    # a fully per-cell table that is NOT uniform, against the same table through an index
    A, B = gpu.DeviceMatrix(c['V']), gpu.DeviceMatrix(c['V'])
    A.assemble_anisotropic((TABLE3[c['idx']], None, None))
    B.assemble_anisotropic((TABLE3, c['idx'], None))
    assert np.array_equal(_bits(A.to_csr()[2]), _bits(B.to_csr()[2]))


# ---------------------------------------------------------------------------------------------- 4. frame objectivity
def test_rotating_the_body_and_the_frames_rotates_the_operator(gpu, region_cases):
    c = region_cases["file"]
    Q = ar.random_rotations(1, 77)[0]
    K = gpu.DeviceMatrix(c['V'])
    K.assemble_anisotropic((TABLE3, c['idx'], c['R']))
    meshq = gpu.DeviceMesh(c['co'] @ Q.T, c['ce'])
    Vq = gpu.DeviceSpace(meshq, 3)
    Kq = gpu.DeviceMatrix(Vq)
    Kq.assemble_anisotropic((TABLE3, c['idx'], np.einsum('ij,cjk->cik', Q, c['R'])))
    T = sp.kron(sp.identity(len(c['co'])), Q).tocsr()
    ref = (T @ _csr(K) @ T.T).tocsr()
    ref.sort_indices()
    _check_against(_csr(Kq), ref)
    # plane strain: a rotation about z
    c2 = region_cases["triangles"]
    Qz = ar.rotation_about([0.0, 0.0, 1.0], 0.7)
    K2 = gpu.DeviceMatrix(c2['V'])
    K2.assemble_anisotropic((TABLE3, c2['idx'], c2['R']))
    co3 = np.zeros((len(c2['co']), 3))
    co3[:, :2] = c2['co'][:, :2]
    V2q = gpu.DeviceSpace(gpu.DeviceMesh((co3 @ Qz.T)[:, :c2['co'].shape[1]], c2['ce']), ncomp=2)
    K2q = gpu.DeviceMatrix(V2q)
    K2q.assemble_anisotropic((TABLE3, c2['idx'], np.einsum('ij,cjk->cik', Qz, c2['R'])))
    T2 = sp.kron(sp.identity(len(c2['co'])), Qz[:2, :2]).tocsr()
    ref2 = (T2 @ _csr(K2) @ T2.T).tocsr()
    ref2.sort_indices()
    _check_against(_csr(K2q), ref2)


# ---------------------------------------------------------------------------------------------- 5. the eigenstrain load
ALPHA_DT = 50.0 * np.array([[1e-6, 2e-6, -1e-6], [2e-6, 3e-5, 4e-6], [-1e-6, 4e-6, 2e-5]])


def _eigenstrain(nc, d):
    A = ALPHA_DT
    if d == 3:
        return np.tile([A[0, 0], A[1, 1], A[2, 2], A[0, 1], A[0, 2], A[1, 2]], (nc, 1))
    return np.tile([A[0, 0], A[1, 1], A[2, 2], A[0, 1]], (nc, 1))       # plane strain: eps*_zz stays, no out-of-plane shear


@pytest.mark.parametrize("name", ["file", "box", "triangles"])
def test_eigenstrain_load_balances_the_linear_field(gpu, region_cases, name):
    """u_lin = eps* x has the strain eps* in every cell: K u_lin = int (C : eps*) : grad v on EVERY row, and sigma = C : (eps - eps*) = 0.
    Plane strain: eps*_zz has no displacement counterpart (e_zz = 0), so the field balances the load of the in-plane part."""
    c = region_cases[name]
    d, nc, V = c['d'], len(c['ce']), c['V']
    material = (TABLE3, c['idx'], c['R'])
    eig = _eigenstrain(nc, d)
    if d == 2:
        eig[:, 2] = 0.0
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_anisotropic_load(V, material, eig, b, add=False)
    bh = b.get()
    bref = ar.eigenstress_load(len(c['co']), c['co'], c['ce'], c['Dg'], eig)
    assert np.abs(bh - bref).max() <= 1e-12 * np.abs(bref).max()
    u_lin = (c['co'][:, :d] @ ALPHA_DT[:d, :d].T).ravel()
    K = gpu.DeviceMatrix(V)
    K.assemble_anisotropic(material)
    x, y = gpu.DeviceVector(V.n_local, u_lin), gpu.DeviceVector(V.n_owned)
    K.spmv(x, y)
    print(name, "max|K u_lin - b| / max|b| = %.3e" % (np.abs(y.get() - bh).max() / np.abs(bh).max()))
    assert np.abs(y.get() - bh).max() <= 1e-12 * np.abs(bh).max()
    # add=True on top of itself doubles it
    gpu.assemble_anisotropic_load(V, material, eig, b, add=True)
    assert np.abs(b.get() - 2.0 * bh).max() <= 4 * np.finfo(float).eps * np.abs(bh).max()
    s_eig = gpu.anisotropic_stress(V, None, material, eigenstrain=eig, cell_stress=True)
    s_lin = gpu.anisotropic_stress(V, x, material, eigenstrain=eig, cell_stress=True)
    assert np.abs(s_eig + ar.cell_stress(c['co'], c['ce'], None, c['Dg'], -eig)).max() <= 1e-12 * np.abs(s_eig).max()
    print(name, "max|sigma(u_lin) - C:eps*| / max|C:eps*| = %.3e" % (np.abs(s_lin).max() / np.abs(s_eig).max()))
    assert np.abs(s_lin).max() <= 1e-12 * np.abs(s_eig).max()


# ---------------------------------------------------------------------------------------------- 6. stress and von Mises load
@pytest.mark.parametrize("name", ["file", "box", "triangles"])
def test_stress_and_von_mises_load_of_a_random_field(gpu, region_cases, name):
    c = region_cases[name]
    d, nc, V = c['d'], len(c['ce']), c['V']
    P = gpu.DeviceSpace(c['mesh'], 1)
    uh = 1e-3 * np.random.default_rng(9).standard_normal(V.n_local)
    u = gpu.DeviceVector(V.n_local, uh)
    eig = _eigenstrain(nc, d) * np.linspace(0.5, 1.5, nc)[:, None]
    material = (TABLE3, c['idx'], c['R'])
    b = gpu.DeviceVector(P.n_owned)
    sig = gpu.anisotropic_stress(V, u, material, eigenstrain=eig, cell_stress=True, p1_space=P, vm_rhs=b)
    ref = ar.cell_stress(c['co'], c['ce'], uh[:V.n_owned], c['Dg'], eig)
    assert sig.shape == ref.shape == (nc, 6 if d == 3 else 4)
    assert np.abs(sig - ref).max() <= 1e-12 * np.abs(ref).max()
    bref = ar.von_mises_rhs(len(c['co']), c['co'], c['ce'], ref)
    assert np.abs(b.get() - bref).max() <= 1e-12 * np.abs(bref).max()
    # isotropic D: the right-hand side of fs_assemble_von_mises
    mu, lm = fo.lame(E_ISO, NU_ISO)
    b2, b3 = gpu.DeviceVector(P.n_owned), gpu.DeviceVector(P.n_owned)
    gpu.anisotropic_stress(V, u, (ar.to_library(ar.isotropic_voigt(E_ISO, NU_ISO))[None], None, None), p1_space=P, vm_rhs=b2)
    gpu.assemble_von_mises(V, u, mu, lm, P, b3)
    assert np.abs(b2.get() - b3.get()).max() <= 1e-12 * np.abs(b3.get()).max()


# ---------------------------------------------------------------------------------------------- 7. what the backend refuses
def test_wrong_lengths_ranges_and_spaces_are_refused(gpu):
    co, ce = fo.box_mesh((0, 0, 0), (1.0, 1.0, 1.0), 2, 2, 2)
    nc = len(ce)
    mesh = gpu.DeviceMesh(co, ce)
    V = gpu.DeviceSpace(mesh, 3)
    A = gpu.DeviceMatrix(V)
    D = TABLE3
    R = ar.random_rotations(nc, 1)
    ok_index = np.zeros(nc, dtype=np.int32)
    bad = [(D, ok_index[:-1], None),                    # index too short
           (D, None, None),                             # 3 materials, no index, 48 cells
           (D, ok_index, R[:-1]),                       # frames too short
           (D[:, :5, :5], ok_index, None),              # not 6x6
           (D, ok_index.astype(np.float64), None),      # index not integer
           (D, ok_index + 3, None),                     # index out of range (the C call's check)
           (D, ok_index - 1, None)]
    for k, material in enumerate(bad):
        with pytest.raises(gpu.BackendError):
            A.assemble_anisotropic(material)
    skew = D.copy()
    skew[0, 0, 1] *= 2.0
    with pytest.raises(gpu.BackendError, match="symmetric"):
        A.assemble_anisotropic((skew, ok_index, None))
    nan = D.copy()
    nan[1, 2, 2] = np.nan
    with pytest.raises(gpu.BackendError, match="finite"):
        A.assemble_anisotropic((nan, ok_index, None))
    with pytest.raises(gpu.BackendError):
        A.assemble_anisotropic((D, ok_index, None), mass=('cell', np.ones(nc - 1)))
    b = gpu.DeviceVector(V.n_owned)
    with pytest.raises(gpu.BackendError):
        gpu.assemble_anisotropic_load(V, (D, ok_index, None), np.zeros((nc, 4)), b)
    with pytest.raises(gpu.BackendError):
        gpu.anisotropic_stress(V, None, (D, ok_index, None), eigenstrain=np.zeros((nc - 1, 6)), cell_stress=True)
    with pytest.raises(gpu.BackendError):
        gpu.anisotropic_stress(V, None, (D, ok_index, None), p1_space=gpu.DeviceSpace(mesh, 1))
    S = gpu.DeviceSpace(mesh, 1)
    with pytest.raises(gpu.BackendError):               # a scalar space
        gpu.DeviceMatrix(S).assemble_anisotropic((D, ok_index, None))
    V2 = gpu.DeviceSpace(mesh, 3, degree=2)
    with pytest.raises(gpu.BackendError):               # a P2 space
        gpu.DeviceMatrix(V2).assemble_anisotropic((D, ok_index, None))
    with pytest.raises(gpu.BackendError):
        gpu.assemble_anisotropic_load(V2, (D, ok_index, None), np.zeros((nc, 6)), gpu.DeviceVector(V2.n_owned))
    # plane strain: a material that couples the plane with the out-of-plane shears, a frame that tilts z
    c2, e2 = fo.rectangle_mesh((0.0, 0.0), (1.0, 1.0), 2, 2)
    T = gpu.DeviceSpace(gpu.DeviceMesh(c2, e2), ncomp=2)
    tilted = ar.global_D(D[:1], None, np.tile(ar.rotation_about([1.0, 0.0, 0.0], 0.4), (1, 1, 1)), 1)
    with pytest.raises(gpu.BackendError, match="monoclinic"):
        gpu.DeviceMatrix(T).assemble_anisotropic((0.5 * (tilted + tilted.transpose(0, 2, 1)), None, None))
    with pytest.raises(gpu.BackendError, match="about z"):
        gpu.DeviceMatrix(T).assemble_anisotropic((D[:1], None, np.tile(ar.rotation_about([1.0, 0.0, 0.0], 0.4), (len(e2), 1, 1))))
    # and the matrix is untouched by the refused calls
    A.assemble_anisotropic((D, ok_index, None))
    assert np.isfinite(A.to_csr()[2]).all()


# ---------------------------------------------------------------------------------------------- solver cases
def _rollers(dim):
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    def plane(i):
        return AutoSubDomain(lambda x: near(x[i], 0))

    bcs = OrderedDict()
    for i, name in enumerate("xyz"[:dim]):
        val = [None] * dim
        val[i] = Constant(0.0)
        bcs["roller_" + name] = {'boundary': plane(i), 'boundary_id': i + 1, 'type': 'Dirichlet', 'value': tuple(val)}
    return bcs


def _solver(material, dim=3, n=(2, 2, 8), size=(1.0, 1.0, 2.0), bcs=None, regions=None, preconditioner=None, modal=None, degree=1,
            **extra):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, MeshFunction
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    if dim == 3:
        mesh = BoxMesh(Point(0, 0, 0), Point(*size), *n)
    else:
        mesh = RectangleMesh(Point(0, 0), Point(*size[:2]), *n[:2])
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = dict({'name': 'composite', 'density': 1600.0, 'thermal_expansion_coefficient': 0.0}, **material)
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", degree)
    s['boundary_conditions'] = bcs if bcs is not None else _rollers(dim)
    s['solver_settings']['reference_values'] = {'temperature': 293}
    sp_ = {'krylov_relative_tolerance': 1e-12}
    if preconditioner:
        sp_['preconditioner'] = preconditioner
    s['solver_settings']['solver_parameters'] = sp_
    if modal is not None:
        s['solver_settings']['modal_settings'] = dict(modal)
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = None
    s.update(extra)
    solver = LinearElasticitySolver(s)
    solver.reference_load_sign = False
    if regions is not None:
        sub = MeshFunction("size_t", mesh, dim)
        sub.array()[:] = regions(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1))
        solver.subdomains = sub
    return solver


def _halves(axis, at):
    return lambda cen: np.where(cen[:, axis] < at, 1, 2)


# ---------------------------------------------------------------------------------------------- 8. on-axis bar
@pytest.mark.parametrize("preconditioner", [None, "jacobi"])
def test_on_axis_orthotropic_bar_is_exact(gpu, preconditioner):
    """Rollers on x = 0, y = 0, z = 0 and the traction T on z = L: sigma = T e_z e_z, u = T (S13 x, S23 y, S33 z); von Mises |T|."""
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    T, L = 3e7, 2.0
    bcs = _rollers(3)
    bcs["pull"] = {'boundary': AutoSubDomain(lambda x: near(x[2], L)), 'boundary_id': 4, 'type': 'stress', 'value': Constant((0.0, 0.0, T))}
    solver = _solver({'orthotropic': dict(ar.CFRP)}, bcs=bcs, preconditioner=preconditioner)
    u = solver.solve()
    X = solver.function_space.node_coordinates()
    exact = T * X * np.array([CFRP_S[0, 2], CFRP_S[1, 2], CFRP_S[2, 2]])[None, :]
    print("bar: max error / max exact = %.3e" % (np.abs(u.node_values() - exact).max() / np.abs(exact).max()))
    assert np.abs(u.node_values() - exact).max() <= 1e-8 * np.abs(exact).max()
    if preconditioner is None:
        assert solver.last_solve_stats.get('amg_levels', 0) >= 1
    vm = solver.von_Mises(u).vector().get_local()
    assert np.abs(vm - T).max() <= 1e-8 * T
    s = solver.sigma(u)
    assert np.abs(s - T * np.diag([0.0, 0.0, 1.0])[None]).max() <= 1e-8 * T


def test_on_axis_orthotropic_strip_in_plane_strain_is_exact(gpu):
    """Plane strain, rollers on x = 0 and y = 0, the traction T on x = L: u = T (S'11 x, S'12 y) with the plane-strain compliance
    S'_ij = S_ij - S_i3 S_j3 / S_33; the 2-D von Mises convention gives sqrt(5/6) |T|."""
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    T, L = 3e7, 2.0
    bcs = _rollers(2)
    bcs["pull"] = {'boundary': AutoSubDomain(lambda x: near(x[0], L)), 'boundary_id': 4, 'type': 'stress', 'value': Constant((T, 0.0))}
    solver = _solver({'orthotropic': dict(ar.CFRP)}, dim=2, n=(8, 2), size=(L, 1.0), bcs=bcs)
    u = solver.solve()
    Sp = ar.plane_strain_compliance(CFRP_S[:3, :3])
    X = solver.function_space.node_coordinates()[:, :2]
    exact = T * X * np.array([Sp[0, 0], Sp[0, 1]])[None, :]
    assert np.abs(u.node_values() - exact).max() <= 1e-8 * np.abs(exact).max()
    vm = solver.von_Mises(u).vector().get_local()
    assert np.abs(vm - np.sqrt(5.0 / 6.0) * T).max() <= 1e-8 * T


# ---------------------------------------------------------------------------------------------- 9. off-axis patch test
def test_off_axis_material_in_two_regions_follows_a_prescribed_homogeneous_strain(gpu):
    """The fibres are turned by 30 degrees about a skew axis.  Region 1 gives that material as its tensor rotated on the host and no
    frame (the identity), region 2 as the on-axis tensor with the frame: the same material twice, so u = eps0 x prescribed on all six
    faces is the solution in the interior as well (a homogeneous strain is in equilibrium only in a homogeneous body) - and only if the
    frame path of the kernel equals the rotated tensor."""
    from fenicssolver_amd.fem import AutoSubDomain, Expression
    R = ar.rotation_about([1.0, 2.0, -1.0], np.pi / 6)
    rotated = ar.matrix6(ar.rotate4(ar.tensor4(CFRP_V, ar.VOIGT), R), ar.VOIGT)
    rotated = 0.5 * (rotated + rotated.T)
    eps0 = 1e-3 * np.array([[1.0, 0.4, -0.3], [0.4, -0.5, 0.2], [-0.3, 0.2, 0.8]])
    value = Expression(tuple("%.17g*x[0] + %.17g*x[1] + %.17g*x[2]" % tuple(row) for row in eps0), degree=1)
    bcs = OrderedDict()
    bcs["skin"] = {'boundary': AutoSubDomain(lambda x, on_boundary: on_boundary), 'boundary_id': 1, 'type': 'Dirichlet', 'value': value}
    material = {'elasticity_tensor': {'a': {'subdomain_id': 1, 'value': rotated}, 'b': {'subdomain_id': 2, 'value': CFRP_V}},
                'material_orientation': {'a': {'subdomain_id': 1, 'value': np.eye(3)}, 'b': {'subdomain_id': 2, 'value': R}}}
    solver = _solver(material, n=(4, 4, 6), size=(1.0, 1.0, 1.5), bcs=bcs, regions=_halves(2, 0.75))
    u = solver.solve()
    X = solver.function_space.node_coordinates()
    exact = X @ eps0.T
    interior = np.all((X > 1e-12) & (X < np.array([1.0, 1.0, 1.5]) - 1e-12), axis=1)
    assert interior.sum() == 3 * 3 * 5
    err = np.abs(u.node_values() - exact)[interior].max()
    print("patch: interior error / max exact = %.3e" % (err / np.abs(exact).max()))
    assert err <= 1e-8 * np.abs(exact).max()
    assert solver.last_solve_stats.get('amg_levels', 0) >= 1


# ---------------------------------------------------------------------------------------------- 10. thermal expansion
def test_free_thermal_expansion_of_two_orthotropic_regions(gpu):
    """Rollers on three planes, two regions with different D and the same principal expansions on axis, dT = 50: the body expands
    freely, u = dT (a1 x, a2 y, a3 z), and sigma(u) equals the eigenstress C : alpha dT cell by cell."""
    alpha, dT = np.array([1e-6, 3e-5, 2e-5]), 50.0
    material = {'elasticity_tensor': {'a': {'subdomain_id': 1, 'value': CFRP_V}, 'b': {'subdomain_id': 2, 'value': GFRP_V}},
                'thermal_expansion_coefficient': list(alpha)}
    solver = _solver(material, n=(2, 2, 6), regions=_halves(2, 1.5), temperature_distribution=343.0)
    u = solver.solve()
    X = solver.function_space.node_coordinates()
    exact = dT * alpha[None, :] * X
    print("thermal: max error / max exact = %.3e" % (np.abs(u.node_values() - exact).max() / np.abs(exact).max()))
    assert np.abs(u.node_values() - exact).max() <= 1e-9 * np.abs(exact).max()
    table, index, _ = solver.stiffness_tensor()
    eigenstress = np.einsum('cij,j->ci', table[index][:, :3, :3], alpha * dT)            # C : alpha dT: normal components only
    s = solver.sigma(u)
    assert len(np.unique(index)) == 2
    diag = np.stack([s[:, 0, 0], s[:, 1, 1], s[:, 2, 2]], axis=1)
    off = np.stack([s[:, 0, 1], s[:, 0, 2], s[:, 1, 2]], axis=1)
    assert max(np.abs(diag - eigenstress).max(), np.abs(off).max()) <= 1e-8 * np.abs(eigenstress).max()


# ---------------------------------------------------------------------------------------------- 11. modal analysis
def test_modes_of_a_clamped_orthotropic_box_match_the_reference(gpu):
    """The criterion and the bounds of tests/test_gpu_modal.py (_check_against_dense), against eigsh on the numpy reference's K, M."""
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    nm = 6
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0)), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0.0, 0.0, 0.0))}
    solver = _solver({'orthotropic': dict(ar.CFRP)}, n=(4, 4, 12), size=(1.0, 0.8, 3.0), bcs=bcs, modal={'number_of_modes': nm})
    solver.solve_modal()
    assert solver.modal_stats['n_converged'] == nm
    co, ce = solver.mesh.coordinates(), solver.mesh.cells()
    D = np.broadcast_to(ar.to_library(CFRP_V), (len(ce), 6, 6))
    K = ar.assemble(len(co), ce, ar.local_stiffness(co, ce, D), 3)
    M = ar.assemble(len(co), ce, ar.local_mass(co, ce, 1600.0), 3)
    free = np.flatnonzero(np.repeat(co[:, 2] > 1e-12, 3))
    Kf, Mf = K[free][:, free].tocsc(), M[free][:, free].tocsc()
    lam_ref, phi_ref = spla.eigsh(Kf, k=nm, M=Mf, sigma=0.0, which='LM')
    order = np.argsort(lam_ref)
    lam_ref, phi_ref = lam_ref[order], phi_ref[:, order]
    lam = solver.eigenvalues
    print("modal: lambda", lam, "reference", lam_ref)
    assert lam.shape == (nm,) and np.all(np.diff(lam) >= 0)
    assert np.all(np.abs(lam - lam_ref) <= 1e-9 * np.abs(lam_ref).max()), (lam, lam_ref)
    Phi = np.stack([f.vector().get_local() for f in solver.modes], axis=1)
    cons = np.setdiff1d(np.arange(Phi.shape[0]), free)
    assert np.all(Phi[cons] == 0.0)
    P = Phi[free]
    assert np.abs(P.T @ (Mf @ P) - np.eye(nm)).max() <= 1e-10
    for j in range(nm):
        r = Kf @ P[:, j] - lam[j] * (Mf @ P[:, j])
        assert np.linalg.norm(r) <= 1e-8 * abs(lam[j]) * np.linalg.norm(Mf @ P[:, j]), j
        c = abs(P[:, j] @ (Mf @ phi_ref[:, j])) / np.sqrt((P[:, j] @ (Mf @ P[:, j])) * (phi_ref[:, j] @ (Mf @ phi_ref[:, j])))
        assert c >= 1 - 1e-7, (j, c)
    assert np.allclose(solver.natural_frequencies, np.sqrt(np.maximum(lam, 0)) / (2 * np.pi))


# ---------------------------------------------------------------------------------------------- 12. refusals
def test_refusals_come_before_any_device_work(gpu, monkeypatch):
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd.fem import AutoSubDomain, near
    from fenicssolver_amd import backend, fem

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    for name in ("DeviceMatrix", "DeviceVector", "DeviceSpace", "DeviceMesh", "AMG", "krylov_solve", "eigen_solve", "buckling_solve"):
        monkeypatch.setattr(backend, name, boom)
    monkeypatch.setattr(fem.FunctionSpace, "device", boom, raising=False)
    ANISO = {'orthotropic': dict(ar.CFRP)}
    for btype in ("contact", "sliding"):
        bcs = _rollers(3)
        bcs["floor"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 2.0)), 'boundary_id': 4, 'type': btype, 'value': 0.0}
        with pytest.raises(SolverError, match="'contact' / 'sliding'"):
            _solver(ANISO, bcs=bcs).solve()
    with pytest.raises(SolverError, match="P2 displacement spaces are not supported"):
        _solver(ANISO, n=(1, 1, 2), degree=2).solve()
    dyn = _solver(ANISO)
    dyn.solving_dynamics = True
    with pytest.raises(SolverError, match="solving_dynamics"):
        dyn.solve()
    with pytest.raises(SolverError, match="does not take an anisotropic material"):
        _solver(ANISO).solve_buckling()
    with pytest.raises(SolverError, match="given together with"):
        _solver(dict(ANISO, elastic_modulus=2e11, poisson_ratio=0.3)).solve()
    with pytest.raises(SolverError, match="not a proper rotation"):
        _solver(dict(ANISO, material_orientation=np.diag([1.0, -1.0, 1.0]))).solve()
    per = _solver(ANISO)
    monkeypatch.setattr(per.function_space, "periodic_pairs", lambda: (np.array([0]), np.array([1])), raising=False)
    with pytest.raises(SolverError, match="periodic"):
        per.solve()
    from fenicssolver_amd import parallel
    ranks = _solver(ANISO)
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(SolverError, match="one rank"):
        ranks.solve()


# ---------------------------------------------------------------------------------------------- 13. nothing cached across the paths
def test_isotropic_case_is_bitwise_the_same_before_and_after_an_anisotropic_solve(gpu):
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near

    def case(material):
        bcs = _rollers(3)
        bcs["pull"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 2.0)), 'boundary_id': 4, 'type': 'stress', 'value': Constant((1e6, 0.0, 3e7))}
        return _solver(material, bcs=bcs)
    iso = {'elastic_modulus': E_ISO, 'poisson_ratio': NU_ISO}
    s1 = case(iso)
    before = s1.solve().vector().get_local().copy()
    vm_before = s1.von_Mises(s1.w_current).vector().get_local().copy()
    a = case({'orthotropic': dict(ar.CFRP), 'material_orientation': ar.rotation_about([1.0, 2.0, -1.0], np.pi / 6)})
    ua = a.solve()
    a.von_Mises(ua)
    assert np.abs(ua.vector().get_local()).max() > 0.0
    s2 = case(iso)
    after = s2.solve().vector().get_local()
    assert np.array_equal(_bits(before), _bits(after))
    assert np.array_equal(_bits(vm_before), _bits(s2.von_Mises(s2.w_current).vector().get_local()))
    # and the solver that ran first, once more
    again = s1.solve().vector().get_local()
    assert np.array_equal(_bits(before), _bits(again))


# ---------------------------------------------------------------------------------------------- 14. every load, the transient loop
@pytest.mark.parametrize("dim", [3, 2])
def test_isotropic_tensor_through_the_anisotropic_path_equals_the_isotropic_solver(gpu, dim):
    """An isotropic material given as 'elasticity_tensor' runs through the new operator, the new thermal load (per-cell eigenstrain
    against the div_coef load) and the same body force, pressure and displacement BCs in the reference's transient loop: the field
    of the isotropic solver, and its von Mises stress, to the solver tolerance."""
    from fenicssolver_amd.fem import AutoSubDomain, Constant, near
    from fenicssolver_amd.LinearElasticitySolver import isotropic_stiffness
    L = 2.0

    def case(material):
        ax = 2 if dim == 3 else 0
        bcs = OrderedDict()
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[ax], 0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0,) * dim)}
        bcs["push"] = {'boundary': AutoSubDomain(lambda x: near(x[ax], L)), 'boundary_id': 2, 'type': 'pressure', 'value': 2e6}
        s = _solver(dict(material, thermal_expansion_coefficient=1.2e-5), dim=dim, n=(2, 2, 8) if dim == 3 else (8, 2),
                    size=(1.0, 1.0, L) if dim == 3 else (L, 1.0), bcs=bcs, temperature_distribution=343.0,
                    body_source=Constant((0.0, -7800.0 * 9.81, 0.0)[:dim]))
        s.transient_settings.update({'transient': True, 'starting_time': 0.0, 'time_step': 0.1, 'ending_time': 0.2})
        return s
    iso = case({'elastic_modulus': E_ISO, 'poisson_ratio': NU_ISO})
    ui = iso.solve()
    ani = case({'elasticity_tensor': isotropic_stiffness(E_ISO, NU_ISO)})
    ua = ani.solve()
    assert ani.current_step == iso.current_step >= 2
    a, b = ua.vector().get_local(), ui.vector().get_local()
    print("wiring %d-D: max difference / max = %.3e" % (dim, np.abs(a - b).max() / np.abs(b).max()))
    assert np.abs(a - b).max() <= 1e-8 * np.abs(b).max()
    vi, va = iso.von_Mises(ui).vector().get_local(), ani.von_Mises(ua).vector().get_local()
    assert np.abs(va - vi).max() <= 1e-8 * np.abs(vi).max()
    assert np.abs(ani.sigma(ua) - iso.sigma(ui)).max() <= 1e-8 * np.abs(iso.sigma(ui)).max()


# ---------------------------------------------------------------------------------------------- 15. a mesh uploaded in locality order
class _SkewFrames:
    """Per-cell frames as a degree-0 expression: a rotation about a skew axis by an angle that varies over the body."""

    @staticmethod
    def at(x):
        return ar.rotation_about([1.0, 2.0, -1.0], 0.3 * x[0] + 0.2 * x[1] + 0.1 * x[2])


def _file_mesh_solver(data_dir, transient=False):
    from fenicssolver_amd.fem import Mesh, VectorFunctionSpace, MeshFunction, AutoSubDomain, Constant, UserExpression, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver

    class Frames(UserExpression):
        def value_shape(self):
            return (9,)

        def eval(self, value, x):
            value[:] = _SkewFrames.at(x).ravel()
    mesh = Mesh(os.path.join(data_dir, "mesh.xml"))
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0)), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0.0, 0.0, 0.0))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'laminate', 'density': 1600.0, 'thermal_expansion_coefficient': [1e-6, 3e-5, 2e-5],
                     'elasticity_tensor': {'a': {'subdomain_id': 1, 'value': CFRP_V}, 'b': {'subdomain_id': 2, 'value': GFRP_V},
                                           'c': {'subdomain_id': 3, 'value': ar.isotropic_voigt(3.5e9, 0.35)}},
                     'material_orientation': Frames(degree=0)}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = 343.0
    if transient:
        s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 0.1, 'ending_time': 0.2}
    solver = LinearElasticitySolver(s)
    solver.reference_load_sign = False
    co, ce = mesh.coordinates(), mesh.cells()
    sub = MeshFunction("size_t", mesh, 3)
    sub.array()[:] = _three_regions(co, ce, 3) + 1
    solver.subdomains = sub
    return solver


def test_file_mesh_in_locality_order_gets_its_material_cell_by_cell(gpu, data_dir, monkeypatch):
    """FS_RENUMBER=1 (automatic from 50 000 vertices): the device numbers vertices and cells along a Morton curve, the host arrays keep
    the file numbering.  Three regions, per-cell frames and the thermal eigenstrain must follow their cells: the assembled system
    against the numpy reference in the device's numbering, the solution against the run in file order, and the calls that come after a
    first solve - von_Mises, the next transient step - on the same solver."""
    monkeypatch.setenv("FS_RENUMBER", "1")
    solver = _file_mesh_solver(data_dir, transient=True)
    F, bcs = solver.generate_form(0, None, None, None, None)
    A, b = solver.assemble_system(F, [])
    loc = F.space.localizer()
    assert loc is not None and not np.array_equal(loc.part.cell_gids, np.arange(len(loc.part.cell_gids)))      # cells ARE permuted
    co, ce = solver.mesh.coordinates(), solver.mesh.cells()
    nc = len(ce)
    cen = co[ce.astype(np.int64)].mean(axis=1)
    R = np.stack([_SkewFrames.at(x) for x in cen])
    idx = _three_regions(co, ce, 3)
    Dg = ar.global_D(TABLE3, idx, R, nc)
    Kref = _reference_operator(co, ce, 3, Dg)
    alpha_g = np.einsum('cik,k,cjk->cij', R, np.array([1e-6, 3e-5, 2e-5]), R) * 50.0
    eig = np.stack([alpha_g[:, 0, 0], alpha_g[:, 1, 1], alpha_g[:, 2, 2], alpha_g[:, 0, 1], alpha_g[:, 0, 2], alpha_g[:, 1, 2]], axis=1)
    bref = ar.eigenstress_load(len(co), co, ce, Dg, eig)
    p = (np.asarray(loc.l2g, dtype=np.int64)[:, None] * 3 + np.arange(3)).ravel()
    Rp = Kref[p][:, p].tocsr()
    Rp.sort_indices()
    _check_against(_csr(A), Rp)
    assert np.abs(b.get() - bref[p]).max() <= 1e-12 * np.abs(bref).max()
    # the whole solve, two transient steps, then von_Mises: the field of the run in file order
    u = solver.solve()
    assert solver.current_step >= 2
    vm = solver.von_Mises(u).vector().get_local()
    monkeypatch.setenv("FS_RENUMBER", "0")
    plain = _file_mesh_solver(data_dir, transient=True)
    up = plain.solve()
    assert plain.function_space.localizer() is None
    a, c = u.vector().get_local(), up.vector().get_local()
    print("renumbered against file order: max difference / max = %.3e" % (np.abs(a - c).max() / np.abs(c).max()))
    assert np.abs(c).max() > 0.0 and np.abs(a - c).max() <= 1e-8 * np.abs(c).max()
    vmp = plain.von_Mises(up).vector().get_local()
    assert np.abs(vm - vmp).max() <= 1e-8 * np.abs(vmp).max()
    # modal analysis does not serve the renumbered upload: it says so instead of reading the material by the wrong cells
    from fenicssolver_amd.SolverBase import SolverError
    monkeypatch.setenv("FS_RENUMBER", "1")
    modal = _file_mesh_solver(data_dir)
    with pytest.raises(SolverError, match="locality order"):
        modal.solve_modal()
