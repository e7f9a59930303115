"""LargeDeformationSolver and fs_assemble_large_deformation on the MI355X: the reduced system against the numpy restatement
(tests/large_deformation_reference.py) at random states, the rigid rotation, the reference example and a 3-D beam against the host
monolithic Newton step by step, the AMG set-ups, the product kind, repeatability, a mesh uploaded in locality order and save()."""
import copy
import os
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sps

import large_deformation_reference as ldr
from test_large_deformation_host import example_settings, QUIET

pytestmark = pytest.mark.gpu


def _csr(A):
    rp, ci, va, (nr, nc) = A.to_csr()
    return sps.csr_matrix((va, ci, rp), shape=(nr, nc))


def _end_facets(co, cells, x_end):
    """(cell, local vertex opposite) of the boundary facets on the plane x = x_end."""
    out = []
    d = co.shape[1]
    for c in range(len(cells)):
        for k in range(d + 1):
            if np.all(np.abs(co[np.delete(cells[c], k), 0] - x_end) < 1e-12):
                out.append((c, k))
    return out


def _mesh(d):
    from fenicssolver_amd.fem import RectangleMesh, BoxMesh, Point
    if d == 2:
        return RectangleMesh(Point(0.0, 0.0), Point(3.0, 1.0), 6, 2, 'crossed')
    return BoxMesh(Point(0, 0, 0), Point(2.0, 1.0, 0.8), 4, 3, 2)


class _Dev:
    def __init__(self, mesh):
        from fenicssolver_amd import backend
        from fenicssolver_amd.fem import FunctionSpace
        backend.init()
        self.d = d = mesh.geometry().dim()
        self.V = FunctionSpace(mesh, "CG", 1, _ncomp=d)
        Vd = self.V.device()
        assert self.V.localizer() is None
        self.nv = nv = mesh.num_vertices()
        self.W4 = backend.DeviceSpace(Vd.mesh, 4, 1)
        self.J = backend.DeviceMatrix(self.W4)
        self.vec = {k: backend.DeviceVector(n) for k, n in (('u', nv * d), ('u0', nv * d), ('w', nv * 4), ('w0', nv * 4), ('rhs', nv * 4))}

    def assemble(self, P, x, x0, mask, facets, g):
        from fenicssolver_amd import backend
        d, nv = self.d, self.nv
        u, v, p = P.split(x)
        u0, v0, p0 = P.split(x0)
        blk = lambda v_, p_: np.concatenate([v_, np.zeros((nv, 3 - d)), p_[:, None]], axis=1).reshape(-1)   # noqa: E731
        self.vec['u'].set(np.ascontiguousarray(u).reshape(-1))
        self.vec['u0'].set(np.ascontiguousarray(u0).reshape(-1))
        self.vec['w'].set(blk(v, p))
        self.vec['w0'].set(blk(v0, p0))
        fc = np.array([f[0] for f in facets], dtype=np.int32)
        fo = np.array([f[1] for f in facets], dtype=np.int32)
        info = backend.assemble_large_deformation(self.J, self.vec['rhs'], self.vec['u'], self.vec['w'], self.vec['u0'], self.vec['w0'],
                                                  P.dt, P.q, P.mu, P.lmbda, mask, body_force=tuple(P.body) + (0.0,) * (3 - d),
                                                  facet_cell=fc, facet_opposite=fo, facet_g=np.asarray(g).reshape(len(fc), d))
        return _csr(self.J), self.vec['rhs'].get()[:4 * nv], info


def _random_case(d, seed):
    rng = np.random.default_rng(seed)
    mesh = _mesh(d)
    co, cells = mesh.coordinates(), mesh.cells().astype(np.int64)
    fl = _end_facets(co, cells, co[:, 0].max())
    g = rng.normal(size=(len(fl), d))
    P = ldr.Problem(co, cells, 0.2, 0.5, 1.7, 2.9, body=rng.normal(size=d), facets=[(c, k, g[i]) for i, (c, k) in enumerate(fl)])
    x = 0.05 * rng.normal(size=P.nv * P.nb)
    x0 = 0.05 * rng.normal(size=P.nv * P.nb)
    xs, x0s = x.reshape(P.nv, P.nb), x0.reshape(P.nv, P.nb)
    left = np.nonzero(co[:, 0] == 0.0)[0]
    xs[left, :2 * d] = x0s[left, :2 * d] = 0.0                       # a clamp: u and v
    mask = np.zeros(P.nv, dtype=np.uint8)
    mask[left] = (1 << d) - 1 | (((1 << d) - 1) << 3)
    pfix = np.nonzero(co[:, 0] == co[:, 0].max())[0][:1]
    mask[pfix] |= 1 << 6
    dofs = np.concatenate([P.dof(left, f, k) for f in ('u', 'v') for k in range(d)] + [P.dof(pfix, 'p')])
    return mesh, P, x, x0, mask, dofs, fl, g


def _to_device_layout(P, A, b, vp):
    """host (v, p) rows / columns -> device block-4 dofs"""
    d = P.d
    node, comp = vp // P.nb, vp % P.nb - d
    slot = np.where(comp < d, comp, 3)
    dev = node * 4 + slot
    n4 = P.nv * 4
    M = sps.coo_matrix(A)
    Ad = sps.csr_matrix((M.data, (dev[M.row], dev[M.col])), shape=(n4, n4))
    bd = np.zeros(n4)
    bd[dev] = b
    return Ad, bd


@pytest.mark.parametrize("d", [2, 3])
def test_reduced_system_matches_the_host_and_repeats_bit_for_bit(d):
    mesh, P, x, x0, mask, dofs, fl, g = _random_case(d, 20 + d)
    dev = _Dev(mesh)
    Jd, rd, info = dev.assemble(P, x, x0, mask, fl, g)
    A, b, vp, _, _, _ = P.reduced_system(x, x0, dofs)
    Ah, bh = _to_device_layout(P, A, b, vp)
    if d == 2:                                   # the dummy slot: identity rows and columns, zero right-hand side
        dummy = np.arange(P.nv) * 4 + 2
        assert np.array_equal(Jd[dummy].toarray(), sps.csr_matrix((np.ones(P.nv), (np.arange(P.nv), dummy)), shape=(P.nv, 4 * P.nv)).toarray())
        assert np.all(rd[dummy] == 0.0) and abs(Jd[:, dummy]).sum() == P.nv
        Ah = Ah + sps.csr_matrix((np.ones(P.nv), (dummy, dummy)), shape=Ah.shape)
    err = abs(Jd - Ah).max()
    assert err <= 1e-12 * abs(Ah).max(), err
    assert np.abs(rd - bh).max() <= 1e-12 * np.abs(bh).max()
    rn = P.residual_norm(x, x0, dofs)
    assert abs(info['residual_norm'] - rn) <= 1e-12 * rn and info['n_bad'] == 0 and info['first_bad_cell'] == -1
    J2, r2, info2 = dev.assemble(P, x, x0, mask, fl, g)
    assert np.array_equal(J2.data, Jd.data) and np.array_equal(r2, rd) and info2['residual_norm'] == info['residual_norm']


@pytest.mark.parametrize("d", [2, 3])
def test_device_residual_vanishes_at_a_rigid_rotation(d):
    mesh = _mesh(d)
    co, cells = mesh.coordinates(), mesh.cells().astype(np.int64)
    P = ldr.Problem(co, cells, 0.25, 0.5, 3.0, 5.0)
    th = 0.8
    Q = np.eye(d)
    Q[:2, :2] = [[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]]
    u = co @ Q.T - co
    x = P.join(u, np.zeros_like(u), np.zeros(P.nv))
    dev = _Dev(mesh)
    mask = np.zeros(P.nv, dtype=np.uint8)
    _, rhs, info = dev.assemble(P, x, x, mask, [], np.zeros((0, d)))
    assert info['residual_norm'] <= 1e-12 and np.abs(rhs).max() <= 1e-12
    x1 = P.join(u * 1.01, np.zeros_like(u), np.zeros(P.nv))
    _, _, info1 = dev.assemble(P, x1, x1, mask, [], np.zeros((0, d)))
    assert info1['residual_norm'] > 1e-3


def _host_run(solver_settings_fn, P_of, n_steps, left, d):
    """the host monolithic Newton, step by step: [(iterations, u, v, p)]"""
    P = P_of()
    dofs = np.concatenate([P.dof(left, f, k) for f in ('u', 'v') for k in range(d)])
    x = np.zeros(P.nv * P.nb)
    out = []
    for _ in range(n_steps):
        x, its = P.newton(x, x, dofs, np.zeros(len(dofs)))
        out.append((its,) + tuple(a.copy() for a in P.split(x)))
    return out


def _compare(solver, host):
    assert len(solver.step_history) == len(host)
    assert solver.step_newton_iterations == [h[0] for h in host]
    for (u, v, p), (_, uh, vh, ph) in zip(solver.step_history, host):
        for a, b in ((u, uh), (v, vh), (p, ph)):
            assert np.abs(a - b).max() <= 1e-7 * np.abs(b).max(), np.abs(a - b).max() / np.abs(b).max()


def test_reference_example_matches_the_host_newton_at_every_step():
    from fenicssolver_amd.LargeDeformationSolver import LargeDeformationSolver
    s = example_settings()
    solver = LargeDeformationSolver(s)
    solver.keep_history = True
    solver.solve()
    mesh = s['mesh']
    co, cells = mesh.coordinates(), mesh.cells().astype(np.int64)
    mu, lmbda = solver.material_constants()
    fl = _end_facets(co, cells, 20.0)
    host = _host_run(None, lambda: ldr.Problem(co, cells, 0.25, 0.5, mu, lmbda, facets=[(c, k, (0.0, 5.0)) for c, k in fl]), 20,
                     np.nonzero(co[:, 0] == 0.0)[0], 2)
    _compare(solver, host)
    assert solver.last_solve_stats['product_kind'] == 4
    assert solver.amg_setups == 0
    u, v, p = solver.split()
    assert np.array_equal(u.vector()._values().reshape(-1, 2), solver.step_history[-1][0])
    print("2-D example: Newton", solver.step_newton_iterations, "FGMRES", solver.step_krylov_iterations[:3])


def beam_settings(n=(40, 4, 4), L=10.0, force=(0.0, 0.0, 2.0), dt=0.25, steps=5, mesh=None):
    from fenicssolver_amd.fem import BoxMesh, Point, AutoSubDomain, near
    from fenicssolver_amd import SolverBase as SB
    if mesh is None:
        mesh = BoxMesh(Point(0, 0, 0), Point(L, 1.0, 1.0), *n)
    bcs = OrderedDict()
    bcs["clamp"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'variable': 'all', 'value': (0.0,) * 7}
    bcs["end"] = {'boundary': AutoSubDomain(lambda x: near(x[0], L)), 'boundary_id': 2, 'type': 'force', 'value': force}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': 1e5, 'poisson_ratio': 0.3, 'density': 1000,
                     'thermal_expansion_coefficient': 2e-6}
    s['mesh'] = mesh
    s['boundary_conditions'] = bcs
    s['solver_settings'] = {'transient_settings': {'transient': True, 'starting_time': 0, 'time_step': dt,
                                                   'ending_time': dt * steps - 1e-9},
                            'reference_values': {'temperature': 293}}
    s['report_settings'] = dict(QUIET)
    return s


def test_3d_beam_matches_the_host_newton_with_one_amg_setup():
    from fenicssolver_amd.LargeDeformationSolver import LargeDeformationSolver
    s = beam_settings()
    solver = LargeDeformationSolver(s)
    solver.keep_history = True
    solver.solve()
    assert len(solver.step_history) == 5
    assert solver.amg_setups == 1
    assert solver.last_solve_stats['product_kind'] == 4
    mesh = s['mesh']
    co, cells = mesh.coordinates(), mesh.cells().astype(np.int64)
    mu, lmbda = solver.material_constants()
    fl = _end_facets(co, cells, 10.0)
    left = np.nonzero(co[:, 0] == 0.0)[0]
    P_of = lambda: ldr.Problem(co, cells, 0.25, 0.5, mu, lmbda, facets=[(c, k, (0.0, 0.0, 2.0)) for c, k in fl])   # noqa: E731
    P = P_of()
    dofs = np.concatenate([P.dof(left, f, k) for f in ('u', 'v') for k in range(3)] + [P.dof(left, 'p')])
    x = np.zeros(P.nv * P.nb)
    host = []
    for _ in range(5):
        x, its = P.newton(x, x, dofs, np.zeros(len(dofs)))
        host.append((its,) + tuple(a.copy() for a in P.split(x)))
    _compare(solver, host)
    print("3-D beam: Newton", solver.step_newton_iterations, "FGMRES", solver.step_krylov_iterations)


def test_two_runs_give_identical_bits():
    from fenicssolver_amd.LargeDeformationSolver import LargeDeformationSolver
    out = []
    for _ in range(2):
        solver = LargeDeformationSolver(beam_settings(n=(12, 3, 3), L=4.0, steps=2))
        solver.solve()
        out.append(solver.w_current.vector()._values().copy())
    assert np.array_equal(out[0], out[1])


def test_mesh_uploaded_in_locality_order_gives_the_file_order_solution(monkeypatch):
    from fenicssolver_amd.LargeDeformationSolver import LargeDeformationSolver
    from fenicssolver_amd.fem import BoxMesh, Mesh, Point
    box = BoxMesh(Point(0, 0, 0), Point(4.0, 1.0, 1.0), 12, 3, 3)
    rng = np.random.default_rng(3)
    perm = rng.permutation(box.num_vertices())                  # a "file" numbering that says nothing about locality
    inv = np.empty_like(perm)
    inv[perm] = np.arange(len(perm))
    co = box.coordinates()[perm]
    cells = inv[box.cells().astype(np.int64)][rng.permutation(box.num_cells())]
    res = {}
    for flag in ("0", "1"):
        monkeypatch.setenv("FS_RENUMBER", flag)
        solver = LargeDeformationSolver(beam_settings(L=4.0, steps=2, mesh=Mesh(coords=co, cells=cells)))
        solver.solve()
        res[flag] = (solver.w_current.vector()._values().copy(), solver.function_space.displacement_space().localizer())
    assert res["0"][1] is None and res["1"][1] is not None
    a, b = res["0"][0], res["1"][0]
    assert np.abs(a - b).max() <= 1e-9 * np.abs(a).max()


def test_save_writes_vtus_with_the_three_fields(tmp_path):
    from fenicssolver_amd.LargeDeformationSolver import LargeDeformationSolver
    s = example_settings(nx=8, ny=2, length=2.0, t_end=0.5)
    solver = LargeDeformationSolver(s)
    solver.solve()
    pvd = str(tmp_path / "ld.pvd")
    solver.save(pvd)
    solver.save(pvd)
    vtus = sorted(p for p in os.listdir(tmp_path) if p.endswith(".vtu"))
    assert vtus == ["ld000000.vtu", "ld000001.vtu"]
    text = open(tmp_path / vtus[0]).read()
    for name, ncomp in (("displacement", 2), ("velocity", 2), ("pressure", 1)):
        assert 'Name="%s" NumberOfComponents="%d"' % (name, ncomp) in text
    import xml.etree.ElementTree as ET
    root = ET.parse(tmp_path / vtus[0]).getroot()
    arrays = {a.get("Name"): np.array(a.text.split(), dtype=float) for a in root.iter("DataArray") if a.get("Name") in
              ("displacement", "velocity", "pressure")}
    u, v, p = solver.split()
    assert np.allclose(arrays["displacement"], u.vector()._values(), rtol=1e-15, atol=0)
    assert np.allclose(arrays["pressure"], p.vector()._values(), rtol=1e-15, atol=0)
    assert "ld000001.vtu" in open(pvd).read()
