"""Frictionless contact and sliding supports on the GPU: the per-node change of basis (fs_matrix_rotate_nodes,
fs_vector_rotate_nodes) and the active-set update (fs_contact_update) against the host reference (tests/contact_reference.py), and
LinearElasticitySolver.solve_contact on a patch test and on the four fixtures against the reference's active-set loop with direct
solves.  The sizes are the smallest with a partial last slice (45 nodes), several slices (72 nodes), an unstructured pattern
(mesh.xml) and block size 2."""
import os

import numpy as np
import pytest
import scipy.sparse as sp

import contact_reference as cr
from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu
EPS = np.finfo(np.float64).eps


def _csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


# ------------------------------------------------------------------------------------------------ spaces and frame sets
def _spaces(gpu, data_dir):
    """(name, coords [n, d], DeviceSpace): the box of 45 nodes, the box of 72 nodes (two slices), mesh.xml, plane strain."""
    for name, (nx, ny, nz), p1 in (("odd box", (4, 2, 2), (2.0, 1.0, 1.0)), ("two slices", (5, 3, 2), (2.0, 1.0, 0.5))):
        mesh = gpu.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), p1)
        xyz, _, _ = mesh.get()
        yield name, xyz, gpu.DeviceSpace(mesh, 3, 1)
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(data_dir, "mesh.xml"))
    yield "mesh.xml", co, gpu.DeviceSpace(gpu.DeviceMesh(co, ce), 3, 1)
    co2, ce2 = fo.rectangle_mesh((0.0, 0.0), (2.0, 0.5), 9, 4)
    yield "plane strain", co2, gpu.DeviceSpace(gpu.DeviceMesh(co2, ce2), 2, 1)


def _frame_sets(co, seed):
    """(nodes, normals): one face (the last coordinate at its minimum) and a scattered set with node 0 and the last node.  The
    normals are generic, with e_k, -e_k and one whose last component is zero among them."""
    n, d = co.shape
    rng = np.random.default_rng(seed)
    face = np.flatnonzero(co[:, d - 1] == co[:, d - 1].min())
    scattered = np.union1d([0, n - 1], rng.choice(n, size=max(3, n // 5), replace=False))
    for nodes in (face, scattered):
        nrm = rng.standard_normal((len(nodes), d))
        nrm[0] = 0.0
        nrm[0, d - 1] = 1.0
        nrm[1] = 0.0
        nrm[1, d - 1] = -1.0
        nrm[2, d - 1] = 0.0
        yield nodes.astype(np.int32), nrm


def _stiffness(gpu, V, modulus=cr.E):
    K = gpu.DeviceMatrix(V)
    K.assemble(lame=fo.lame(modulus, cr.NU))
    return K


# ------------------------------------------------------------------------------------------------ 1. the change of basis
def test_rotate_nodes_matches_the_host(gpu, data_dir):
    for si, (name, co, V) in enumerate(_spaces(gpu, data_dir)):
        d = co.shape[1]
        K0 = _csr(_stiffness(gpu, V))
        scale = np.abs(K0.data).max()
        for fi, (nodes, nrm) in enumerate(_frame_sets(co, 10 * si)):
            tag = (name, fi)
            frames = gpu.ContactFrames(V, nodes, nrm)
            H, sigma, unit = cr.frames(nrm)
            assert np.array_equal(frames.sigma, sigma) and np.abs(frames.normals - unit).max() <= 4 * EPS, tag
            K = _stiffness(gpu, V)
            K.rotate_nodes(frames)
            Kp = _csr(K)
            ref = cr.rotate_matrix(K0, nodes, H)
            assert np.array_equal(Kp.indptr, K0.indptr) and np.array_equal(Kp.indices, K0.indices), (tag, "pattern")
            err = abs(Kp - ref).max()
            sym = abs(Kp - Kp.T).max()
            print("%s / set %d: %d frames, max|K' - H K H| / max|K| = %.2e, asymmetry %.2e" % (name, fi, len(nodes), err / scale, sym / scale))
            assert err <= 1e-13 * scale, (tag, err / scale)
            assert sym <= 1e-13 * scale, (tag, sym / scale)
            # blocks with neither node framed: the same bits
            framed = np.zeros(len(co), dtype=bool)
            framed[nodes] = True
            rows = np.repeat(np.arange(K0.shape[0]), np.diff(K0.indptr))
            plain = ~framed[rows // d] & ~framed[K0.indices // d]
            assert plain.any() and (~plain).any(), tag
            assert np.array_equal(_bits(Kp.data[plain]), _bits(K0.data[plain])), (tag, "unframed blocks")
            assert np.abs(Kp.data[~plain] - K0.data[~plain]).max() > 1e-3 * scale, (tag, "the rotation changed nothing")
            # H is its own inverse
            K.rotate_nodes(frames)
            back = np.abs(_csr(K).data - K0.data).max()
            assert back <= 1e-13 * scale, (tag, back / scale)
            # the same call on the same values: the same bits
            K2 = _stiffness(gpu, V)
            K2.rotate_nodes(frames)
            assert np.array_equal(_bits(_csr(K2).data), _bits(Kp.data)), (tag, "bits")
            # vectors
            vh = np.random.default_rng(fi).standard_normal(V.n_local)
            v = gpu.DeviceVector(V.n_local, vh)
            v.rotate_nodes(frames)
            got = v.get()
            vref = cr.rotate_vector(vh, nodes, H)
            assert np.abs(got - vref).max() <= 1e-13 * np.abs(vh).max(), tag
            keep = np.repeat(~framed, d)
            assert np.array_equal(_bits(got[keep]), _bits(vh[keep])), tag
            # (H v)_k = sigma n . v
            nd = d * nodes.astype(np.int64) + d - 1
            ndotv = np.einsum("ai,ai->a", unit, vh.reshape(-1, d)[nodes])
            assert np.abs(got[nd] - sigma * ndotv).max() <= 1e-13 * np.abs(vh).max(), tag
            v2 = gpu.DeviceVector(V.n_local, vh)
            v2.rotate_nodes(frames)
            assert np.array_equal(_bits(v2.get()), _bits(got)), tag
            v.rotate_nodes(frames)
            assert np.abs(v.get() - vh).max() <= 1e-13 * np.abs(vh).max(), tag
            for h in (K, K2, v, v2, frames):
                h.close()


def test_frames_refuse_bad_input(gpu):
    mesh = gpu.DeviceMesh.box(2, 2, 2)
    V = gpu.DeviceSpace(mesh, 3, 1)
    ez = np.tile([0.0, 0.0, 1.0], (2, 1))
    with pytest.raises(gpu.BackendError, match="zero or non-finite normal"):
        gpu.ContactFrames(V, [1, 2], np.zeros((2, 3)))
    with pytest.raises(gpu.BackendError, match="strictly ascending"):
        gpu.ContactFrames(V, [2, 1], ez)
    with pytest.raises(gpu.BackendError, match="outside"):
        gpu.ContactFrames(V, [1, 27], ez)
    S = gpu.DeviceSpace(mesh, 1, 1)
    with pytest.raises(gpu.BackendError, match="vector CG1"):
        gpu.ContactFrames(S, [1, 2], np.ones((2, 1)))
    frames = gpu.ContactFrames(V, [1, 2], ez)
    A = gpu.DeviceMatrix(S)
    with pytest.raises(gpu.BackendError, match="not on the frames' space"):
        A.rotate_nodes(frames)
    with pytest.raises(gpu.BackendError, match="entries"):
        gpu.DeviceVector(5).rotate_nodes(frames)


# ------------------------------------------------------------------------------------------------ 2. the active-set update
def test_contact_update_matches_the_host(gpu, data_dir):
    """Unit modulus here: the bound of both lambda and the penetration is 1e-13 sum |K'_row| |u'|, and with E = 2e11 it would exceed
    every penetration of a displacement of 1e-3 - no flag of an inactive node could be checked."""
    for si, (name, co, V) in enumerate(_spaces(gpu, data_dir)):
        d = co.shape[1]
        for fi, (nodes, nrm) in enumerate(_frame_sets(co, 10 * si + 1)):
            tag = (name, fi)
            rng = np.random.default_rng(100 * si + fi)
            m = len(nodes)
            bilateral = np.zeros(m, dtype=bool)
            bilateral[rng.choice(m, size=max(1, m // 6), replace=False)] = True
            prior = rng.random(m) < 0.5
            frames = gpu.ContactFrames(V, nodes, nrm, np.zeros(m), bilateral, prior)
            K = _stiffness(gpu, V, modulus=1.0)
            K.rotate_nodes(frames)
            Kp = _csr(K)
            up = 1e-3 * rng.standard_normal(V.n_local)
            bp = Kp @ (1e-3 * rng.standard_normal(V.n_local))
            nd = d * nodes.astype(np.int64) + d - 1
            free = np.flatnonzero(~bilateral)
            # planted exact zeros.  lambda: an active node whose whole row meets u' = 0 and b' = 0 (it releases); penetration: an
            # inactive node with u'_normal = sigma g exactly (it stays out)
            i0, i1 = free[0], free[-1]
            assert i0 != i1, tag
            prior[i0], prior[i1] = True, False
            row = Kp[nd[i0]]
            up.reshape(-1, d)[np.unique(row.indices // d)] = 0.0
            bp[nd[i0]] = 0.0
            sigma = frames.sigma
            values = 1e-3 * rng.standard_normal(m)
            values[i1] = sigma[i1] * up[nd[i1]]
            frames.close()
            frames = gpu.ContactFrames(V, nodes, nrm, values, bilateral, prior)
            lam_h, pen_h, next_h, scale = cr.contact_update(Kp, up, bp, d, nodes, sigma, values, prior | bilateral, bilateral)
            bound = 1e-13 * (abs(Kp[nd]) @ np.abs(up))
            assert lam_h[i0] == 0.0 and pen_h[i1] == 0.0 and bound[i0] == 0.0, tag
            ud, bd = gpu.DeviceVector(V.n_local, up), gpu.DeviceVector(V.n_owned, bp[:V.n_owned])
            changed, n_active = gpu.contact_update(frames, K, ud, bd)
            act, lam, pen = frames.get()
            print("%s / set %d: %d nodes, max|lambda - host| / bound = %.2e" % (
                name, fi, m, (np.abs(lam - lam_h)[bound > 0] / bound[bound > 0]).max()))
            assert np.all(np.abs(lam - lam_h) <= bound), (tag, np.abs(lam - lam_h).max())
            assert np.all(np.abs(pen - pen_h) <= bound), (tag, np.abs(pen - pen_h).max())
            assert lam[i0] == 0.0 and pen[i1] == 0.0, tag
            was = prior | bilateral
            decisive = np.where(was, lam_h, pen_h)
            sure = (np.abs(decisive) > bound) | bilateral
            sure[[i0, i1]] = True                                   # exact zeros on both sides
            assert np.array_equal(act[sure], next_h[sure]), tag
            assert not act[i0] and not act[i1] and np.all(act[bilateral]), tag
            assert sure.all(), (tag, "a random value fell inside the rounding bound: change the seed")        # precondition of the counts
            assert changed == int((next_h != was).sum()) and n_active == int(next_h.sum()), (tag, changed, n_active)
            assert changed > 0 and 0 < n_active < m, tag
            # a second update from the new flags counts again from zero; the same call twice gives the same bits
            f2 = gpu.ContactFrames(V, nodes, nrm, values, bilateral, prior)
            c2 = gpu.contact_update(f2, K, ud, bd)
            a2, l2, p2 = f2.get()
            assert c2 == (changed, n_active) and np.array_equal(a2, act), tag
            assert np.array_equal(_bits(l2), _bits(lam)) and np.array_equal(_bits(p2), _bits(pen)), tag
            lam_3, pen_3, next_3, _ = cr.contact_update(Kp, up, bp, d, nodes, sigma, values, next_h, bilateral)
            c3 = gpu.contact_update(f2, K, ud, bd)
            assert c3 == (int((next_3 != next_h).sum()), int(next_3.sum())), (tag, c3)
            for h in (K, ud, bd, frames, f2):
                h.close()


# ------------------------------------------------------------------------------------------------ 3. patch test
def test_patch_test_between_oblique_sliding_faces(gpu):
    """The rotated box (0,0,0)-(2,1,0.5) between two sliding faces, z = 0 held (n . u = 0, the normal averaged from the facets) and
    z = 0.5 pushed in by delta (n . u = -delta, the normal given), its face x = 0 carrying the exact field: uniaxial stress along the
    box's z, u = R diag(nu' e, nu' e, -e) R^T x with e = delta / 0.5 and nu' = nu (free lateral faces).  The field is linear and P1
    reproduces it; the bound is the one of test_bimaterial_bar_is_exact (AMG-CG at krylov_relative_tolerance 1e-12): 1e-8 max|u|."""
    from fenicssolver_amd.fem import AutoSubDomain, Expression
    fx = cr.oblique()
    R = fx.R
    delta, h = 1e-3, 0.5
    e = delta / h
    M = R @ np.diag([cr.NU * e, cr.NU * e, -e]) @ R.T
    exact = fx.coords @ M.T
    field = Expression(tuple("%.17g*x[0] + %.17g*x[1] + %.17g*x[2]" % tuple(M[i]) for i in range(3)), degree=1)

    def local(x):
        return R.T @ np.asarray(x, dtype=np.float64)[:3]
    fx.dirichlet, fx.traction, fx.body = [], None, np.zeros(3)
    n_top = tuple(R @ np.array([0.0, 0.0, 1.0]))
    extra = {
        'held': {'boundary': AutoSubDomain(lambda x: abs(local(x)[0]) < 1e-9), 'boundary_id': 1, 'type': 'Dirichlet', 'value': field},
        'bottom': {'boundary': AutoSubDomain(lambda x: abs(local(x)[2]) < 1e-9), 'boundary_id': 2, 'type': 'sliding'},
        'top': {'boundary': AutoSubDomain(lambda x: abs(local(x)[2] - h) < 1e-9), 'boundary_id': 3, 'type': 'sliding', 'normal': n_top,
                'value': -delta}}
    solver = cr.make_solver(fx, with_contact=False, extra_bcs=extra)
    u = solver.solve().vector().get_local().reshape(-1, 3)
    err = np.abs(u - exact).max() / np.abs(exact).max()
    print("patch test: max|u - exact| / max|u| = %.3e" % err, solver.contact_stats)
    assert err <= 1e-8
    st = solver.contact_stats
    assert st['outer_iterations'] == 1 and st['amg_setups'] == 1 and st['active_history'] == [40]
    nodes, active, gaps = solver.contact_status()
    assert len(nodes) == 40 and active.all()
    assert np.abs(gaps).max() <= 16 * EPS * np.abs(u).max()
    # the supports carry the uniaxial stress E e: lambda_a = E e * (lumped area of a), i.e. the pressure E e at every node.  With
    # lambda - lambda_exact = n . (K (u - u_exact))_a the error is at most sqrt(3) |K|_inf max|u - u_exact|.
    _, lam = solver.contact_forces()
    p = solver.contact_pressure().vector().get_local()[nodes]
    K = fo.assemble_p1_elasticity(fx.coords, fx.cells, cr.E, cr.NU)
    tol = np.sqrt(3.0) * abs(K).sum(axis=1).max() * np.abs(u - exact).max() + 1e-12 * cr.E * e
    assert np.all(lam > 0.0)
    area = lam / p
    print("patch test: max|lambda - E e area| = %.3e, tolerance %.3e" % (np.abs(lam - cr.E * e * area).max(), tol))
    assert np.abs(lam - cr.E * e * area).max() <= tol
    bf = np.concatenate([fx.facets_on(lambda x: np.abs(x[:, 2]) < 1e-9), fx.facets_on(lambda x: np.abs(x[:, 2] - h) < 1e-9)])
    assert np.abs(area - cr.lumped_areas(fx.coords, bf)[nodes]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ 4. the fixtures
def _norm2_inverse(Kc):
    return 1.0 / np.linalg.svd(Kc.toarray(), compute_uv=False)[-1]


def _residual(Kc, bc, up):
    """b_c - K_c u' in extended precision, so that the evaluation adds nothing to the residuals it measures."""
    A = Kc.toarray().astype(np.longdouble)
    return np.asarray(bc.astype(np.longdouble) - A @ up.astype(np.longdouble), dtype=np.float64)


@pytest.mark.parametrize("name", list(cr.FIXTURES))
def test_fixture_through_the_solver(gpu, name):
    fx = cr.FIXTURES[name]()
    d = fx.dim
    ref = fx.reference()
    solver = cr.make_solver(fx)
    u = solver.solve().vector().get_local().copy()
    st = solver.contact_stats
    nodes, active, gaps = solver.contact_status()
    fnodes, lam = solver.contact_forces()
    print(name, st)
    # the active set is the reference's
    assert np.array_equal(nodes, ref["nodes"]) and np.array_equal(fnodes, nodes)
    assert np.array_equal(active, ref["active"]), (st['active_history'], ref["history"])
    # signs and margins: the fixture conditions with 1e-3, loosened only by the iterative solve
    assert 0 < active.sum() < len(active)
    assert np.all(lam[active] >= 1e-3 * lam.max()) and np.all(lam[~active] == 0.0)
    assert np.all(gaps[~active] >= 1e-3 * gaps.max())
    # distance to the reference: u - u_ref = K_c^-1 (r_ref - r_gpu) on the constrained system of the common active set
    H = ref["H"]
    up = cr.rotate_vector(u, nodes, H)
    Kc, bc = ref["Kc"], ref["bc"]
    r_gpu, r_ref = _residual(Kc, bc, up), _residual(Kc, bc, ref["up"])
    bound = _norm2_inverse(Kc) * (np.linalg.norm(r_gpu) + np.linalg.norm(r_ref))
    dist = np.linalg.norm(u - ref["u"])
    print("%s: |u - u_ref| = %.3e, bound %.3e, |r_gpu| = %.3e, |r_ref| = %.3e, |u| = %.3e" % (
        name, dist, bound, np.linalg.norm(r_gpu), np.linalg.norm(r_ref), np.linalg.norm(u)))
    assert dist <= bound
    # active nodes sit on the obstacle
    ndotu = np.einsum("ai,ai->a", ref["normals"], u.reshape(-1, d)[nodes])
    assert np.abs(ndotu - ref["gaps"])[active].max() <= 16 * EPS * np.abs(u).max()
    assert np.abs(gaps - (ref["gaps"] - ndotu)).max() <= 16 * EPS * np.abs(u).max()
    # the multipliers are the normal components of b - K u of the device's own u (the oracle's K and b: assembly and the row sums
    # round at 1e-16 of sum |K_row| |u|; 1e-12 leaves room for the length of the rows)
    kk = cr.kkt(ref["K"], ref["b"], d, u, nodes, ref["normals"], ref["gaps"], active, ref["dir_dofs"])
    assert np.abs(lam - kk["lambda"]).max() <= 1e-12 * (abs(ref["K"]) @ np.abs(u)).max()
    # the pressure integrates to the total force over the marked facets
    p = solver.contact_pressure().vector().get_local()
    bf = fx.facets_on(fx.on_contact)
    integral = (cr.facet_measures(fx.coords, bf)[:, None] * p[bf] / bf.shape[1]).sum()
    assert abs(integral - lam.sum()) <= 1e-12 * lam.sum()
    assert np.all(p[np.setdiff1d(np.arange(len(p)), nodes[active])] == 0.0)
    if name == "strip":
        # equilibrium along z: only the obstacle holds the strip up, so sum lambda = weight - lift, less the z residual of the free dofs
        load = 3.0 * cr.BODY - cr.STRIP_LIFT
        slack = np.sqrt(len(u)) * np.linalg.norm(r_gpu) + 1e-12 * (abs(ref["K"]) @ np.abs(u)).sum()
        print("strip: sum lambda = %.9e, load %.9e, slack %.3e" % (lam.sum(), load, slack))
        assert abs(lam.sum() - load) <= slack
        assert abs(lam.sum() - load) <= 1e-7 * load
    # the statistics tell the same story
    assert st['active_history'][0] == ref["history"][0] == len(nodes) and st['active_history'][-1] == int(active.sum())
    assert st['outer_iterations'] == len(st['active_history']) == len(st['cg_iterations'])
    assert st['amg_setups'] == (st['outer_iterations'] if d == 3 else 0)
    for key in ('copy_dirichlet_ms', 'amg_setup_ms', 'cg_ms', 'update_ms'):
        assert len(st[key]) == st['outer_iterations'] and all(t >= 0.0 for t in st[key])
    # a second run gives the same bits
    again = cr.make_solver(fx)
    u2 = again.solve().vector().get_local()
    assert np.array_equal(_bits(u2), _bits(u))
    assert np.array_equal(_bits(again.contact_forces()[1]), _bits(lam))


# ------------------------------------------------------------------------------------------------ 5. nothing touches
def test_a_gap_too_large_to_close_changes_nothing(gpu):
    fx = cr.oblique()
    solver = cr.make_solver(fx, contact_settings={'initial_active': 'none'}, gap_scale=1e6)
    u = solver.solve().vector().get_local().copy()
    st = solver.contact_stats
    assert st['outer_iterations'] == 1 and st['active_history'] == [0] and st['amg_setups'] == 1
    nodes, active, gaps = solver.contact_status()
    assert not active.any() and np.all(gaps > 0.0) and np.all(solver.contact_forces()[1] == 0.0)
    plain = cr.make_solver(fx, with_contact=False)
    u0 = plain.solve().vector().get_local()
    K, b, dofs, vals, _, _, _ = fx.system()
    Kc, bc = fo.apply_dirichlet(K, b, dofs, vals, True)
    r1, r0 = _residual(Kc, bc, u), _residual(Kc, bc, u0)
    bound = _norm2_inverse(Kc) * (np.linalg.norm(r1) + np.linalg.norm(r0))
    dist = np.linalg.norm(u - u0)
    print("no contact: |u - u_plain| = %.3e, bound %.3e, |u| = %.3e" % (dist, bound, np.linalg.norm(u0)))
    assert np.linalg.norm(u0) > 0.0 and dist <= bound


# ------------------------------------------------------------------------------------------------ 6. an early stop
def test_max_iterations_names_the_history(gpu):
    from fenicssolver_amd.SolverBase import SolverError
    solver = cr.make_solver(cr.punch(), contact_settings={'max_iterations': 1})
    with pytest.raises(SolverError, match=r"max_iterations = 1 \(active counts \[81, 9\]\)"):
        solver.solve()
