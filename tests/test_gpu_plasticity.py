"""PlasticitySolver and fs_assemble_plasticity on the MI355X: the tangent without yielding against the linear operator bit for bit,
the kernels against the numpy reference (tests/plasticity_reference.py) on a mixed elastic / yielded state, the uniaxial closed
form, the solver against the reference Newton step by step, the history discipline and von_Mises() after yielding."""
import copy
import os
from collections import OrderedDict

import numpy as np
import pytest
import scipy.sparse as sps

import plasticity_reference as pr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E_, NU_ = 200.0, 0.3
MU_, LM_ = E_ / (2 * (1 + NU_)), E_ * NU_ / ((1 + NU_) * (1 - 2 * NU_))

# Measured on the MI355X (this file: the tests print every figure before they assert), and the bounds derived from them: 10 x the
# measured GPU-minus-reference difference, since the error the stopping tests leave belongs to the mesh family, not to one mesh.
# Uniaxial closed form, Newton and Krylov at their defaults (relative 1e-9 / 1e-8): largest difference relative to sigma_y (stress) and to
# the yield strain (strains, p) 3.5e-9 on the 4 x 3 x 3 box (third step); the 6 x 5 x 4 box gives 8.4e-9.
UNIAXIAL_MEASURED = 3.5e-9
UNIAXIAL_TOL = 10 * UNIAXIAL_MEASURED
# Solver against the reference Newton, Krylov tolerance 1e-12: largest relative difference of u and p over all steps and the four
# parametrisations 1.75e-9 (p, plane strain, H = E/10, last loading step); u alone: 7.7e-11.
SOLVER_MEASURED = 1.75e-9
SOLVER_TOL = 10 * SOLVER_MEASURED


def _device(mesh):
    from fenicssolver_amd.fem import VectorFunctionSpace
    from fenicssolver_amd import backend
    backend.init()
    V = VectorFunctionSpace(mesh, "Lagrange", 1)
    return V, V.device()


def _csr(A):
    rp, ci, va, (nr, nc) = A.to_csr()
    return sps.csr_matrix((va, ci, rp), shape=(nr, nc))


def _box(n=(4, 3, 3), p1=(1.0, 0.8, 0.6)):
    from fenicssolver_amd.fem import BoxMesh, Point
    return BoxMesh(Point(0, 0, 0), Point(*p1), *n)


def _rect(n=(6, 5), p1=(1.0, 0.7)):
    from fenicssolver_amd.fem import RectangleMesh, Point
    return RectangleMesh(Point(0, 0), Point(*p1), *n)


def _smooth_u(co, d, amp):
    x = co[:, :d]
    u = np.stack([amp * np.sin(1.3 * x[:, 0] + 0.7 * x[:, 1]) + 0.3 * amp * x[:, 1] ** 2,
                  amp * np.cos(0.9 * x[:, 0] - 1.1 * x[:, 1])] + ([amp * x[:, 0] * x[:, 2] + 0.5 * amp * np.sin(2 * x[:, 2])] if d == 3 else []),
                 axis=1)
    return u.ravel()


def mixed_state(d):
    """A smooth displacement with strains around the yield strain, a random admissible committed history and a material that varies
    from cell to cell: (mesh, u, eps_p [nc,3,3], p [nc], material [nc,4])."""
    mesh = _box() if d == 3 else _rect()
    nc = mesh.num_cells()
    rng = np.random.default_rng(40 + d)
    u = _smooth_u(mesh.coordinates(), d, 1.7e-3 if d == 3 else 2.5e-3)
    b = 4e-4 * rng.standard_normal((nc, 3, 3))
    ep = 0.5 * (b + np.transpose(b, (0, 2, 1)))
    if d == 2:
        ep[:, :2, 2] = ep[:, 2, :2] = 0.0
    ep -= np.trace(ep, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3.0
    p = 1e-3 * rng.random(nc)
    mat = np.stack([MU_ * (1 + 0.2 * rng.random(nc)), LM_ * (1 + 0.2 * rng.random(nc)), 0.4 * (1 + 0.2 * rng.random(nc)),
                    20.0 * rng.random(nc)], axis=1)
    return mesh, u, ep, p, mat


# ---- 1. no yielding: the linear operator, bit for bit ---------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("cellwise", [False, True])
def test_tangent_without_yielding_is_the_linear_operator_bit_for_bit(d, cellwise):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    uh = _smooth_u(mesh.coordinates(), d, 0.05)
    if cellwise:
        rng = np.random.default_rng(1)
        mu, lm = 3.1 * (1 + rng.random(nc)), 4.7 * (1 + rng.random(nc))
        lame = ("cell", np.stack([mu, lm], axis=1))
        material = ("cell", np.stack([mu, lm, np.full(nc, 1e3), 2.0 * rng.random(nc)], axis=1))
    else:
        mu, lm = 3.1, 4.7
        lame, material = (mu, lm), (mu, lm, 1e3, 0.5)
    # the yield stress lies above every trial q of the reference
    st = pr.assemble(mesh.coordinates()[:, :d], mesh.cells(), uh, np.zeros((nc, 3, 3)), np.zeros(nc), mu, lm, 1e3, 0.5, tangent=False)
    assert st["fy"].max() < -1.0
    A = backend.DeviceMatrix(dV)
    A.assemble(lame=lame)
    hist = backend.PlasticHistory(dV)
    K = backend.DeviceMatrix(dV)
    r = backend.DeviceVector(dV.n_owned)
    info = backend.assemble_plasticity(dV, backend.DeviceVector(dV.n_local, uh), hist, material, K=K, r=r)
    assert info == {"n_yielded": 0, "n_nonfinite": 0, "first_nonfinite_cell": -1}
    a, k = A.to_csr(), K.to_csr()
    assert np.array_equal(a[0], k[0]) and np.array_equal(a[1], k[1])
    assert np.array_equal(a[2], k[2])
    # the history is untouched: committed and trial state are still zero
    for trial in (False, True):
        ep, p, _ = hist.get(trial=trial)
        assert not ep.any() and not p.any()
    # and the force is the linear operator's product, to rounding
    Au = backend.DeviceVector(dV.n_owned)
    A.spmv(backend.DeviceVector(dV.n_local, uh), Au)
    assert np.abs(r.get() - Au.get()).max() <= 1e-12 * np.abs(Au.get()).max()


def _cantilever_case(d, cls_settings=None, H=20.0, sy=0.5, loads=None, steps=None, n=None, krylov=1e-12, bimaterial=True):
    """3-D: a box clamped at x = 0 under an end traction (0, 0, -T) on x = L, the yield stress 0.5 for x < L/2 and 0.8 beyond
    (bimaterial).  2-D (plane strain): a rectangle fixed at y = 0 under the traction (0, -T) on the part 0.5 <= x <= 1.5 of its top edge.
    loads: T per step."""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, MeshFunction, near
    from fenicssolver_amd import SolverBase as SB
    bcs = OrderedDict()
    if d == 3:
        n = n or (8, 3, 3)
        mesh = BoxMesh(Point(0, 0, 0), Point(4, 1, 1), *n)
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0, 0.0, 0.0))}
        val = [Constant((0.0, 0.0, -T)) for T in loads]
        bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 4.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': val if len(val) > 1 else val[0]}
    else:
        n = n or (16, 8)
        mesh = RectangleMesh(Point(0, 0), Point(2, 1), *n)
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[1], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0, 0.0))}
        val = [Constant((0.0, -T)) for T in loads]
        bcs["punch"] = {'boundary': AutoSubDomain(lambda x: near(x[1], 1.0) and 0.5 - 1e-12 <= x[0] <= 1.5 + 1e-12), 'boundary_id': 2,
                        'type': 'stress', 'value': val if len(val) > 1 else val[0]}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': 7800, 'thermal_expansion_coefficient': 0.0,
                     'yield_stress': sy, 'hardening_modulus': H}
    if d == 3 and bimaterial:
        s['material']['yield_stress'] = {'weak': {'subdomain_id': 1, 'value': 0.5}, 'strong': {'subdomain_id': 2, 'value': 0.8}}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': krylov}
    if len(loads) > 1:
        s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 1.0,
                                                      'ending_time': float(len(loads))}
    sub = None
    if d == 3 and bimaterial:
        sub = MeshFunction("size_t", mesh, 3)
        sub.array()[:] = np.where(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1)[:, 0] < 2.0, 1, 2)
    return s, mesh, sub


def _facet_load(mesh, d, pred, g):
    """int g . v ds over the exterior facets whose vertices all satisfy pred: |facet| / d per vertex"""
    co = mesh.coordinates()[:, :d]
    fac = mesh.facets()[mesh.exterior_facets()].astype(np.int64)
    sel = fac[np.all(pred(co[fac]), axis=1)]
    q = co[sel]
    size = np.linalg.norm(q[:, 1] - q[:, 0], axis=1) if d == 2 else 0.5 * np.linalg.norm(np.cross(q[:, 1] - q[:, 0], q[:, 2] - q[:, 0]), axis=1)
    f = np.zeros(co.size)
    for k in range(d):
        np.add.at(f, (sel * d + k).ravel(), np.repeat(g[k] * size / d, d))
    return f


def _reference_steps(mesh, d, sub, H, loads, rtol=1e-9, sy=0.5):
    co = mesh.coordinates()[:, :d]
    if d == 3:
        unit = _facet_load(mesh, 3, lambda x: np.abs(x[..., 0] - 4.0) < 1e-12, (0.0, 0.0, -1.0))
        dofs = (np.nonzero(np.abs(co[:, 0]) < 1e-12)[0][:, None] * 3 + np.arange(3)).ravel()
        syv = np.where(sub.array() == 1, 0.5, 0.8) if sub is not None else sy
    else:
        unit = _facet_load(mesh, 2, lambda x: (np.abs(x[..., 1] - 1.0) < 1e-12) & (x[..., 0] > 0.5 - 1e-12) & (x[..., 0] < 1.5 + 1e-12), (0.0, -1.0))
        dofs = (np.nonzero(np.abs(co[:, 1]) < 1e-12)[0][:, None] * 2 + np.arange(2)).ravel()
        syv = sy
    steps = pr.solve_steps(co, mesh.cells(), (MU_, LM_, syv, H), [(T * unit, dofs, np.zeros(len(dofs))) for T in loads], rtol=rtol)
    return steps, np.broadcast_to(syv, (mesh.num_cells(),))


@pytest.mark.parametrize("d", [3, 2])
def test_solver_without_yielding_returns_the_linear_solution(d):
    """A load far below yield: one Newton step with the linear operator.  Both solves stop at a Krylov residual of 1e-12 relative,
    so the two fields agree to cond(K) x 1e-12; these meshes have cond(K) < 1e4."""
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    T = 0.01 if d == 3 else 0.1
    s, mesh, sub = _cantilever_case(d, loads=[T])
    ps = PlasticitySolver(copy.deepcopy(s))
    ps.subdomains = sub
    u = ps.solve().vector()._values().copy()
    s['material']['yield_stress'] = 1.0
    lin = LinearElasticitySolver(s)
    lin.reference_load_sign = False
    ul = lin.solve().vector()._values()
    assert ps.yielded_cells == [0] and not ps.cumulative_plastic_strain().any() and not ps.plastic_strain().any()
    assert np.abs(ul).max() > 1e-4
    assert np.abs(u - ul).max() <= 1e-8 * np.abs(ul).max()


# ---- 2. the kernels against the reference on a mixed state ----------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
def test_kernels_match_the_host_reference_and_are_deterministic(d):
    from fenicssolver_amd import backend
    mesh, uh, ep, p, mat = mixed_state(d)
    V, dV = _device(mesh)
    ref = pr.assemble(mesh.coordinates()[:, :d], mesh.cells(), uh, ep, p, *mat.T)
    fy = ref["fy"]
    # the branch of a cell within rounding of f = 0 is undetermined: the inputs keep every cell away from it, with both branches present
    assert np.abs(fy / mat[:, 2]).min() > 1e-6
    assert (fy > 0).mean() >= 0.25 and (fy < 0).mean() >= 0.25
    hist = backend.PlasticHistory(dV)
    hist.set(pr.pack(ep, d), p)
    u = backend.DeviceVector(dV.n_local, uh)
    outs = []
    for _ in range(2):
        K = backend.DeviceMatrix(dV)
        r = backend.DeviceVector(dV.n_owned)
        info = backend.assemble_plasticity(dV, u, hist, ("cell", mat), K=K, r=r)
        ept, pt, sgt = hist.get(trial=True)
        outs.append((K.to_csr()[2], r.get(), ept, pt, sgt))
        Kd = _csr(K)
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)
    assert info["n_yielded"] == int((fy > 0).sum()) and info["n_nonfinite"] == 0
    errs = {"K": abs(Kd - ref["K"]).max() / abs(ref["K"]).max(),
            "r": np.abs(outs[0][1] - ref["f"]).max() / np.abs(ref["f"]).max(),
            "eps_p": np.abs(outs[0][2] - pr.pack(ref["ep"], d)).max() / np.abs(ref["ep"]).max(),
            "p": np.abs(outs[0][3] - ref["p"]).max() / np.abs(ref["p"]).max(),
            "sigma": np.abs(outs[0][4] - pr.pack(ref["sigma"], d)).max() / np.abs(ref["sigma"]).max()}
    print("\nkernels against the reference, d = %d: %s" % (d, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) <= 1e-12
    # the committed state is what was set, bit for bit
    epc, pc, _ = hist.get()
    assert np.array_equal(epc, pr.pack(ep, d)) and np.array_equal(pc, p)


# ---- 2b. add=True adds to what the target holds ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
def test_add_accumulates_onto_the_target_bit_for_bit(d):
    """Tangent and force with add=True equal y + x bit for bit (one fp64 addition per entry): y the target's content (the linear
    operator in the matrix, known values in the vector), x the result with add=False.  3 x 3 x 4 box: 216 cells, 80 nodes (a partial
    second slice); 5 x 4 square: 40 cells, 30 nodes."""
    from fenicssolver_amd import backend
    mesh = _box((3, 3, 4)) if d == 3 else _rect((5, 4))
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    assert (nc, mesh.num_vertices()) == ((216, 80) if d == 3 else (40, 30))
    rng = np.random.default_rng(60 + d)
    uh = _smooth_u(mesh.coordinates(), d, 1.7e-3 if d == 3 else 2.5e-3)
    mat = np.stack([MU_ * (1 + 0.2 * rng.random(nc)), LM_ * (1 + 0.2 * rng.random(nc)), 0.2 * (1 + 0.2 * rng.random(nc)),
                    20.0 * rng.random(nc)], axis=1)
    hist = backend.PlasticHistory(dV)
    u = backend.DeviceVector(dV.n_local, uh)
    K, r = backend.DeviceMatrix(dV), backend.DeviceVector(dV.n_owned)
    info = backend.assemble_plasticity(dV, u, hist, ("cell", mat), K=K, r=r)
    assert 0 < info["n_yielded"] < nc                      # the rank-one part of the tangent takes part
    xk, xr = K.to_csr()[2], r.get()
    y = 0.37 + rng.standard_normal(dV.n_owned)
    Ka, ra = backend.DeviceMatrix(dV), backend.DeviceVector(dV.n_owned, y)
    Ka.assemble(lame=(MU_, LM_))
    yk = Ka.to_csr()[2]
    backend.assemble_plasticity(dV, u, hist, ("cell", mat), K=Ka, r=ra, add=True)
    assert np.array_equal(Ka.to_csr()[2], yk + xk)
    assert np.array_equal(ra.get(), y + xr)


# ---- 3. the uniaxial closed form ------------------------------------------------------------------------------------------------
def _uniaxial_case(d, path, H, n=None, L=1.0):
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    mesh = BoxMesh(Point(0, 0, 0), Point(L, L, L), *(n or (4, 3, 3))) if d == 3 else RectangleMesh(Point(0, 0), Point(L, L), *(n or (6, 5)))
    bcs = OrderedDict()

    def plane(k, v):
        return AutoSubDomain(lambda x: near(x[k], v))
    for k, name in enumerate("xyz"[:d]):
        val = [None] * d
        val[k] = Constant(0.0)
        bcs["roller_" + name] = {'boundary': plane(k, 0.0), 'boundary_id': k + 1, 'type': 'Dirichlet', 'value': tuple(val)}
    val = [None] * d
    val[0] = [float(e) * L for e in path]
    bcs["pull"] = {'boundary': plane(0, L), 'boundary_id': 9, 'type': 'Dirichlet', 'value': tuple(val)}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': 7800, 'thermal_expansion_coefficient': 0.0,
                     'yield_stress': 0.5, 'hardening_modulus': H}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 1.0, 'ending_time': float(len(path))}
    return s, mesh


@pytest.mark.parametrize("n", [(4, 3, 3), (6, 5, 4)])
def test_uniaxial_closed_form_in_every_cell_and_step(n):
    """Roller planes on x = 0, y = 0, z = 0 and a prescribed u_x on x = L: elastic, past yield, further loading, partial unloading.
    The state is homogeneous, so CG1 carries it exactly and every cell follows the 1-D closed form."""
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    H, sy = 20.0, 0.5
    ey = sy / E_
    path = [0.5 * ey, 1.5 * ey, 3.0 * ey, 4.0 * ey, 3.5 * ey]
    s, mesh = _uniaxial_case(3, path, H, n)
    solver = PlasticitySolver(s)
    exact = pr.uniaxial(path, E_, NU_, sy, H)
    seen = []
    solve_form = solver.solve_form

    def checked(F, u_, bcs):
        out = solve_form(F, u_, bcs)
        k = len(seen)
        sxx, p, lat = exact[k]
        sg, pc = solver.stress(), solver.cumulative_plastic_strain()
        eps = pr.strains(mesh.coordinates(), mesh.cells(), out.vector()._values())[0]
        other = sg.copy()
        other[:, 0] = 0.0
        seen.append(max(np.abs(sg[:, 0] - sxx).max() / sy, np.abs(other).max() / sy, np.abs(pc - p).max() / ey,
                        np.abs(eps[:, 1, 1] - lat).max() / ey, np.abs(eps[:, 2, 2] - lat).max() / ey,
                        np.abs(eps[:, 0, 0] - path[k]).max() / ey))
        return out
    solver.solve_form = checked
    solver.solve()
    Et = E_ * H / (E_ + H)
    assert abs(exact[0][0] - E_ * path[0]) < 1e-15 and abs(exact[3][0] - (sy + Et * (path[3] - ey))) < 1e-15
    assert exact[4][1] == exact[3][1] and abs(exact[4][0] - (exact[3][0] - E_ * 0.5 * ey)) < 1e-15        # elastic unloading, p frozen
    assert solver.yielded_cells == [0, mesh.num_cells(), mesh.num_cells(), mesh.num_cells(), 0]
    print("\nuniaxial closed form, mesh %s: largest relative difference per step %s, Newton iterations %s" % (
        n, ["%.2e" % x for x in seen], solver.newton_iterations_per_step))
    assert max(seen) <= UNIAXIAL_TOL


# ---- 4. the solver against the reference Newton ---------------------------------------------------------------------------------
LOADS = {3: [0.03, 0.045, 0.055, 0.06, 0.045], 2: [0.6, 0.64, 0.68, 0.72, 0.75, 0.6]}      # the last step unloads partially


@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("H", [0.0, E_ / 10])
def test_solver_matches_the_reference_newton_step_by_step(d, H):
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    loads = LOADS[d]
    s, mesh, sub = _cantilever_case(d, H=H, loads=loads)
    ref, syv = _reference_steps(mesh, d, sub, H, loads)
    last = ref[-2]                                   # the last loading step
    assert 0.10 <= (last["fy"] > 0).mean() <= 0.90
    assert all(st["iterations"] <= 8 for st in ref)
    solver = PlasticitySolver(s)
    solver.subdomains = sub
    seen = []
    solve_form = solver.solve_form

    def checked(F, u_, bcs):
        k = len(seen)
        ep_before = solver.history.get()[1].copy() if solver.history is not None else np.zeros(mesh.num_cells())
        out = solve_form(F, u_, bcs)
        st = ref[k]
        pc = solver.cumulative_plastic_strain()
        near = np.abs(st["fy"]) < 1e-6 * syv
        assert near.mean() <= 0.01
        yielded_dev = pc > ep_before                  # cells whose p grew in this step
        assert np.array_equal(yielded_dev[~near], (st["fy"] > 0)[~near])
        assert solver.yielded_cells[-1] == int(yielded_dev.sum())
        assert abs(solver.newton_iterations - st["iterations"]) <= 1 and solver.newton_iterations <= 8
        u = out.vector()._values()
        seen.append((np.abs(u - st["u"]).max() / np.abs(st["u"]).max(), np.abs(pc - st["p"]).max() / max(np.abs(ref[-1]["p"]).max(), 1e-300)))
        return out
    solver.solve_form = checked
    solver.solve()
    assert len(seen) == len(loads)
    print("\nsolver against the reference Newton, d = %d, H = %g: relative difference (u, p) per step %s, Newton iterations %s, yielded %s" % (
        d, H, [("%.2e" % a, "%.2e" % b) for a, b in seen], solver.newton_iterations_per_step, solver.yielded_cells))
    assert max(max(a, b) for a, b in seen) <= SOLVER_TOL


# ---- 5. history discipline --------------------------------------------------------------------------------------------------------
def test_rejected_trials_and_failed_steps_leave_the_committed_history_untouched():
    from fenicssolver_amd import backend
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    # (a) evaluations - what the Newton driver does with a trial iterate, one with a non-finite entry included - change the trial state only
    mesh, uh, ep, p, mat = mixed_state(3)
    V, dV = _device(mesh)
    hist = backend.PlasticHistory(dV)
    hist.set(pr.pack(ep, 3), p)
    before = hist.get()
    bad = uh.copy()
    bad[7] = np.nan
    for x, nonfinite in ((uh, False), (bad, True), (0.5 * uh, False)):
        info = backend.assemble_plasticity(dV, backend.DeviceVector(dV.n_local, x), hist, ("cell", mat), K=backend.DeviceMatrix(dV),
                                           r=backend.DeviceVector(dV.n_owned))
        assert (info["n_nonfinite"] > 0) == nonfinite
        after = hist.get()
        assert all(np.array_equal(a, b) for a, b in zip(before, after))
    assert not np.array_equal(hist.get(trial=True)[1], before[1])
    # (b) a load step that does not converge (one Newton iteration allowed on a yielding step) raises and commits nothing
    s2, mesh, sub = _cantilever_case(3, loads=LOADS[3][:4])
    solver = PlasticitySolver(s2)
    solver.subdomains = sub
    solve_form = solver.solve_form
    state = {}

    def limited(F, u_, bcs):
        if len(solver.yielded_cells) == 3:
            state["before"] = solver.history.get()
            solver.solver_settings['solver_parameters']['newton_solver'] = {'maximum_iterations': 1}
        return solve_form(F, u_, bcs)
    solver.solve_form = limited
    with pytest.raises(SolverError, match="did not converge in 1 iterations"):
        solver.solve()
    after = solver.history.get()
    assert state["before"][1].max() > 0.0
    assert all(np.array_equal(a, b) for a, b in zip(state["before"], after))


def test_two_solves_give_the_same_bits():
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    out = []
    for _ in range(2):
        s, mesh, sub = _cantilever_case(3, loads=LOADS[3])
        solver = PlasticitySolver(s)
        solver.subdomains = sub
        u = solver.solve().vector()._values().copy()
        out.append((u, solver.cumulative_plastic_strain(), solver.plastic_strain(), solver.stress()))
    assert out[0][1].max() > 0.0
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    # the same solver again starts from the virgin state
    u3 = solver.solve().vector()._values()
    assert np.array_equal(u3, out[0][0]) and np.array_equal(solver.cumulative_plastic_strain(), out[0][1])


XML_LOADS = [0.02, 0.04, 0.055, 0.065, 0.05]


def _xml_case(monkeypatch, renumber):
    """tests/golden/data/mesh.xml (a 10 x 5 x 20 block) with its region file, uploaded in file order or in locality order: clamped at
    z = 0, sheared at z = 20, the yield stress by region."""
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.fem import Mesh, MeshFunction, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    monkeypatch.setenv("FS_RENUMBER", "1" if renumber else "0")
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
    mesh = Mesh(os.path.join(data, "mesh.xml"))
    sub = MeshFunction("size_t", mesh, os.path.join(data, "mesh_physical_region.xml"))
    ids = np.unique(np.asarray(sub.array(), dtype=np.int64))
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'value': Constant((0.0, 0.0, 0.0))}
    bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 20.0)), 'boundary_id': 2, 'type': 'stress',
                  'value': [Constant((T, 0.0, 0.0)) for T in XML_LOADS]}
    s = copy.deepcopy(SB.default_case_settings)
    sy = {int(i): 0.5 + 0.05 * k for k, i in enumerate(ids)}
    s['material'] = {'name': 'steel', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': 7800, 'thermal_expansion_coefficient': 0.0,
                     'yield_stress': {'r%d' % i: {'subdomain_id': i, 'value': v} for i, v in sy.items()}, 'hardening_modulus': 20.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': 1.0, 'ending_time': float(len(XML_LOADS))}
    solver = PlasticitySolver(s)
    solver.subdomains = sub
    syv = np.array([sy[int(i)] for i in np.asarray(sub.array(), dtype=np.int64)])
    return solver, mesh, syv


def xml_reference(mesh, syv):
    co = mesh.coordinates()
    unit = _facet_load(mesh, 3, lambda x: np.abs(x[..., 2] - 20.0) < 1e-9, (1.0, 0.0, 0.0))
    dofs = (np.nonzero(np.abs(co[:, 2]) < 1e-9)[0][:, None] * 3 + np.arange(3)).ravel()
    return pr.solve_steps(co, mesh.cells(), (MU_, LM_, syv, 20.0), [(T * unit, dofs, np.zeros(len(dofs))) for T in XML_LOADS])


@pytest.mark.parametrize("renumber", [False, True])
def test_accessors_use_the_callers_cell_numbering_on_a_file_mesh(monkeypatch, renumber):
    solver, mesh, syv = _xml_case(monkeypatch, renumber)
    u = solver.solve().vector()._values()
    assert (solver.function_space.localizer() is not None) == renumber
    ref = xml_reference(mesh, syv)[-1]
    assert (ref["p"] > 0).mean() > 0.02 and (ref["p"] == 0).mean() > 0.02
    p, ep, sg = solver.cumulative_plastic_strain(), solver.plastic_strain(), solver.stress()
    # a permutation of the cells would put p > 0 where the reference has none: the comparison is cell by cell, in the file's numbering
    assert np.abs(p - ref["p"]).max() <= SOLVER_TOL * ref["p"].max()
    assert np.abs(ep - pr.pack(ref["ep"], 3)).max() <= SOLVER_TOL * np.abs(ref["ep"]).max()
    assert np.abs(sg - pr.pack(ref["sigma"], 3)).max() <= SOLVER_TOL * np.abs(ref["sigma"]).max()
    assert np.abs(u - ref["u"]).max() <= SOLVER_TOL * np.abs(ref["u"]).max()


def test_accessors_on_a_box_mesh_match_the_reference_cell_by_cell():
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    s, mesh, sub = _cantilever_case(3, loads=LOADS[3])
    solver = PlasticitySolver(s)
    solver.subdomains = sub
    solver.solve()
    ref, _ = _reference_steps(mesh, 3, sub, 20.0, LOADS[3])
    assert np.abs(solver.cumulative_plastic_strain() - ref[-1]["p"]).max() <= SOLVER_TOL * ref[-1]["p"].max()
    assert np.abs(solver.stress() - pr.pack(ref[-1]["sigma"], 3)).max() <= SOLVER_TOL * np.abs(ref[-1]["sigma"]).max()


# ---- 6. von_Mises() after yielding ------------------------------------------------------------------------------------------------
def _p1_projection(mesh, d, cell_values):
    """the consistent L2 projection of a cell-wise field onto CG1, on the host"""
    import scipy.sparse.linalg as spla
    ce = mesh.cells().astype(np.int64)
    _, V = pr.gradients(mesh.coordinates(), ce)
    nv = mesh.num_vertices()
    b = np.bincount(ce.ravel(), weights=np.repeat(cell_values * V / (d + 1), d + 1), minlength=nv)
    Me = V[:, None, None] * (np.ones((d + 1, d + 1)) + np.eye(d + 1))[None] / ((d + 1) * (d + 2))
    M = sps.csr_matrix((Me.ravel(), (np.repeat(ce, d + 1, axis=1).ravel(), np.tile(ce, (1, d + 1)).ravel())), shape=(nv, nv))
    return spla.spsolve(M.tocsc(), b)


@pytest.mark.parametrize("d", [3, 2])
def test_von_mises_projects_the_returned_stress(d):
    from fenicssolver_amd.PlasticitySolver import PlasticitySolver
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    H = 20.0
    loads = LOADS[d][:-1]                               # stop at the last loading step: yielded cells are on the yield surface
    s, mesh, sub = _cantilever_case(d, H=H, loads=loads)
    solver = PlasticitySolver(s)
    solver.subdomains = sub
    u = solver.solve()
    vm = solver.von_Mises(u).vector()._values()
    ref, syv = _reference_steps(mesh, d, sub, H, loads)
    vm_cells = pr.von_mises(ref[-1]["sigma"])
    p = solver.cumulative_plastic_strain()
    assert p.max() > 0.0
    # every cell value obeys q <= sigma_y + H p; the projection overshoots by what the same projection of the reference's cell values does
    host = _p1_projection(mesh, d, vm_cells)
    overshoot = max(host.max() - vm_cells.max(), 0.0)
    assert np.abs(solver.von_Mises_cells() - vm_cells).max() <= SOLVER_TOL * vm_cells.max()
    assert np.abs(vm - host).max() <= 1e-9 * host.max() + SOLVER_TOL * vm_cells.max()
    assert vm.max() <= (syv + H * p).max() + overshoot + 1e-9 * vm_cells.max()
    # the inherited method reports the elastic stress of u, which exceeds the yield surface where p > 0
    elastic = LinearElasticitySolver.von_Mises(solver, u).vector()._values()
    ce = mesh.cells().astype(np.int64)
    touched = np.unique(ce[p > 0])
    assert np.abs(elastic[touched] - vm[touched]).max() > 1e-3 * vm.max()
    assert elastic.max() > vm.max()
