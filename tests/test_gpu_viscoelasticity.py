"""ViscoelasticitySolver and fs_assemble_viscoelastic on the MI355X: the kernels against the numpy reference
(tests/viscoelastic_reference.py), the empty series, the semigroup property on the device, the shear-relaxation closed form, the
solver against the reference marcher step by step, the instantaneous and long-term limits, equilibrium of the stored stress and the
history discipline."""
import copy
import functools
import os
from collections import OrderedDict

import numpy as np
import pytest

import viscoelastic_reference as vr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E_, NU_ = 200.0, 0.3
MU_, LM_ = E_ / (2 * (1 + NU_)), E_ * NU_ / ((1 + NU_) * (1 - 2 * NU_))
G2, TAU2 = np.array([0.3, 0.2]), np.array([0.5, 5.0])        # two terms, relaxation times a decade apart

KERNEL_TOL = 1e-12          # set by the issue: update and history load against the reference, relative to the largest entry
SEMIGROUP_TOL = 1e-13       # set by the issue: two half steps against one step on the device

# Measured on the MI355X (this file: the tests print every figure before they assert), every solver test with the Krylov tolerance at
# 1e-12 ('krylov_relative_tolerance'), and the bounds derived from them: 10 x the measured GPU-minus-reference difference, since the
# residue the stopping test leaves belongs to the mesh family, not to one mesh.
# Shear relaxation closed form: largest |sigma - closed form| / (G0 gamma0) over cells and steps 1.03e-11 on the 4 x 3 x 3 box (one- and
# two-step ramp alike), 1.80e-11 on the 6 x 5 x 4 box (last step) - the homogeneous state is a few hundred free nodes solved to 1e-12.
RELAX_MEASURED = 1.80e-11
RELAX_TOL = 10 * RELAX_MEASURED
# Solver against the reference marcher (sparse direct solve per step), cantilever 8 x 3 x 3 and rectangle 16 x 8, per-region series, seven
# steps: largest relative difference 8.98e-13 (sigma, 3-D, fourth step); u alone 7.46e-13; plane strain 6.52e-13 / 1.94e-13.
SOLVER_MEASURED = 8.98e-13
SOLVER_TOL = 10 * SOLVER_MEASURED
# The same comparison on tests/golden/data/mesh.xml (a 10 x 5 x 20 block of 4 000 cells, sheared across its long axis: a worse
# conditioned operator) after four steps: file order u 1.40e-12, sigma 1.49e-11, h 2.03e-11, e 1.84e-11; locality order u 2.30e-12,
# sigma 3.99e-11, h 6.23e-11, e 5.64e-11.
FILE_MESH_MEASURED = 6.23e-11
FILE_MESH_TOL = 10 * FILE_MESH_MEASURED
# Limits, cantilever 8 x 3 x 3: u after a step of 1e-9 tau_min against the elastic solution with (G0, K) 1.18e-10; after a step of
# 1e9 tau_max against the elastic solution with (G0 g_inf, K) 1.42e-10; the steady solve against the latter 3.09e-13.  The first two
# are the step factors, not the solve: mu_eff / G0 - 1 = -sum g_k x_k / 2 = -(0.3 x 1e-9 + 0.2 x 1e-10) / 2 = -1.6e-10.
LIMIT_MEASURED = 1.42e-10
LIMIT_TOL = 10 * LIMIT_MEASURED
# Equilibrium: || int B^T sigma dx - f_ext || over the free dofs / || f_ext || after every step, from the STORED stress - the true
# residual of the step's linear system: 4.00e-12 (3-D, last step), 1.75e-12 in plane strain.
EQUILIBRIUM_MEASURED = 4.00e-12
EQUILIBRIUM_TOL = 10 * EQUILIBRIUM_MEASURED
# Empty series against LinearElasticitySolver on the same case (two Krylov solves to 1e-12): 3.83e-14 in 3-D, 0 in plane strain.
LINEAR_MEASURED = 3.83e-14
LINEAR_TOL = 10 * LINEAR_MEASURED


def _device(mesh):
    from fenicssolver_amd.fem import VectorFunctionSpace
    from fenicssolver_amd import backend
    backend.init()
    V = VectorFunctionSpace(mesh, "Lagrange", 1)
    return V, V.device()


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


def _random_dev(rng, shape, d, scale):
    """random symmetric trace-free tensors [..., 3, 3]; plane strain: no xz, yz components (they are not stored)"""
    b = scale * rng.standard_normal(shape + (3, 3))
    t = 0.5 * (b + np.swapaxes(b, -1, -2))
    if d == 2:
        t[..., :2, 2] = 0.0
        t[..., 2, :2] = 0.0
    return t - np.trace(t, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0


def _pack_h(h, d):
    nc, nt = h.shape[:2]
    return vr.pack(h.reshape(nc * nt, 3, 3), d).reshape(nc, nt, -1)


MATERIALS = {
    # (mu, lambda, g [nt], tau [nt]); the relaxation times put dt / tau on both sides of the series switch-over (1e-5) and far beyond 1
    "const1": (MU_, LM_, np.array([0.4]), np.array([0.7])),
    "const8": (MU_, LM_, np.array([0.05, 0.1, 0.15, 0.05, 0.1, 0.2, 0.05, 0.1]), np.array([1e7, 4e4 + 0.5, 90.0, 3.0, 0.4, 0.05, 1e-3, 1e-9])),
}


def _material(kind, nc):
    """(device material argument, (mu, lambda, g, tau) for the reference)"""
    if kind != "cell3":
        mu, lm, g, tau = MATERIALS[kind]
        return (mu, lm, list(zip(g, tau))), (mu, lm, g, tau)
    rng = np.random.default_rng(7)
    mu, lm = MU_ * (1 + 0.2 * rng.random(nc)), LM_ * (1 + 0.2 * rng.random(nc))
    g = np.stack([0.3 * rng.random(nc) + 0.01, 0.3 * rng.random(nc) + 0.01, 0.3 * rng.random(nc) + 0.01], axis=1)
    tau = np.stack([10.0 ** rng.uniform(-3, 0, nc), 10.0 ** rng.uniform(0, 3, nc), 10.0 ** rng.uniform(4, 8, nc)], axis=1)
    arr = np.concatenate([mu[:, None], lm[:, None], np.stack([g, tau], axis=2).reshape(nc, 6)], axis=1)
    return ("cell", arr), (mu, lm, g, tau)


# ---- 1. the kernels against the reference -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("kind", ["cell3", "const1", "const8"])
def test_kernels_match_the_host_reference_and_are_deterministic(d, kind):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    co, ce = mesh.coordinates()[:, :d], mesh.cells()
    dev_mat, (mu, lm, g, tau) = _material(kind, nc)
    nt = g.shape[-1]
    rng = np.random.default_rng(50 + d)
    uh = _smooth_u(mesh.coordinates(), d, 2e-3)
    e0, h0 = _random_dev(rng, (nc,), d, 1e-3), _random_dev(rng, (nc, nt), d, 1e-3)
    dt = 0.4
    hist = backend.ViscoHistory(dV, nt)
    hist.set(vr.pack(e0, d), _pack_h(h0, d))
    u = backend.DeviceVector(dV.n_local, uh)

    def run(material):
        r = backend.DeviceVector(dV.n_owned, np.full(dV.n_owned, 123.0))           # overwritten
        info = backend.assemble_viscoelastic(dV, hist, material, dt, load=r, u=u)
        assert info["n_nonfinite"] == 0 and info["first_nonfinite_cell"] == -1
        return (r.get(),) + hist.get(trial=True)
    first, second = run(dev_mat), run(dev_mat)
    for a, b in zip(first, second):
        assert np.array_equal(a, b)
    load, e1, h1, sg = first
    ref_e, ref_h, ref_s = vr.update(vr.strains(co, ce, uh)[0], e0, h0, mu, lm, g, tau, dt)
    ref_load = vr.history_load(co, ce, e0, h0, mu, g, tau, dt)
    errs = {"load": np.abs(load - ref_load).max() / np.abs(ref_load).max(),
            "e": np.abs(e1 - vr.pack(ref_e, d)).max() / np.abs(ref_e).max(),
            "h": np.abs(h1 - _pack_h(ref_h, d)).max() / np.abs(ref_h).max(),
            "sigma": np.abs(sg - vr.pack(ref_s, d)).max() / np.abs(ref_s).max()}
    print("\nkernels against the reference, d = %d, %s: %s" % (d, kind, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) <= KERNEL_TOL
    # the committed state is what was set, bit for bit
    ec, hc, _ = hist.get()
    assert np.array_equal(ec, vr.pack(e0, d)) and np.array_equal(hc, _pack_h(h0, d))
    if kind != "cell3":
        # a per-cell array that holds the constant in every cell gives the constant's bits
        row = np.concatenate([[mu, lm], np.stack([g, tau], axis=1).ravel()])
        third = run(("cell", np.tile(row, (nc, 1))))
        for a, b in zip(first, third):
            assert np.array_equal(a, b)


# ---- 1b. add=True adds to what the target holds ---------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("kind", ["cell3", "const1"])
def test_add_accumulates_onto_the_target_bit_for_bit(d, kind):
    """History load and internal force with add=True equal y + x bit for bit (one fp64 addition per entry): y the known content of
    the vector, x the result with add=False.  3 x 3 x 4 box: 216 cells, 80 nodes (a partial second slice); 5 x 4 square: 40 cells,
    30 nodes."""
    from fenicssolver_amd import backend
    mesh = _box((3, 3, 4)) if d == 3 else _rect((5, 4))
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    assert (nc, mesh.num_vertices()) == ((216, 80) if d == 3 else (40, 30))
    dev_mat, (mu, lm, g, tau) = _material(kind, nc)
    nt = g.shape[-1]
    rng = np.random.default_rng(70 + d)
    hist = backend.ViscoHistory(dV, nt)
    hist.set(vr.pack(_random_dev(rng, (nc,), d, 1e-3), d), _pack_h(_random_dev(rng, (nc, nt), d, 1e-3), d))
    u = backend.DeviceVector(dV.n_local, _smooth_u(mesh.coordinates(), d, 2e-3))
    dt = 0.4
    y = 0.37 + rng.standard_normal(dV.n_owned)
    x = backend.DeviceVector(dV.n_owned)
    backend.assemble_viscoelastic(dV, hist, dev_mat, dt, load=x, u=u)            # the load, then the trial stress of u
    ya = backend.DeviceVector(dV.n_owned, y)
    backend.assemble_viscoelastic(dV, hist, dev_mat, dt, load=ya, add=True)
    assert np.abs(x.get()).max() > 0.0
    assert np.array_equal(ya.get(), y + x.get())
    backend.assemble_viscoelastic(dV, hist, dev_mat, dt, force=x)
    ya.set(y)
    backend.assemble_viscoelastic(dV, hist, dev_mat, dt, force=ya, add=True)
    assert np.abs(x.get()).max() > 0.0
    assert np.array_equal(ya.get(), y + x.get())


def test_a_nonfinite_displacement_is_counted_and_the_c_abi_refuses_bad_input():
    from fenicssolver_amd import backend
    mesh = _box()
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    uh = _smooth_u(mesh.coordinates(), 3, 2e-3)
    hist = backend.ViscoHistory(dV, 1)
    bad = uh.copy()
    bad[7] = np.nan
    info = backend.assemble_viscoelastic(dV, hist, (MU_, LM_, [(0.4, 0.7)]), 0.4, u=backend.DeviceVector(dV.n_local, bad))
    touched = np.nonzero((mesh.cells() == 2).any(axis=1))[0]           # dof 7 belongs to vertex 2
    assert info["n_nonfinite"] == len(touched) and info["first_nonfinite_cell"] in touched
    u = backend.DeviceVector(dV.n_local, uh)
    for material, dt, match in [((MU_, LM_, [(0.0, 0.7)]), 0.4, "must be positive"), ((MU_, LM_, [(0.4, -1.0)]), 0.4, "must be positive"),
                                ((MU_, LM_, [(1.0, 0.7)]), 0.4, "sum g_k < 1"), ((MU_, LM_, [(0.4, 0.7)]), 0.0, "dt > 0"),
                                ((MU_, LM_, [(0.4, 0.7)]), float("inf"), "dt > 0"), ((MU_, LM_, [(0.4, 0.7)]), float("nan"), "dt > 0"),
                                ((MU_, LM_, [(0.2, 0.7), (0.2, 0.7)]), 0.4, "created for 1")]:
        with pytest.raises(backend.BackendError, match=match):
            backend.assemble_viscoelastic(dV, hist, material, dt, u=u)
    arr = np.tile([MU_, LM_, 0.4, 0.7], (nc, 1))
    arr[5, 2] = -0.1
    with pytest.raises(backend.BackendError, match=r"cell 5 \(device order\)"):
        backend.assemble_viscoelastic(dV, hist, ("cell", arr), 0.4, u=u)
    with pytest.raises(backend.BackendError, match="FS_VISCO_MAX_TERMS"):
        backend.ViscoHistory(dV, 9)
    from fenicssolver_amd.fem import FunctionSpace
    with pytest.raises(backend.BackendError, match="vector CG1"):
        backend.ViscoHistory(FunctionSpace(mesh, "P", 1).device(), 1)


# ---- 2. the empty series ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
def test_empty_series_has_no_history_load(d):
    from fenicssolver_amd import backend
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    hist = backend.ViscoHistory(dV, 0)
    hist.set(vr.pack(_random_dev(np.random.default_rng(1), (nc,), d, 1e-3), d), np.zeros((nc, 0, hist.n_comp)))
    for material in ((MU_, LM_, []), ("cell", np.tile([MU_, LM_], (nc, 1)))):
        r = backend.DeviceVector(dV.n_owned, np.full(dV.n_owned, 123.0))
        backend.assemble_viscoelastic(dV, hist, material, 0.4, load=r)
        assert np.all(r.get() == 0.0)


def _cantilever_case(d, series, loads=1.0, times=None, krylov=1e-12, n=None):
    """3-D: a box clamped at x = 0 under the dead end traction (0, 0, -T) on x = 4, region 1 for x < 2 and region 2 beyond.  2-D (plane
    strain): a rectangle fixed at y = 0 under the traction (0, -T) on the part 0.5 <= x <= 1.5 of its top edge, region 1 for x < 1.
    times: the time points (None: the steady, long-term solve)."""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, MeshFunction, near
    from fenicssolver_amd import SolverBase as SB
    bcs = OrderedDict()
    if d == 3:
        mesh = BoxMesh(Point(0, 0, 0), Point(4, 1, 1), *(n or (8, 3, 3)))
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0, 0.0, 0.0))}
        bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 4.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': Constant((0.0, 0.0, -loads))}
    else:
        mesh = RectangleMesh(Point(0, 0), Point(2, 1), *(n or (16, 8)))
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[1], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0, 0.0))}
        bcs["punch"] = {'boundary': AutoSubDomain(lambda x: near(x[1], 1.0) and 0.5 - 1e-12 <= x[0] <= 1.5 + 1e-12), 'boundary_id': 2,
                        'type': 'stress', 'value': Constant((0.0, -loads))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'polymer', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': 1200, 'thermal_expansion_coefficient': 0.0,
                     'prony_series': series}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': krylov}
    if times is not None:
        s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': times[0], 'time_series': list(times),
                                                      'ending_time': times[-1] - 1e-9 * (times[-1] - times[-2])}
    sub = MeshFunction("size_t", mesh, d)
    sub.array()[:] = np.where(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1)[:, 0] < (2.0 if d == 3 else 1.0), 1, 2)
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


def _cantilever_loads(mesh, d, T=1.0):
    """(f_ext, Dirichlet dofs) of _cantilever_case on the host"""
    co = mesh.coordinates()[:, :d]
    if d == 3:
        f = _facet_load(mesh, 3, lambda x: np.abs(x[..., 0] - 4.0) < 1e-12, (0.0, 0.0, -T))
        dofs = (np.nonzero(np.abs(co[:, 0]) < 1e-12)[0][:, None] * 3 + np.arange(3)).ravel()
    else:
        f = _facet_load(mesh, 2, lambda x: (np.abs(x[..., 1] - 1.0) < 1e-12) & (x[..., 0] > 0.5 - 1e-12) & (x[..., 0] < 1.5 + 1e-12), (0.0, -T))
        dofs = (np.nonzero(np.abs(co[:, 1]) < 1e-12)[0][:, None] * 2 + np.arange(2)).ravel()
    return f, dofs


def _term(g, tau):
    return {'relative_modulus': g, 'relaxation_time': tau}


def _regions(a, b):
    return {'near': {'subdomain_id': 1, 'value': a}, 'far': {'subdomain_id': 2, 'value': b}}


SERIES_CONST = [_term(0.3, 0.5), _term(0.2, 5.0)]
SERIES_REGION = [_term(_regions(0.3, 0.15), _regions(0.5, 0.2)), _term(0.2, _regions(5.0, 2.0))]
T_LOAD = 0.01


def _region_terms(sub):
    first = sub.array() == 1
    g = np.stack([np.where(first, 0.3, 0.15), np.full(first.size, 0.2)], axis=1)
    tau = np.stack([np.where(first, 0.5, 0.2), np.where(first, 5.0, 2.0)], axis=1)
    return g, tau


@pytest.mark.parametrize("d", [3, 2])
def test_solver_with_an_empty_series_returns_the_linear_solution(d):
    """The same operator, right-hand side and Krylov solve on both sides: the two fields agree to what the stopping test leaves."""
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    s, mesh, sub = _cantilever_case(d, [], loads=T_LOAD, times=[0.0, 1.0, 2.0])
    vs = ViscoelasticitySolver(copy.deepcopy(s))
    u = vs.solve().vector()._values().copy()
    assert vs.viscous_strains().shape == (mesh.num_cells(), 0, 6 if d == 3 else 4)
    del s['material']['prony_series']
    s['solver_settings']['transient_settings'] = {'transient': False, 'starting_time': 0.0, 'time_step': 1.0, 'ending_time': 1.0}
    lin = LinearElasticitySolver(s)
    lin.reference_load_sign = False
    ul = lin.solve().vector()._values()
    assert np.abs(ul).max() > 1e-5
    print("\nempty series against the linear solver, d = %d: %.2e" % (d, np.abs(u - ul).max() / np.abs(ul).max()))
    assert np.abs(u - ul).max() <= LINEAR_TOL * np.abs(ul).max()
    assert vs.operator_assemblies == 1


# ---- 3. the semigroup property on the device ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("d", [3, 2])
def test_two_half_steps_equal_one_step_on_the_device(d):
    from fenicssolver_amd import backend
    mesh = _box((6, 5, 4)) if d == 3 else _rect()
    V, dV = _device(mesh)
    nc = mesh.num_cells()
    co, ce = mesh.coordinates()[:, :d], mesh.cells()
    dev_mat, (mu, lm, g, tau) = _material("cell3", nc)
    rng = np.random.default_rng(60 + d)
    u0, u1 = _smooth_u(mesh.coordinates(), d, 2e-3), 1.7 * _smooth_u(mesh.coordinates() + 0.1, d, 2e-3)
    e0 = vr.pack(vr.dev(vr.strains(co, ce, u0)[0]), d)           # the committed strain is the strain of u0: u is linear in time
    h0 = _pack_h(_random_dev(rng, (nc, 3), d, 1e-3), d)
    dt = 0.4

    def vec(x):
        return backend.DeviceVector(dV.n_local, x)
    one = backend.ViscoHistory(dV, 3)
    one.set(e0, h0)
    backend.assemble_viscoelastic(dV, one, dev_mat, dt, u=vec(u1))
    two = backend.ViscoHistory(dV, 3)
    two.set(e0, h0)
    backend.assemble_viscoelastic(dV, two, dev_mat, 0.5 * dt, u=vec(0.5 * (u0 + u1)))
    two.commit()
    backend.assemble_viscoelastic(dV, two, dev_mat, 0.5 * dt, u=vec(u1))
    (_, h_one, s_one), (_, h_two, s_two) = one.get(trial=True), two.get(trial=True)
    eh, es = np.abs(h_two - h_one).max() / np.abs(h_one).max(), np.abs(s_two - s_one).max() / np.abs(s_one).max()
    print("\nsemigroup on the device, d = %d: h %.2e, sigma %.2e" % (d, eh, es))
    assert eh <= SEMIGROUP_TOL and es <= SEMIGROUP_TOL


# ---- 4. stress relaxation: the closed form ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n, ramp_steps", [((4, 3, 3), 1), ((6, 5, 4), 1), ((4, 3, 3), 2)])
def test_shear_relaxation_closed_form_in_every_cell_and_step(n, ramp_steps):
    """Simple shear u = gamma(t) y e_x on the whole boundary, ramped linearly over [0, t1] and held for six steps.  ramp_steps 1: a
    constant boundary value, the first step ramps from the zero state; 2: the boundary value is a per-step sequence that reaches
    gamma0 / 2 at t1 / 2 - the strain is still linear in time, so the recursion stays exact and the closed form the same.  The
    state is homogeneous, so CG1 carries it exactly and every cell follows the closed form."""
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, Expression, near
    from fenicssolver_amd import SolverBase as SB
    L = (1.0, 0.8, 0.6)
    gamma0, t1, dt, nhold = 1e-3, 0.3, 0.4, 6
    mesh = BoxMesh(Point(0, 0, 0), Point(*L), *n)
    bcs = OrderedDict()
    bcs["all"] = {'boundary': AutoSubDomain(lambda x: any(near(x[k], 0.0) or near(x[k], L[k]) for k in range(3))), 'boundary_id': 1,
                  'type': 'Dirichlet', 'value': (Expression("%r * x[1]" % gamma0, degree=1), Constant(0.0), Constant(0.0))}
    times = [t1 * (k + 1) / ramp_steps for k in range(ramp_steps)] + [t1 + dt * (k + 1) for k in range(nhold)]
    if ramp_steps > 1:
        bcs["all"]['value'] = ([Expression("%r * x[1]" % (gamma0 * min(t / t1, 1.0)), degree=1) for t in times], Constant(0.0), Constant(0.0))
    times = [0.0] + times
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'polymer', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': 1200, 'thermal_expansion_coefficient': 0.0,
                     'prony_series': [_term(float(g), float(t)) for g, t in zip(G2, TAU2)]}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_series': times, 'ending_time': times[-1] - 1e-9}
    solver = ViscoelasticitySolver(s)
    seen = []
    solve_form = solver.solve_form

    def checked(F, u_, bcs_):
        out = solve_form(F, u_, bcs_)
        k = len(seen)
        t = times[k + 1]
        exact = vr.shear_ramp_hold(MU_, gamma0, G2, TAU2, t1, t) if k >= ramp_steps - 1 else vr.shear_ramp(MU_, gamma0, G2, TAU2, t1, t)
        sg = solver.stress()
        other = sg.copy()
        other[:, 3] = 0.0
        seen.append(max(np.abs(sg[:, 3] - exact).max(), np.abs(other).max()) / (MU_ * gamma0))
        return out
    solver.solve_form = checked
    solver.solve()
    assert len(seen) == nhold + ramp_steps
    assert abs(vr.shear_ramp(MU_, gamma0, G2, TAU2, t1, t1) - vr.shear_ramp_hold(MU_, gamma0, G2, TAU2, t1, t1)) <= 1e-15 * MU_ * gamma0
    assert vr.shear_ramp_hold(MU_, gamma0, G2, TAU2, t1, times[-1]) < 0.8 * vr.shear_ramp_hold(MU_, gamma0, G2, TAU2, t1, t1)
    print("\nshear relaxation closed form, mesh %s, ramp in %d step(s): largest difference / (G0 gamma0) per step %s" % (n, ramp_steps, ["%.2e" % x for x in seen]))
    assert max(seen) <= RELAX_TOL
    # the relaxation modulus of the solver is the closed form's instant-ramp limit
    assert abs(solver.relaxation_modulus(2.0) - vr.relaxation_modulus(MU_, G2, TAU2, 2.0)) <= 1e-14 * MU_


# ---- 5. the solver against the reference marcher, 7. equilibrium --------------------------------------------------------------------
CREEP_TIMES = [0.0, 0.25, 0.5, 0.75, 1.0, 2.0, 3.0, 4.0]          # seven steps, one change of the step length


@functools.lru_cache(maxsize=None)
def _creep_run(d):
    """The creep case once per dimension: per step the solver's (u, sigma) differences to the reference marcher and the equilibrium
    residual of the stored stress; the build counters at the end."""
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    from fenicssolver_amd import backend
    s, mesh, sub = _cantilever_case(d, copy.deepcopy(SERIES_REGION), loads=T_LOAD, times=CREEP_TIMES)
    co = mesh.coordinates()[:, :d]
    f_ext, dofs = _cantilever_loads(mesh, d, T_LOAD)
    g, tau = _region_terms(sub)
    dts = np.diff(CREEP_TIMES)
    ref = vr.march(co, mesh.cells(), (MU_, LM_, g, tau), [(float(dt), f_ext, dofs, np.zeros(len(dofs))) for dt in dts])
    solver = ViscoelasticitySolver(s)
    solver.subdomains = sub
    free = np.ones(f_ext.size, dtype=bool)
    free[dofs] = False
    rec = []
    solve_form = solver.solve_form

    def checked(F, u_, bcs_):
        out = solve_form(F, u_, bcs_)
        st = ref[len(rec)]
        u = out.vector()._values()
        dV = solver.function_space.device()
        assert solver.function_space.localizer() is None                   # a generated mesh: device order = host order
        r = backend.DeviceVector(dV.n_owned)
        backend.assemble_viscoelastic(dV, solver.history, F.material_spec(), F.dt, force=r)
        res = r.get()[:f_ext.size] - f_ext
        rec.append({"u": np.abs(u - st["u"]).max() / np.abs(st["u"]).max(),
                    "sigma": np.abs(solver.stress() - vr.pack(st["sigma"], d)).max() / np.abs(st["sigma"]).max(),
                    "equilibrium": np.linalg.norm(res[free]) / np.linalg.norm(f_ext), "umax": np.abs(u).max()})
        return out
    solver.solve_form = checked
    solver.solve()
    return rec, solver.operator_assemblies, solver.amg_setups, ref


@pytest.mark.parametrize("d", [3, 2])
def test_solver_matches_the_reference_marcher_step_by_step(d):
    rec, n_ops, n_amg, ref = _creep_run(d)
    assert len(rec) == len(CREEP_TIMES) - 1
    # it creeps: the tip keeps moving under the constant load
    assert rec[-1]["umax"] > 1.15 * rec[0]["umax"]
    print("\nsolver against the reference marcher, d = %d: relative difference (u, sigma) per step %s" % (
        d, [("%.2e" % r["u"], "%.2e" % r["sigma"]) for r in rec]))
    assert max(max(r["u"], r["sigma"]) for r in rec) <= SOLVER_TOL
    # the effective operator is assembled once per distinct step length; in 3-D its AMG hierarchy too (2-D is Jacobi-CG: no hierarchy)
    distinct = len(set(np.diff(CREEP_TIMES).tolist()))
    assert distinct == 2 and n_ops == distinct
    assert n_amg == (distinct if d == 3 else 0)


@pytest.mark.parametrize("d", [3, 2])
def test_stored_stress_is_in_equilibrium_with_the_loads_after_every_step(d):
    rec = _creep_run(d)[0]
    print("\nequilibrium of the stored stress, d = %d: |int B^T sigma - f_ext| / |f_ext| on the free dofs per step %s" % (
        d, ["%.2e" % r["equilibrium"] for r in rec]))
    assert max(r["equilibrium"] for r in rec) <= EQUILIBRIUM_TOL


# ---- 6. the limits ----------------------------------------------------------------------------------------------------------------
def test_instantaneous_and_long_term_limits_are_the_elastic_solutions():
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    t1 = 1e-9 * TAU2.min()
    s, mesh, sub = _cantilever_case(3, copy.deepcopy(SERIES_CONST), loads=T_LOAD, times=[0.0, t1, t1 + 1e9 * TAU2.max()])
    f_ext, dofs = _cantilever_loads(mesh, 3, T_LOAD)
    co = mesh.coordinates()
    ginf = 1.0 - G2.sum()
    K = LM_ + 2.0 * MU_ / 3.0
    u_inst = vr.elastic_solve(co, mesh.cells(), MU_, LM_, f_ext, dofs, 0.0)
    u_long = vr.elastic_solve(co, mesh.cells(), MU_ * ginf, K - 2.0 * MU_ * ginf / 3.0, f_ext, dofs, 0.0)
    assert np.abs(u_long).max() > 1.3 * np.abs(u_inst).max()
    solver = ViscoelasticitySolver(copy.deepcopy(s))
    got = []
    solve_form = solver.solve_form

    def keep(F, u_, bcs_):
        out = solve_form(F, u_, bcs_)
        got.append(out.vector()._values().copy())
        return out
    solver.solve_form = keep
    solver.solve()
    assert len(got) == 2
    s['solver_settings']['transient_settings'] = {'transient': False, 'starting_time': 0.0, 'time_step': 1.0, 'ending_time': 1.0}
    steady = ViscoelasticitySolver(s)
    u_steady = steady.solve().vector()._values()
    errs = {"instantaneous": np.abs(got[0] - u_inst).max() / np.abs(u_inst).max(),
            "long-term": np.abs(got[1] - u_long).max() / np.abs(u_long).max(),
            "steady": np.abs(u_steady - u_long).max() / np.abs(u_long).max(),
            "steady against the long step": np.abs(u_steady - got[1]).max() / np.abs(u_long).max()}
    print("\nlimits: %s" % {k: "%.2e" % v for k, v in errs.items()})
    assert max(errs.values()) <= LIMIT_TOL
    # the steady solve keeps no viscous strains and stores the long-term stress
    assert steady.viscous_strains().shape[1] == 0
    sig = vr.update(vr.strains(co, mesh.cells(), u_long)[0], np.zeros((mesh.num_cells(), 3, 3)), np.zeros((mesh.num_cells(), 0, 3, 3)),
                    MU_ * ginf, K - 2.0 * MU_ * ginf / 3.0, np.zeros(0), np.zeros(0), 1.0)[2]
    assert np.abs(steady.stress() - vr.pack(sig, 3)).max() <= LIMIT_TOL * np.abs(sig).max()


# ---- 8. discipline ------------------------------------------------------------------------------------------------------------------
def test_a_failed_solve_leaves_the_committed_history_untouched():
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    from fenicssolver_amd.SolverBase import SolverError
    s, mesh, sub = _cantilever_case(3, copy.deepcopy(SERIES_REGION), loads=T_LOAD, times=CREEP_TIMES)
    solver = ViscoelasticitySolver(s)
    solver.subdomains = sub
    solve_form = solver.solve_form
    state = {"steps": 0}

    def limited(F, u_, bcs_):
        if state["steps"] == 3:
            state["before"] = solver.history.get()
            solver.solver_settings['solver_parameters'].update({'maximum_iterations': 1, 'krylov_maximum_iterations': 1})
        state["steps"] += 1
        return solve_form(F, u_, bcs_)
    solver.solve_form = limited
    with pytest.raises(SolverError, match="did not converge"):
        solver.solve()
    after = solver.history.get()
    assert state["steps"] == 4 and np.abs(state["before"][1]).max() > 0.0
    assert all(np.array_equal(a, b) for a, b in zip(state["before"], after))


def test_two_solves_give_the_same_bits():
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    out = []
    for _ in range(2):
        s, mesh, sub = _cantilever_case(3, copy.deepcopy(SERIES_REGION), loads=T_LOAD, times=CREEP_TIMES)
        solver = ViscoelasticitySolver(s)
        solver.subdomains = sub
        u = solver.solve().vector()._values().copy()
        out.append((u, solver.stress(), solver.viscous_strains(), solver.deviatoric_strain()))
    assert np.abs(out[0][2]).max() > 0.0
    for a, b in zip(out[0], out[1]):
        assert np.array_equal(a, b)
    # the same solver again starts from the zero state
    u3 = solver.solve().vector()._values()
    assert np.array_equal(u3, out[0][0]) and np.array_equal(solver.viscous_strains(), out[0][2])
    assert solver.operator_assemblies == 2


XML_TIMES = [0.0, 0.5, 1.0, 2.0, 3.0]


def _xml_mesh():
    from fenicssolver_amd.fem import Mesh, MeshFunction
    data = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")
    mesh = Mesh(os.path.join(data, "mesh.xml"))
    sub = MeshFunction("size_t", mesh, os.path.join(data, "mesh_physical_region.xml"))
    ids = np.unique(np.asarray(sub.array(), dtype=np.int64))
    g1 = {int(i): 0.15 + 0.1 * k for k, i in enumerate(ids)}
    tau1 = {int(i): 0.3 * (1 + k) for k, i in enumerate(ids)}
    return mesh, sub, g1, tau1


@functools.lru_cache(maxsize=None)
def _xml_reference():
    mesh, sub, g1, tau1 = _xml_mesh()
    co = mesh.coordinates()
    ids = np.asarray(sub.array(), dtype=np.int64)
    g = np.stack([np.array([g1[int(i)] for i in ids]), np.full(ids.size, 0.2)], axis=1)
    tau = np.stack([np.array([tau1[int(i)] for i in ids]), np.full(ids.size, 4.0)], axis=1)
    f_ext = _facet_load(mesh, 3, lambda x: np.abs(x[..., 2] - 20.0) < 1e-9, (T_LOAD, 0.0, 0.0))
    dofs = (np.nonzero(np.abs(co[:, 2]) < 1e-9)[0][:, None] * 3 + np.arange(3)).ravel()
    return vr.march(co, mesh.cells(), (MU_, LM_, g, tau), [(float(dt), f_ext, dofs, np.zeros(len(dofs))) for dt in np.diff(XML_TIMES)])[-1]


@pytest.mark.parametrize("renumber", [False, True])
def test_accessors_use_the_callers_cell_numbering_on_a_file_mesh(monkeypatch, renumber):
    """tests/golden/data/mesh.xml (a 10 x 5 x 20 block) with its region file, uploaded in file order or in locality order: clamped at
    z = 0, sheared at z = 20, the first Prony term by region."""
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    from fenicssolver_amd.fem import VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    monkeypatch.setenv("FS_RENUMBER", "1" if renumber else "0")
    mesh, sub, g1, tau1 = _xml_mesh()
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                    'value': Constant((0.0, 0.0, 0.0))}
    bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 20.0)), 'boundary_id': 2, 'type': 'stress', 'value': Constant((T_LOAD, 0.0, 0.0))}
    s = copy.deepcopy(SB.default_case_settings)
    series = [_term({'r%d' % i: {'subdomain_id': i, 'value': v} for i, v in g1.items()},
                    {'r%d' % i: {'subdomain_id': i, 'value': v} for i, v in tau1.items()}), _term(0.2, 4.0)]
    s['material'] = {'name': 'polymer', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': 1200, 'thermal_expansion_coefficient': 0.0,
                     'prony_series': series}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET)
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-12}
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_series': XML_TIMES, 'ending_time': XML_TIMES[-1] - 1e-9}
    solver = ViscoelasticitySolver(s)
    solver.subdomains = sub
    u = solver.solve().vector()._values()
    assert (solver.function_space.localizer() is not None) == renumber
    ref = _xml_reference()
    sg, h, e = solver.stress(), solver.viscous_strains(), solver.deviatoric_strain()
    # the regions differ, so a permutation of the cells would show: the comparison is cell by cell, in the file's numbering
    errs = {"u": np.abs(u - ref["u"]).max() / np.abs(ref["u"]).max(),
            "sigma": np.abs(sg - vr.pack(ref["sigma"], 3)).max() / np.abs(ref["sigma"]).max(),
            "h": np.abs(h - _pack_h(ref["h"], 3)).max() / np.abs(ref["h"]).max(),
            "e": np.abs(e - vr.pack(ref["e"], 3)).max() / np.abs(ref["e"]).max()}
    print("\nfile mesh, renumber = %s: %s" % (renumber, {k: "%.2e" % v for k, v in errs.items()}))
    assert max(errs.values()) <= FILE_MESH_TOL
    # von_Mises() projects the stored stress
    vm_cells = vr.von_mises(ref["sigma"])
    assert np.abs(solver.von_Mises_cells() - vm_cells).max() <= FILE_MESH_TOL * vm_cells.max()
    vm = solver.von_Mises().vector()._values()
    assert np.all(np.isfinite(vm)) and 0.5 * vm_cells.max() < vm.max() < 1.5 * vm_cells.max()


# ---- 9. the command line ------------------------------------------------------------------------------------------------------------
def test_command_line_runs_the_json_relaxation_case_end_to_end():
    """python -m fenicssolver_amd case.json with "solver_name": "ViscoelasticitySolver": the top face of the block is sheared in a
    short first step and held; the shear stress relaxes towards its long-term value."""
    import subprocess
    import sys
    from fenicssolver_amd.main import main
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    case_file = os.path.join(root, "tests", "golden", "data", "TestViscoelasticRelaxation.json")
    env = dict(os.environ, FENICSSOLVER_BATCH="1", PYTHONPATH=root + os.pathsep + os.environ.get("PYTHONPATH", ""))
    run = subprocess.run([sys.executable, "-m", "fenicssolver_amd", case_file], cwd=root, env=env, capture_output=True, text=True, timeout=120)
    assert run.returncode == 0, run.stdout[-2000:] + run.stderr[-2000:]
    # the same case in this process: what the run computed
    solver = main(case_file)
    assert len(solver.step_stats) == 5 and solver.operator_assemblies == 5
    sg, h = solver.stress(), solver.viscous_strains()
    assert np.all(np.isfinite(sg)) and np.abs(h).max() > 0.0
    # The mean shear stress sigma_xz (the shear force on the top face) at t = 4 against the long-term equilibrium of the same case: it
    # has not fully relaxed yet, and it cannot exceed the long-term value by more than the shear modulus does,
    # G(3.99) / G_inf = (0.5 + 0.3 exp(-3.99/0.5) + 0.2 exp(-3.99/5)) / 0.5 = 1.180, since the bulk modulus does not relax at all.
    from fenicssolver_amd.main import load_settings
    from fenicssolver_amd.ViscoelasticitySolver import ViscoelasticitySolver
    s = load_settings(case_file)
    s['solver_settings']['transient_settings'] = {'transient': False, 'starting_time': 0.0, 'time_step': 1.0, 'ending_time': 1.0}
    steady = ViscoelasticitySolver(s)
    steady.solve()
    ratio = sg[:, 4].mean() / steady.stress()[:, 4].mean()
    print("\ncommand-line relaxation case: mean sigma_xz at t = 4 over its long-term value: %.4f" % ratio)
    assert 1.05 < ratio < 1.181

