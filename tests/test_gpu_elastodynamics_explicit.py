"""The explicit scheme of ElastodynamicsSolver and the fs_dyn_explicit_* kernels on the MI355X: the kernels against numpy row by row,
split invariance and repeatability bit for bit, the solver against the reference marcher (tests/elastodynamics_explicit_reference.py)
step by step, single modes against their closed form, the discrete energy identities, the step bounds, the build discipline and the
refusals of the library."""
import copy
import functools
import math
import os
from collections import OrderedDict

import numpy as np
import pytest
import scipy.linalg
import scipy.sparse as sp

import elastodynamics_explicit_reference as xr

pytestmark = pytest.mark.gpu

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E_, NU_, RHO_ = 200.0, 0.3, 1.0
MU_, LM_ = E_ / (2 * (1 + NU_)), E_ * NU_ / ((1 + NU_) * (1 - 2 * NU_))

ROW_TOL = 32 * 2.0 ** -53       # set by the issue: per row |device - numpy| <= 32 x 2^-53 x (sum of the absolute terms of that row)
ENERGY_TOL = 1e-12              # set by the issue: the energy halves of a step against numpy with the device's own fields, relative

# Measured on the MI355X (this file: the tests print every figure before they assert), and the bounds derived from them: 10 x the
# measured figure, the margin covering the mesh family rather than one mesh.
# Solver against the reference marcher, 40 steps of 0.5 x critical_time_step(), GPU minus reference relative to the largest entry of
# the reference field at that step, largest over the steps as (u, v, a, traces):
#   cantilever 8 x 3 x 3, Ricker tip load                                    1.16e-15  1.45e-15  2.12e-15  8.00e-16
#   rectangle 16 x 8, moving Dirichlet side                                  7.38e-16  2.32e-15  6.60e-15  5.20e-16
#   tests/golden/data/mesh.xml, per-region E and density                     1.33e-15  1.25e-15  2.31e-15  6.51e-17
MARCH_MEASURED = {"u": 1.33e-15, "v": 2.32e-15, "a": 6.60e-15, "traces": 8.00e-16}
MARCH_TOL = {k: 10 * v for k, v in MARCH_MEASURED.items()}
# Single mode over the 24 intervals of 0.2 / omega, each taken as q stable substeps (0.2 / omega is 19.6, 1.8 and 1.8 times the stable
# bound of these meshes), against phi cos(omega_h n dt), relative to max |phi|: cantilever mode 0 (q = 40, 960 steps) 6.79e-12, mode 7
# (q = 4, 96 steps) 1.10e-14, rectangle mode 2 (q = 4, 96 steps) 3.47e-14
MODE_MEASURED = 6.79e-12
MODE_TOL = 10 * MODE_MEASURED
# Energy over 200 steps of 0.5 x critical_time_step(), relative to E_0 = E_{1/2}: drift undamped and unloaded 3.76e-14 (cantilever), 4.09e-15 (rectangle); damped
# (eta_M = 0.5), the defect of E_{n+1/2} - E_{n-1/2} + eta_M dt v_n^T diag(m) v_n 6.67e-14, 2.53e-15
ENERGY_DRIFT_MEASURED = 3.76e-14
ENERGY_DRIFT_TOL = 10 * ENERGY_DRIFT_MEASURED
ENERGY_DEFECT_MEASURED = 6.67e-14
ENERGY_DEFECT_TOL = 10 * ENERGY_DEFECT_MEASURED
# Kernels against numpy, largest row figure in units of 2^-53 (the issue's bound is 32): 81 dofs 2.8, 375 dofs 4.4,
# rectangle 3.9, 273 375 dofs 6.4; the energy halves of a step against numpy 6.0e-16 or better (the issue's bound is 1e-12).


@pytest.fixture(autouse=True)
def _file_order(monkeypatch):
    monkeypatch.setenv("FS_RENUMBER", "0")                                  # a file mesh in file order: device order = host order


def _host_csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


def _lumped_mass(M, dV):
    from fenicssolver_amd import backend
    ones, md = backend.DeviceVector(dV.n_local, np.ones(dV.n_local)), backend.DeviceVector(dV.n_owned)
    M.spmv(ones, md)
    return md.get()[:dV.n_owned].copy()


def _product(K, dV, x):
    from fenicssolver_amd import backend
    xd, yd = backend.DeviceVector(dV.n_local, x), backend.DeviceVector(dV.n_owned)
    K.spmv(xd, yd)
    return yd.get()[:dV.n_owned].copy()


# ---- 1. the kernels against numpy ------------------------------------------------------------------------------------------------
def _space(shape):
    """(device space, what keeps it alive) of a shape of the issue's list"""
    from fenicssolver_amd import backend
    from fenicssolver_amd.fem import RectangleMesh, Point, VectorFunctionSpace
    backend.init()
    kind, n = shape
    if kind == "box":
        mesh = backend.DeviceMesh.box(n, n, n)
        return backend.DeviceSpace(mesh, 3, 1), mesh
    V = VectorFunctionSpace(RectangleMesh(Point(0, 0), Point(1.0, 0.7), 6, 5), "Lagrange", 1)
    return V.device(), V


def _operators(dV):
    from fenicssolver_amd import backend
    K, M = backend.DeviceMatrix(dV), backend.DeviceMatrix(dV)
    K.assemble(lame=(MU_, LM_))
    M.assemble(lame=(0.0, 0.0), mass=RHO_)
    m = _lumped_mass(M, dV)
    M.close()
    return K, m


def _update_reference(u, w, y, m, F, g, is_d, dt, eta, sf, sg):
    """(w+, sum of its absolute terms, u+, sum of its absolute terms) of one step, term by term"""
    al = 0.5 * eta * dt
    wn = ((1 - al) * w + dt * (sf * F - y) / m) / (1 + al)
    s_w = (np.abs((1 - al) * w) + dt * (np.abs(sf * F) + np.abs(y)) / m) / (1 + al)
    un, s_u = u + dt * wn, np.abs(u) + dt * s_w
    ud = g * sg
    un, s_u = np.where(is_d, ud, un), np.where(is_d, np.abs(ud), s_u)
    wn, s_w = np.where(is_d, (ud - u) / dt, wn), np.where(is_d, (np.abs(ud) + np.abs(u)) / dt, s_w)
    return wn, s_w, un, s_u


SHAPES = [("box", 2), ("box", 4), ("rect", 0), ("box", 44)]


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%s%d" % s)
def test_kernels_match_numpy_row_by_row(shape):
    from fenicssolver_amd import backend
    dV, keep = _space(shape)
    n = dV.n_owned
    assert shape != ("box", 2) or n == 81
    assert shape != ("box", 4) or n == 375
    assert shape != ("box", 44) or (n == 273375 and n > 1024 * 256)         # the grid-stride loop makes a second trip
    K, m = _operators(dV)
    assert np.all(m > 0.0)
    rng = np.random.default_rng(200 + n)
    u, w, F, v0 = (rng.standard_normal(n) * s for s in (1e-2, 1e-1, 0.5, 1e-1))
    # Dirichlet dofs, some named twice (the last value holds); receivers on a Dirichlet dof, on a free one, one named twice, the last dof
    dd = rng.choice(n - 1, size=max(n // 9, 4), replace=False).astype(np.int32)
    dofs = np.concatenate([dd, dd[:3]])
    vals = rng.standard_normal(len(dofs))
    g = np.zeros(n)
    is_d = np.zeros(n, dtype=bool)
    for i, val in zip(dofs, vals):
        g[i], is_d[i] = val, True
    free = np.nonzero(~is_d)[0]
    rec = np.array([dd[0], free[0], free[-2], dd[1], free[0], n - 1], dtype=np.int32)
    Fg = np.where(is_d, 0.0, F)
    dt, sf, sg, sf2 = 1e-3, 0.7, -1.3, 0.45
    st = backend.ExplicitDynamicsState(dV)
    lines, worst, e_worst, exact = [], 0.0, 0.0, True
    for eta in (0.0, 0.3):
        st.configure(dt, eta, m, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)
        # one step of the march
        st.set(u, w, step=3)
        out = st.advance(K, [sf], [sg], receivers=rec)
        y = st.work()
        u1, w1, step = st.get()
        exact &= np.array_equal(y, _product(K, dV, u)) and step == 4 and out["step"] == 4
        wn, s_w, un, s_u = _update_reference(u, w, y, m, Fg, g, is_d, dt, eta, sf, sg)
        figs = {"w": (np.abs(w1 - wn) / s_w).max(), "u": (np.abs(u1 - un) / np.maximum(s_u, 1e-300)).max()}
        exact &= np.array_equal(u1[is_d], (g * sg)[is_d]) and np.array_equal(out["traces"][0], u1[rec])
        exact &= out["n_nonfinite"] == 0 and out["first_nonfinite_step"] == -1
        # the energy halves of that step, with the device's own fields
        ek, ep = out["energy"][0]
        ek_ref, ep_ref = xr.step_energy(m, w1, u1, y)
        e_fig = max(abs(ek - ek_ref) / abs(ek_ref), abs(ep - ep_ref) / abs(ep_ref))
        # the full-step pair of the new time point: one more product, the state stays
        v, a = st.full_step(K, sf2)
        y2 = st.work()
        u1b, w1b, stepb = st.get()
        exact &= np.array_equal(y2, _product(K, dV, u1)) and np.array_equal(u1b, u1) and np.array_equal(w1b, w1) and stepb == 4
        al = 0.5 * eta * dt
        wp = ((1 - al) * w1 + dt * (sf2 * Fg - y2) / m) / (1 + al)
        s_wp = (np.abs((1 - al) * w1) + dt * (np.abs(sf2 * Fg) + np.abs(y2)) / m) / (1 + al)
        v_ref, s_v = 0.5 * (w1 + wp), 0.5 * (np.abs(w1) + s_wp)
        a_ref, s_a = (wp - w1) / dt, (np.abs(w1) + s_wp) / dt
        figs["v"] = (np.abs(v - v_ref) / s_v)[~is_d].max()
        figs["a"] = (np.abs(a - a_ref) / s_a)[~is_d].max()
        exact &= np.array_equal(v[is_d], w1[is_d]) and not a[is_d].any()
        # the start from (u_0, v_0)
        st.start(K, u, v0, sf, sg, sf2)
        y0 = st.work()
        us, ws, steps_ = st.get()
        u0 = np.where(is_d, g * sg, u)
        exact &= np.array_equal(y0, _product(K, dV, u0)) and steps_ == 1
        a0, s_a0 = (sf * Fg - y0) / m - eta * v0, (np.abs(sf * Fg) + np.abs(y0)) / m + eta * np.abs(v0)
        w_ref, s_ws = v0 + 0.5 * dt * a0, np.abs(v0) + 0.5 * dt * s_a0
        u_ref, s_us = u0 + dt * w_ref, np.abs(u0) + dt * s_ws
        ud = g * sf2
        u_ref, s_us = np.where(is_d, ud, u_ref), np.where(is_d, np.abs(ud), s_us)
        w_ref, s_ws = np.where(is_d, (ud - u0) / dt, w_ref), np.where(is_d, (np.abs(ud) + np.abs(u0)) / dt, s_ws)
        figs["start w"] = (np.abs(ws - w_ref) / np.maximum(s_ws, 1e-300)).max()
        figs["start u"] = (np.abs(us - u_ref) / np.maximum(s_us, 1e-300)).max()
        exact &= np.array_equal(us[is_d], ud[is_d])
        lines.append("%s%d eta_M = %g: largest |device - numpy| / (sum of absolute terms) per row, in units of 2^-53: %s; energy halves "
                     "against numpy, relative: %.2e" % (shape + (eta, {k: "%.2f" % (f * 2.0 ** 53) for k, f in figs.items()}, e_fig)))
        worst, e_worst = max(worst, max(figs.values())), max(e_worst, e_fig)
    # a non-finite field is counted through the energy of its step, and the step is named
    ub = u.copy()
    ub[[1, n - 2]] = np.nan, np.inf
    st.set(ub, w, step=1)
    bad = st.advance(K, [sf, sf], [sg, sg])
    print("\n" + "\n".join(lines))
    assert exact
    assert worst <= ROW_TOL
    assert e_worst <= ENERGY_TOL
    assert bad["n_nonfinite"] == 2 and bad["first_nonfinite_step"] == 0 and bad["step"] == 3
    st.close()
    K.close()


# ---- 2. split invariance and repeatability ---------------------------------------------------------------------------------------
def test_a_march_gives_the_same_bits_however_it_is_split_into_calls():
    from fenicssolver_amd import backend
    dV, keep = _space(("box", 4))
    n = dV.n_owned
    K, m = _operators(dV)
    Kh = _host_csr(K)
    dt = 0.5 * 2.0 / math.sqrt(float((np.asarray(abs(Kh).sum(axis=1)).ravel() / m).max()))
    rng = np.random.default_rng(17)
    u, w, F = rng.standard_normal(n) * 1e-2, rng.standard_normal(n) * 1e-1, rng.standard_normal(n)
    dofs = np.array([0, 1, 2, 30, 31, 0], dtype=np.int32)
    rec = np.array([0, 5, n - 1, 5], dtype=np.int32)
    steps = 130                                                           # two finishing-pass chunks of 64 and a rest
    sf, sg = np.cos(0.1 * np.arange(steps)), 1.0 + 0.2 * np.sin(0.07 * np.arange(steps))
    st = backend.ExplicitDynamicsState(dV)
    st.configure(dt, 0.3, m, load=F, dirichlet_dofs=dofs, dirichlet_values=0.01 * np.arange(1.0, 7.0))

    def run(cuts):
        st.set(u, w, step=1)
        tr, en, bad = [], [], 0
        for a, b in zip(cuts[:-1], cuts[1:]):
            out = st.advance(K, sf[a:b], sg[a:b], receivers=rec)
            tr.append(out["traces"])
            en.append(out["energy"])
            bad += out["n_nonfinite"]
        uu, ww, step = st.get()
        assert step == steps + 1 and bad == 0
        return uu, ww, np.concatenate(tr), np.concatenate(en)
    whole = run([0, steps])
    split = run([0, 1, 8, steps])
    again = run([0, steps])
    assert np.all(np.isfinite(whole[0])) and np.abs(whole[0]).max() > 0.0 and whole[2].shape == (steps, 4) and whole[3].shape == (steps, 2)
    assert np.array_equal(whole[2][:, 1], whole[2][:, 3])                  # a dof named twice is sampled twice
    for a, b, c in zip(whole, split, again):
        assert np.array_equal(a, b) and np.array_equal(a, c)
    st.close()
    K.close()


def test_the_receiver_list_may_change_from_call_to_call_on_one_state():
    """The receiver bits of the device flags follow the list of the call; a bit that is not set leaves its slot of a freshly allocated
    trace buffer unwritten.  Exact: a sample is the field value itself."""
    from fenicssolver_amd import backend
    dV, keep = _space(("box", 2))
    n = dV.n_owned
    assert n == 81
    K, m = _operators(dV)
    rng = np.random.default_rng(23)
    u, w, F = rng.standard_normal(n) * 1e-2, rng.standard_normal(n) * 1e-1, rng.standard_normal(n)
    dofs, vals = np.array([0, 1, 2, 30, 31], dtype=np.int32), 0.01 * np.arange(1.0, 6.0)
    A = np.array([5, 30, 80], dtype=np.int32)                              # one of them a Dirichlet dof
    B = np.array([7, 1, 44], dtype=np.int32)                               # disjoint from A
    C = np.array([80, 80], dtype=np.int32)                                 # shorter, a dof of A, named twice
    sf, sg = rng.standard_normal(7), rng.standard_normal(7)
    st = backend.ExplicitDynamicsState(dV)
    st.configure(1e-3, 0.3, m, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)
    st.set(u, w, step=1)

    def step_with(rec, k):
        out = st.advance(K, sf[k:k + 1], sg[k:k + 1], receivers=rec)
        uu, _, step = st.get()
        assert step == k + 1 and out["step"] == k + 1
        if rec is None:
            assert out["traces"] is None
        else:
            assert out["traces"].shape == (1, len(rec)) and np.array_equal(out["traces"][0], uu[rec]), (k, rec)
    for k, rec in enumerate((A, B, C, None, A), start=1):
        step_with(rec, k)
    uu, ww, step = st.get()
    st.configure(1e-3, 0.3, m, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)      # the flags are uploaded anew, without receiver bits
    st.set(uu, ww, step)
    step_with(B, 6)
    st.close()
    K.close()


# ---- the cases of the solver tests -----------------------------------------------------------------------------------------------
def _xml_mesh():
    from fenicssolver_amd.fem import Mesh
    return Mesh(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data", "mesh.xml"))


def _case(kind, dt, steps, dynamics=None, loaded=True, moving=True, receivers=True, report=None):
    """cantilever: a 4 x 1 x 1 box of 8 x 3 x 3 cells, the face x = 0 fixed, a Ricker traction on the tip x = 4; rectangle: 2 x 1 in plane
    strain, 16 x 8 cells, the edge y = 0 moving in x, a Ricker traction on part of the top edge; xml: tests/golden/data/mesh.xml (a
    10 x 5 x 20 block) in file order, E and the density differing between z < 10 and beyond, the face z = 0 moving in x, sheared at
    z = 20.  The time functions are scaled to the run: the Ricker pulse peaks at 0.4 T, the face moves by 0.01 sin(2 pi t / T)."""
    from fenicssolver_amd.fem import BoxMesh, RectangleMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, MeshFunction, near
    from fenicssolver_amd import SolverBase as SB
    T = dt * steps
    bcs = OrderedDict()
    moves = moving and kind != "cantilever"
    amp = 0.01 if moves else 0.0
    tf = {'time_function': lambda t: math.sin(2.0 * math.pi * t / T)} if moves else {}
    if kind == "cantilever":
        mesh = BoxMesh(Point(0, 0, 0), Point(4, 1, 1), 8, 3, 3)
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0.0, 0.0, 0.0))}
        bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 4.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': Constant((0.0, 0.0, -1.0 if loaded else 0.0))}
        rec = [(4.0, 1.0, 1.0), (2.0, 0.5, 0.4), (0.0, 0.0, 0.0)]          # the last one sits on the fixed face
    elif kind == "rectangle":
        mesh = RectangleMesh(Point(0, 0), Point(2, 1), 16, 8)
        bcs["fixed"] = dict({'boundary': AutoSubDomain(lambda x: near(x[1], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                             'value': Constant((amp, 0.0))}, **tf)
        bcs["punch"] = {'boundary': AutoSubDomain(lambda x: near(x[1], 1.0) and 0.5 - 1e-12 <= x[0] <= 1.5 + 1e-12), 'boundary_id': 2,
                        'type': 'stress', 'value': Constant((0.0, -1.0 if loaded else 0.0))}
        rec = [(1.0, 1.0), (0.3, 0.5), (2.0, 0.0)]                         # the last one sits on the moving edge
    else:
        mesh = _xml_mesh()
        bcs["fixed"] = dict({'boundary': AutoSubDomain(lambda x: near(x[2], 0.0)), 'boundary_id': 1, 'type': 'Dirichlet',
                             'value': Constant((amp, 0.0, 0.0))}, **tf)
        bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 20.0)), 'boundary_id': 2, 'type': 'stress',
                      'value': Constant((1.0 if loaded else 0.0, 0.0, 0.0))}
        rec = [(10.0, 5.0, 20.0), (5.0, 2.0, 10.0), (0.0, 0.0, 0.0)]
    d = mesh.coordinates().shape[1]
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'solid', 'elastic_modulus': E_, 'poisson_ratio': NU_, 'density': RHO_, 'thermal_expansion_coefficient': 0.0}
    if kind == "xml":
        s['material']['elastic_modulus'] = {'near': {'subdomain_id': 1, 'value': E_}, 'far': {'subdomain_id': 2, 'value': 0.6 * E_}}
        s['material']['density'] = {'near': {'subdomain_id': 1, 'value': RHO_}, 'far': {'subdomain_id': 2, 'value': 2.5 * RHO_}}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['report_settings'] = dict(QUIET, **(report or {}))
    s['solver_settings']['transient_settings'] = {'transient': True, 'starting_time': 0.0, 'time_step': dt, 'ending_time': steps * dt}
    s['solver_settings']['dynamics_settings'] = dict({'scheme': 'explicit', 'rayleigh_mass': 0.4}, **(dynamics or {}))
    if loaded:
        s['load_time_function'] = {'type': 'ricker', 'frequency': 2.5 / T, 'delay': 0.4 * T}
    if receivers:
        s['receivers'] = rec
    sub = MeshFunction("size_t", mesh, d)
    axis, mid = (2, 10.0) if kind == "xml" else (0, 2.0 if kind == "cantilever" else 1.0)
    sub.array()[:] = np.where(mesh.coordinates()[mesh.cells().astype(np.int64)].mean(axis=1)[:, axis] < mid, 1, 2)
    return s, sub


def _solver(kind, dt, steps, **kw):
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    s, sub = _case(kind, dt, steps, **kw)
    solver = ElastodynamicsSolver(s)
    solver.subdomains = sub
    return solver


@functools.lru_cache(maxsize=None)
def _probe(kind):
    """(both step bounds, omega, Phi, K, m, the Dirichlet dofs) of an unloaded case with a fixed face: Phi diag(m)-orthonormal and zero
    on the Dirichlet dofs.  Computed once and shared; nobody changes it."""
    solver = _solver(kind, 1e-9, 1, loaded=False, moving=False)
    bounds = solver.time_step_bounds()
    Kh, m = _host_csr(solver._K), solver._mass.copy()
    dofs, _ = solver._dirichlet
    om = Phi = None
    if kind != "xml":
        Kd = Kh.toarray()
        free = np.setdiff1d(np.arange(Kd.shape[0]), dofs)
        lam, vec = scipy.linalg.eigh(Kd[np.ix_(free, free)], np.diag(m[free]))
        Phi = np.zeros((Kd.shape[0], len(free)))
        Phi[free] = vec
        om = np.sqrt(lam)
    solver.close()
    return bounds, om, Phi, Kh, m, np.asarray(dofs)


def _record_steps(monkeypatch, sf_of):
    """every (u_n, w_n, v_n, a_n) the marcher reaches after an advance call, in device order; sf_of() gives the run's load factors"""
    from fenicssolver_amd import backend
    states = []
    advance = backend.ExplicitDynamicsState.advance

    def recording(self, K, *a, **k):
        out = advance(self, K, *a, **k)
        u, w, n = self.get()
        v, acc = self.full_step(K, sf_of()[n])
        states.append((n, u, w, v, acc))
        return out
    monkeypatch.setattr(backend.ExplicitDynamicsState, "advance", recording)
    return states


# ---- 3. the solver against the reference marcher, step by step ------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle", "xml"])
def test_solver_matches_the_reference_marcher_step_by_step(monkeypatch, kind):
    steps = 40
    dt = 0.5 * _probe(kind)[0][0]
    solver = _solver(kind, dt, steps, dynamics={'batch_steps': 1})
    sf, sg = solver.time_factors()
    states = _record_steps(monkeypatch, lambda: sf)
    u_last = solver.solve().vector()._values().copy()
    assert solver.function_space.localizer() is None                       # device order = host order
    u0, v0 = solver.initial_fields()
    dofs, vals = solver._dirichlet
    Kh = _host_csr(solver._K)
    ref = xr.march(Kh, solver._mass, solver._load, u0, v0, dt, steps, eta_m=0.4, sf=sf, dofs=dofs, g=vals, sg=sg)
    assert [s[0] for s in states] == list(range(2, steps + 1)) and len(ref) == steps + 1
    d = solver.dimension
    worst = {"u": 0.0, "v": 0.0, "a": 0.0}
    for n, u, w, v, a in states:
        for k, field in (("u", u), ("v", v), ("a", a)):
            worst[k] = max(worst[k], np.abs(field - ref[n][k]).max() / np.abs(ref[n][k]).max())
    rv = solver.receiver_vertices
    rdofs = (rv[:, None] * d + np.arange(d)[None, :]).ravel()
    tr_ref = np.stack([s['u'][rdofs].reshape(-1, d) for s in ref])
    tr = solver.receiver_traces()
    worst["traces"] = np.abs(tr - tr_ref).max() / np.abs(tr_ref).max()
    print("\nexplicit solver against the reference marcher, %s (%d dofs, dt = %.4g): largest relative difference over %d steps %s" % (
        kind, len(u0), dt, steps, {k: "%.2e" % v for k, v in worst.items()}))
    assert tr.shape == (steps + 1, 3, d) and np.array_equal(tr[0], tr_ref[0])
    # it moves: the load arrives (and the face drives the body)
    assert np.abs(ref[-1]['u']).max() > 1e-6 and np.abs(tr[-1, 0]).max() > 0.0
    assert np.array_equal(u_last, states[-1][1])
    assert np.array_equal(solver.velocity().vector()._values(), states[-1][3])
    assert np.array_equal(solver.acceleration().vector()._values(), states[-1][4])
    # one batch for the whole run gives the same bits as 39 batches of one step
    monkeypatch.undo()
    monkeypatch.setenv("FS_RENUMBER", "0")
    whole = _solver(kind, dt, steps)
    assert np.array_equal(whole.solve().vector()._values(), u_last) and np.array_equal(whole.receiver_traces(), tr)
    assert np.array_equal(whole.velocity().vector()._values(), states[-1][3])
    assert [(s['first_step'], s['steps']) for s in whole.step_stats] == [(1, steps - 1)]
    for k in worst:
        assert worst[k] <= MARCH_TOL[k], (k, worst[k])
    solver.close()
    whole.close()


# ---- 4. single modes -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind, k", [("cantilever", 0), ("cantilever", 7), ("rectangle", 2)])
def test_a_single_mode_marches_at_the_discrete_frequency(monkeypatch, kind, k):
    """u_0 = phi_k, v_0 = 0 over the 24 intervals of 0.2 / omega_k, against phi_k cos(omega_h n dt).  For these modes 0.2 / omega_k lies
    above both step bounds of the mesh (the figure is printed), where the solver refuses to march and the scheme blows up; each interval
    is therefore taken as q equal substeps, the fewest that bring dt to 0.5 x critical_time_step() or below, and EVERY substep is held
    against the closed form of its own dt."""
    bounds, om, Phi, Kh, m, dofs = _probe(kind)
    phi, amp = Phi[:, k], np.abs(Phi[:, k]).max()
    q = max(1, int(math.ceil((0.2 / om[k]) / (0.5 * bounds[0]))))
    dt, steps = 0.2 / om[k] / q, 24 * q
    solver = _solver(kind, dt, steps, loaded=False, moving=False, dynamics={'rayleigh_mass': 0.0}, receivers=False)
    solver.initial_values = {'displacement': phi}
    # every step through the receivers of the library: all dofs of three vertices where the mode is large, and the last field
    top = np.argsort(-np.abs(phi).reshape(-1, solver.dimension).max(axis=1))[:3]
    solver.settings['receivers'] = [tuple(solver.mesh.coordinates()[v]) for v in top]
    u_end = solver.solve().vector()._values()
    oh = xr.discrete_frequency(om[k], dt)
    d = solver.dimension
    rdofs = (solver.receiver_vertices[:, None] * d + np.arange(d)[None, :]).ravel()
    tr = solver.receiver_traces().reshape(steps + 1, -1)
    closed = phi[rdofs][None, :] * np.cos(oh * dt * np.arange(steps + 1))[:, None]
    err = max(np.abs(tr - closed).max(), np.abs(u_end - phi * math.cos(oh * steps * dt)).max()) / amp
    print("\nmode %d of the %s (omega = %.4g): 0.2 / omega = %.4g is %.1f x the stable bound %.4g (upper bound %.4g): %d substeps per interval, "
          "dt = %.4g, %d steps; largest deviation from phi cos(omega_h n dt) %.2e of max |phi|" % (
              k, kind, om[k], 0.2 / om[k], 0.2 / om[k] / bounds[0], bounds[0], bounds[1], q, dt, steps, err))
    assert len(solver.step_stats) == 1 and solver.step_stats[0]['steps'] == steps - 1
    assert abs(math.cos(oh * steps * dt)) < 0.5                            # the run covers a good part of the period: 4.8 rad
    assert err <= MODE_TOL
    solver.close()


# ---- 5. the discrete energy ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle"])
def test_energy_is_conserved_undamped_and_dissipated_by_the_mass_damping(monkeypatch, kind):
    bounds, om, Phi, Kh, m, dofs = _probe(kind)
    u0 = Phi[:, :6] @ np.array([1.0, -0.7, 0.5, 0.4, -0.3, 0.2])
    steps, dt = 200, 0.5 * bounds[0]
    solver = _solver(kind, dt, steps, loaded=False, moving=False, dynamics={'rayleigh_mass': 0.0, 'energy_freq': 1}, receivers=False)
    solver.initial_values = {'displacement': u0}
    solver.solve()
    en = solver.energy()
    shape_ok = en.shape == (steps, 3) and np.array_equal(en[:, 0], np.arange(1, steps + 1))   # no step-0 row
    E = en[:, 1] + en[:, 2]
    drift = np.abs(E - E[0]).max() / E[0]
    n_batches = len(solver.step_stats)
    solver.close()
    # damped: E_{n+1/2} - E_{n-1/2} = -eta_M dt v_n^T diag(m) v_n, v_n = (w_{n-1/2} + w_{n+1/2}) / 2, from the states of every step
    eta = 0.5
    solver = _solver(kind, dt, steps, loaded=False, moving=False, dynamics={'rayleigh_mass': eta, 'energy_freq': 1}, receivers=False)
    solver.initial_values = {'displacement': u0}
    states = _record_steps(monkeypatch, lambda: np.ones(steps + 1))
    solver.solve()
    en = solver.energy()
    Ed = en[:, 1] + en[:, 2]
    ws = {n: w for n, u, w, v, a in states}
    loss = np.array([eta * dt * float(np.sum(m * (0.5 * (ws[n] + ws[n + 1])) ** 2)) for n in range(2, steps)])
    defect = np.abs(np.diff(Ed)[1:] + loss).max() / Ed[0]
    print("\ndiscrete energy of the explicit scheme, %s, %d steps of %.4g: drift %.2e of E_0; eta_M = %g: defect of the dissipation identity "
          "%.2e of E_0, E_end / E_0 = %.4f" % (kind, steps, dt, drift, eta, defect, Ed[-1] / Ed[0]))
    assert shape_ok and n_batches == steps - 1                             # a batch ends at every energy step
    assert en[:, 1].max() > 0.05 * E[0]                                    # the energy does change hands
    assert np.all(np.diff(Ed) < 0.0)                                       # strictly decreasing: a condition, not a measurement
    assert drift <= ENERGY_DRIFT_TOL and defect <= ENERGY_DEFECT_TOL
    solver.close()


# ---- 6. the step bounds ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["cantilever", "rectangle"])
def test_step_bounds_bracket_the_true_limit_and_a_step_above_them_is_refused(monkeypatch, kind):
    from fenicssolver_amd import backend
    from fenicssolver_amd.SolverBase import SolverError
    bounds, om, Phi, Kh, m, dofs = _probe(kind)
    true = 2.0 / om[-1]
    print("\n%s: 2/sqrt(lambda_G) = %.6g <= 2/omega_max = %.6g <= 2/sqrt(lambda_P) = %.6g" % (kind, bounds[0], true, bounds[1]))
    assert bounds[0] <= true <= bounds[1]
    # eta_M does not move the bounds
    damped = _solver(kind, 1e-9, 1, loaded=False, moving=False, dynamics={'rayleigh_mass': 5.0})
    assert damped.time_step_bounds() == bounds and damped.critical_time_step() == bounds[0]
    damped.close()
    # 1.05 x the upper bound: refused before any marching call
    calls = []
    for name in ("start", "advance", "set"):
        fn = getattr(backend.ExplicitDynamicsState, name)
        monkeypatch.setattr(backend.ExplicitDynamicsState, name, lambda self, *a, _fn=fn, _n=name, **k: (calls.append(_n), _fn(self, *a, **k))[1])
    solver = _solver(kind, 1.05 * bounds[1], 10)
    with pytest.raises(SolverError, match=r"exceeds 2/sqrt\(lambda_P\) = .* the stable bound 2/sqrt\(lambda_G\) is "):
        solver.solve()
    assert calls == [] and (solver.state is None or solver.state.get()[2] == 0)
    solver.close()
    # between the two bounds: a warning, and the march runs (the step is below the true limit of this mesh)
    if 1.001 * bounds[0] < 0.98 * true:
        warned = []
        solver = _solver(kind, 0.5 * (bounds[0] + 0.98 * true), 5)
        monkeypatch.setattr(solver.logger, "warning", lambda *a, **k: warned.append(a))
        solver.solve()
        assert len(warned) == 1 and "lies between" in warned[0][0]
        solver.close()


# ---- 7. build discipline and the refusals of the library -------------------------------------------------------------------------
def test_no_operator_is_built_and_a_batch_is_one_call(monkeypatch):
    from fenicssolver_amd import backend
    kind, steps = "cantilever", 40
    dt = 0.5 * _probe(kind)[0][0]
    events = []
    for name in ("advance", "get", "full_step"):
        fn = getattr(backend.ExplicitDynamicsState, name)
        monkeypatch.setattr(backend.ExplicitDynamicsState, name, lambda self, *a, _fn=fn, _n=name, **k: (events.append(_n), _fn(self, *a, **k))[1])
    amg = []
    monkeypatch.setattr(backend.DeviceMatrix, "apply_dirichlet", lambda self, *a, **k: amg.append("eliminate"))
    solver = _solver(kind, dt, steps, dynamics={'energy_freq': 10, 'batch_steps': 7})
    solver.solve()
    assert solver.operator_assemblies == 0 and solver.amg_setups == 0 and amg == [] and getattr(solver, '_amg_cache', None) is None
    # batches: 1 -> 8 -> 10 -> 17 -> 20 -> 27 -> 30 -> 37 -> 40; the fields come to the host after the start and at the end only
    assert [(s['first_step'], s['steps']) for s in solver.step_stats] == [(1, 7), (8, 2), (10, 7), (17, 3), (20, 7), (27, 3), (30, 7), (37, 3)]
    assert events == ["get"] + ["advance"] * 8 + ["get", "full_step"]
    assert all(s['device_ms'] > 0.0 and s['ms_per_step'] == s['device_ms'] / s['steps'] for s in solver.step_stats)
    assert np.array_equal(solver.energy()[:, 0], [10, 20, 30, 40])
    solver.close()


def test_a_blow_up_names_the_step_range_and_both_bounds(monkeypatch):
    """a field that leaves the finite numbers (here: put there through the state, not by an unstable step) is found by the energy of
    its batch and reported with the steps of the batch and both bounds"""
    from fenicssolver_amd import backend
    from fenicssolver_amd.SolverBase import SolverError
    bounds = _probe("rectangle")[0]
    solver = _solver("rectangle", 0.5 * bounds[0], 12, dynamics={'batch_steps': 4})
    advance = backend.ExplicitDynamicsState.advance
    calls = []

    def poisoned(self, K, *a, **k):
        calls.append(1)
        if len(calls) == 2:                                                # the batch of steps 5 .. 9
            u, w, n = self.get()
            u[5] = np.nan
            self.set(u, w, n)
        return advance(self, K, *a, **k)
    monkeypatch.setattr(backend.ExplicitDynamicsState, "advance", poisoned)
    with pytest.raises(SolverError, match=r"not finite in steps 5 \.\. 9 .*2/sqrt\(lambda_G\) = .*2/sqrt\(lambda_P\) = ") as e:
        solver.solve()
    assert "%.6g" % bounds[0] in str(e.value) and "%.6g" % bounds[1] in str(e.value)
    solver.close()


def test_library_refusals_leave_the_state_unchanged():
    from fenicssolver_amd import backend, _lib as L
    import ctypes as C
    backend.init()
    mesh = backend.DeviceMesh.box(2, 2, 2)
    V, V1, V2 = backend.DeviceSpace(mesh, 3, 1), backend.DeviceSpace(mesh, 1, 1), backend.DeviceSpace(mesh, 3, 2)
    Vb = backend.DeviceSpace(backend.DeviceMesh.box(3, 2, 2), 3, 1)
    n = V.n_owned
    h = C.c_void_p()
    for space, msg in ((V1, "vector CG1 spaces on tetrahedra or triangles only"), (V2, "vector CG1 spaces on tetrahedra or triangles only"),
                       (backend.DeviceDGSpace(mesh), "not built for DG spaces")):
        rc = L.load().fs_dyn_explicit_state_create(space.h, C.byref(h))
        assert rc == -1 and msg in L.load().fs_last_error().decode(), (rc, L.load().fs_last_error())
    K, Kb = backend.DeviceMatrix(V), backend.DeviceMatrix(Vb)
    K.assemble(lame=(MU_, LM_))
    Kb.assemble(lame=(MU_, LM_))
    st = backend.ExplicitDynamicsState(V)
    rng = np.random.default_rng(1)
    u, w, F = (rng.standard_normal(n) for _ in range(3))
    m = rng.uniform(0.5, 2.0, n)

    def refused(call, msg):
        with pytest.raises(backend.BackendError, match=msg) as e:
            call()
        assert e.value.rc == -1                                             # FS_ERR_INVALID

    refused(lambda: st.start(K, u, w), "was not configured")
    refused(lambda: st.advance(K, [1.0], [1.0]), "was not configured")
    refused(lambda: st.full_step(K, 1.0), "was not configured")
    dt = 1e-3
    st.configure(dt, 0.1, m, load=F, dirichlet_dofs=[0, 4], dirichlet_values=[1.0, 2.0])
    refused(lambda: st.advance(K, [1.0], [1.0]), "holds no")
    refused(lambda: st.full_step(K, 1.0), "holds no")
    st.set(u, w, step=2)
    first = st.advance(K, [0.5, 0.6], [0.25, 0.3], receivers=[3, n - 1])
    before = st.get(), st.work()

    for bad_dt in (0.0, -0.1, float('inf'), float('nan')):
        refused(lambda: st.configure(bad_dt, 0.1, m), "dt > 0 and finite")
    refused(lambda: st.configure(dt, -0.1, m), "must be >= 0")
    refused(lambda: st.configure(dt, float('nan'), m), "must be >= 0")
    for bad_m in (0.0, -1.0, float('nan')):
        mb = m.copy()
        mb[5] = bad_m
        refused(lambda: st.configure(dt, 0.1, mb), "lumped mass of row 5 .* m_i > 0 is required")
    refused(lambda: st.configure(dt, 0.1, m, dirichlet_dofs=[0, n], dirichlet_values=[1.0, 1.0]), "outside the space")
    refused(lambda: st.configure(dt, 0.1, m, dirichlet_dofs=[-1], dirichlet_values=[1.0]), "outside the space")
    refused(lambda: st.start(Kb, u, w), "another space")
    refused(lambda: st.advance(Kb, [1.0], [1.0]), "another space")
    refused(lambda: st.full_step(Kb, 1.0), "another space")
    refused(lambda: st.advance(K, [1.0], [1.0], receivers=[0, n]), "receiver dof")
    refused(lambda: st.advance(K, [1.0], [1.0], receivers=[-1]), "receiver dof")
    refused(lambda: st.advance(K, [float('nan')], [1.0]), "not finite")
    refused(lambda: st.start(K, u, w, float('inf')), "not finite")
    refused(lambda: st.full_step(K, float('nan')), "not finite")
    refused(lambda: st.set(u, w, step=0), "n >= 1")
    after = st.get(), st.work()
    assert before[0][2] == after[0][2] == 4
    for x0, x1 in zip(before[0][:2] + (before[1],), after[0][:2] + (after[1],)):
        assert np.array_equal(x0, x1)
    # ... and the constants, the mass, the load and the Dirichlet rows too: the same two steps give the same bits
    st.set(u, w, step=2)
    second = st.advance(K, [0.5, 0.6], [0.25, 0.3], receivers=[3, n - 1])
    assert np.array_equal(first["traces"], second["traces"]) and np.array_equal(first["energy"], second["energy"])
    assert np.array_equal(st.get()[0], before[0][0]) and np.array_equal(st.get()[1], before[0][1])
    st.close()
