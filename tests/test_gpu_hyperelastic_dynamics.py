"""HyperelasticDynamicsSolver and the fs_hyper_dyn_* kernel (fs_hyper_dynamics.hip) on the MI355X: internal force and energy against
numpy, one step row by row, the march against the reference marcher (tests/hyperelastic_dynamics_reference.py), split invariance and
repeatability bit for bit, finite rotations, the discrete energy, the small-amplitude limit, inverted cells, the step bounds and the
refusals of the library.  The host conditions these tests rest on are in test_hyperelastic_dynamics_host.py."""
import functools

import numpy as np
import pytest
import scipy.sparse as sp

import hyperelastic_dynamics_cases as hc
import hyperelastic_dynamics_reference as dr

pytestmark = pytest.mark.gpu

MODELS = dr.MODELS
FORCE_TOL = 1e-12               # set by the issue (the project's tolerance for k_hm_force): |f_dev - f_ref| <= 1e-12 max |f_ref|, energy relative
ROW_TOL = 32 * 2.0 ** -53       # set by the issue: per dof |device - numpy| <= 32 x 2^-53 x (sum of the absolute terms of that row)
ENERGY_TOL = 1e-12              # set by the issue: the energy halves of a step against numpy with the device's own fields, relative
ROTATION_TOL = 1e-12            # set by the issue: |u - u_0| / max |u_0| and both energy halves / the linear class's energy

# Measured on the MI355X (this file: the tests print every figure before they assert), and the bounds derived from them: 10 x the
# measured figure.  Solver against the reference marcher, 40 steps of 0.5 x critical_time_step() at finite amplitude, GPU minus reference
# relative to the largest entry of the reference field at that step, largest over the steps as (u, v, a, traces):
#   cantilever 8 x 3 x 3, Ricker tip load, neo-Hookean                       6.25e-14  6.48e-14  1.50e-13  1.54e-15
#   cantilever 8 x 3 x 3, Ricker tip load, St Venant-Kirchhoff               1.52e-13  7.33e-14  1.71e-13  2.53e-15
#   rectangle 16 x 8, moving Dirichlet side, Mooney-Rivlin                   2.25e-15  4.81e-15  3.44e-14  9.97e-16
#   tests/golden/data/mesh.xml, two regions, Yeoh                            2.85e-15  8.12e-15  4.98e-14  1.03e-15
# All below the 1e-11 above which the issue asks for an explanation.  The cantilever's figures are a hundred times those of the linear
# marcher's test because they are taken per step, relative to that step's own field, and the Ricker pulse starts from a load of
# 1e-3 of its peak, so the first steps hold tiny strains: there P(F) = mu (F - F^-T) + .. is a difference of terms of size mu whose
# rounding error, eps mu, is large against the result (1e-13 of it at a strain of 1e-3) - in numpy as on the device.  Where the body
# is driven from the first step (the two moving sides) and in the traces, which are relative to the whole run, the figures are close
# to those of the linear marcher.
MARCH_MEASURED = {"u": 1.52e-13, "v": 7.33e-14, "a": 1.71e-13, "traces": 2.53e-15}
MARCH_TOL = {k: 10 * v for k, v in MARCH_MEASURED.items()}


@pytest.fixture(autouse=True)
def _file_order(monkeypatch):
    monkeypatch.setenv("FS_RENUMBER", "0")                                  # a file mesh in file order: device order = host order


def _args(model, rows):
    """(lame, model, params) of backend.HyperelasticDynamicsState for one row p[4] or per-cell rows [nc, 4]"""
    rows = np.asarray(rows, dtype=np.float64)
    cell = rows.ndim == 2
    if model in ("st_venant_kirchhoff", "neo_hookean"):
        return {"lame": ("cell", np.ascontiguousarray(rows[:, :2])) if cell else (float(rows[0]), float(rows[1])), "model": model}
    n = 3 if model == "mooney_rivlin" else 4
    return {"lame": None, "model": model, "params": ("cell", np.ascontiguousarray(rows[:, :n])) if cell else tuple(float(x) for x in rows[:n])}


def _device(mesh):
    from fenicssolver_amd.fem import VectorFunctionSpace
    from fenicssolver_amd import backend
    backend.init()
    V = VectorFunctionSpace(mesh, "Lagrange", 1)
    assert V.localizer() is None                                           # device order = host order
    return V, V.device()


def _box(n=(4, 3, 3), p1=(1.0, 0.8, 0.6)):
    from fenicssolver_amd.fem import BoxMesh, Point
    return BoxMesh(Point(0, 0, 0), Point(*p1), *n)


def _rect(n=(6, 5), p1=(1.0, 0.7)):
    from fenicssolver_amd.fem import RectangleMesh, Point
    return RectangleMesh(Point(0, 0), Point(*p1), *n)


def _cube(n):
    from fenicssolver_amd.fem import UnitCubeMesh
    return UnitCubeMesh(n, n, n)


def _smooth_u(co, d, amp=0.05):
    """the smooth finite displacement of test_gpu_hyperelastic_models.py"""
    x = co[:, :d]
    u = np.stack([amp * np.sin(1.3 * x[:, 0] + 0.7 * x[:, 1]) + 0.3 * amp * x[:, 1] ** 2,
                  amp * np.cos(0.9 * x[:, 0] - 1.1 * x[:, 1])] + ([amp * x[:, 0] * x[:, 2] + 0.5 * amp * np.sin(2 * x[:, 2])] if d == 3 else []),
                 axis=1)
    return u.ravel()


def _random_rows(model, nc, seed):
    r = np.random.default_rng(seed).random((nc, 4))
    if model in ("st_venant_kirchhoff", "neo_hookean"):
        return np.stack([1.0 + r[:, 0], 2.0 + r[:, 1], 0 * r[:, 2], 0 * r[:, 3]], axis=1)
    if model == "mooney_rivlin":
        return np.stack([0.5 + 0.5 * r[:, 0], 0.2 + 0.2 * r[:, 1], 4.0 + r[:, 2], 0 * r[:, 3]], axis=1)
    return np.stack([0.6 + 0.4 * r[:, 0], -0.1 + 0.05 * r[:, 1], 0.03 + 0.02 * r[:, 2], 5.0 + r[:, 3]], axis=1)


def _held(dV, model, rows, u, m=None):
    """a configured state that holds (u, 0), n = 1"""
    from fenicssolver_amd import backend
    st = backend.HyperelasticDynamicsState(dV, **_args(model, rows))
    st.configure(1e-3, 0.0, np.ones(dV.n_owned) if m is None else m)
    st.set(u, np.zeros(dV.n_owned), 1)
    return st


# ---- 1. internal force and energy against numpy ----------------------------------------------------------------------------------
@pytest.mark.parametrize("model,d", [(m, d) for m in MODELS for d in (3, 2)])
def test_internal_force_and_energy_match_numpy(model, d):
    mesh = _box() if d == 3 else _rect()
    V, dV = _device(mesh)
    u = _smooth_u(mesh.coordinates(), d)
    rows = _random_rows(model, mesh.num_cells(), 5)
    f_ref, e_ref, J = dr.Body(mesh.coordinates(), mesh.cells(), model, rows).force_energy(u)
    assert J.min() > 0.5
    st = _held(dV, model, rows, u)
    f, e = st.internal_force()
    f2, e2 = st.internal_force()
    errs = np.abs(f - f_ref).max() / np.abs(f_ref).max(), abs(e - e_ref) / abs(e_ref)
    print("\n%s d=%d: relative errors force %.2e energy %.2e" % ((model, d) + errs))
    assert np.array_equal(f, f2) and e == e2
    assert max(errs) <= FORCE_TOL
    st.close()
    # one constant row against per-cell rows that hold the same constants: bit for bit
    out = []
    for r in (hc.row(model), np.tile(hc.row(model), (mesh.num_cells(), 1))):
        st = _held(dV, model, r, u)
        out.append(st.internal_force())
        st.close()
    assert np.array_equal(out[0][0], out[1][0]) and out[0][1] == out[1][1] and np.abs(out[0][0]).max() > 0.0


# ---- 2. one step, row by row -------------------------------------------------------------------------------------------------------
def _update_reference(u, w, y, m, F, g, is_d, dt, eta, sf, sg):
    """(w+, sum of its absolute terms, u+, sum of its absolute terms) of one step, term by term; y = f_int(u)"""
    al = 0.5 * eta * dt
    wn = ((1 - al) * w + dt * (sf * F - y) / m) / (1 + al)
    s_w = (np.abs((1 - al) * w) + dt * (np.abs(sf * F) + np.abs(y)) / m) / (1 + al)
    un, s_u = u + dt * wn, np.abs(u) + dt * s_w
    ud = g * sg
    un, s_u = np.where(is_d, ud, un), np.where(is_d, np.abs(ud), s_u)
    wn, s_w = np.where(is_d, (ud - u) / dt, wn), np.where(is_d, (np.abs(ud) + np.abs(u)) / dt, s_w)
    return wn, s_w, un, s_u


@pytest.mark.parametrize("n_cube", [2, 8])
@pytest.mark.parametrize("model", MODELS)
def test_one_step_matches_numpy_row_by_row(model, n_cube):
    """the device's own internal_force(), u, w, m, F and flags in the numpy update formula.  2 x 2 x 2 cells: 81 dofs, one workgroup;
    8 x 8 x 8 cells: 729 nodes in three workgroups, the smallest shape at which an in-place update of u would be read across workgroups"""
    from fenicssolver_amd import backend
    mesh = _cube(n_cube)
    V, dV = _device(mesh)
    n = dV.n_owned
    assert n == (81 if n_cube == 2 else 2187)
    rows = _random_rows(model, mesh.num_cells(), 11) if n_cube == 8 else hc.row(model, 0.05)
    body = dr.Body(mesh.coordinates(), mesh.cells(), model, rows)
    m = body.lumped_mass(1.0 + np.random.default_rng(3).random(mesh.num_cells()))
    rng = np.random.default_rng(200 + n)
    h = 1.0 / n_cube
    u, w, F, v0 = (rng.standard_normal(n) * s for s in (0.02 * h, 1e-1, 0.5, 1e-1))
    assert body.force_energy(u)[2].min() > 0.3
    dd = rng.choice(n - 1, size=max(n // 9, 4), replace=False).astype(np.int32)
    dofs = np.concatenate([dd, dd[:3]])                                     # some named twice: the last value holds
    vals = 0.01 * h * rng.standard_normal(len(dofs))
    g = np.zeros(n)
    is_d = np.zeros(n, dtype=bool)
    for i, val in zip(dofs, vals):
        g[i], is_d[i] = val, True
    free = np.nonzero(~is_d)[0]
    rec = np.array([dd[0], free[0], free[-2], dd[1], free[0], n - 1], dtype=np.int32)
    Fg = np.where(is_d, 0.0, F)
    dt, sf, sg, sf2 = 1e-3, 0.7, -1.3, 0.45
    st = backend.HyperelasticDynamicsState(dV, **_args(model, rows))
    lines, worst, e_worst, exact = [], 0.0, 0.0, True
    for eta in (0.0, 0.3):
        st.configure(dt, eta, m, load=F, dirichlet_dofs=dofs, dirichlet_values=vals)
        st.set(u, w, step=3)
        y = st.internal_force()[0]
        out = st.advance([sf], [sg], receivers=rec)
        u1, w1, step = st.get()
        exact &= step == 4 and out["step"] == 4
        wn, s_w, un, s_u = _update_reference(u, w, y, m, Fg, g, is_d, dt, eta, sf, sg)
        figs = {"w": (np.abs(w1 - wn) / s_w).max(), "u": (np.abs(u1 - un) / np.maximum(s_u, 1e-300)).max()}
        exact &= np.array_equal(u1[is_d], (g * sg)[is_d]) and np.array_equal(out["traces"][0], u1[rec])
        exact &= out["n_nonfinite"] == 0 and out["first_nonfinite_step"] == -1
        # the energy halves of that step: E_kin with the device's own w, Pi(u_n) against numpy
        ek, ep = out["energy"][0]
        ek_ref, ep_ref = 0.5 * float(np.sum(m * w1 * w1)), body.force_energy(u)[1]
        e_fig = max(abs(ek - ek_ref) / abs(ek_ref), abs(ep - ep_ref) / abs(ep_ref))
        # the full-step pair of the new time point: the force is recomputed, the state stays
        y2 = st.internal_force()[0]
        v, a = st.full_step(sf2)
        u1b, w1b, stepb = st.get()
        exact &= np.array_equal(u1b, u1) and np.array_equal(w1b, w1) and stepb == 4
        al = 0.5 * eta * dt
        wp = ((1 - al) * w1 + dt * (sf2 * Fg - y2) / m) / (1 + al)
        s_wp = (np.abs((1 - al) * w1) + dt * (np.abs(sf2 * Fg) + np.abs(y2)) / m) / (1 + al)
        v_ref, s_v = 0.5 * (w1 + wp), 0.5 * (np.abs(w1) + s_wp)
        a_ref, s_a = (wp - w1) / dt, (np.abs(w1) + s_wp) / dt
        figs["v"] = (np.abs(v - v_ref) / s_v)[~is_d].max()
        figs["a"] = (np.abs(a - a_ref) / s_a)[~is_d].max()
        exact &= np.array_equal(v[is_d], w1[is_d]) and not a[is_d].any()
        # the start from (u_0, v_0): the Dirichlet rows of u_0 take g s_g[0] before the force is formed
        u0 = np.where(is_d, g * sg, u)
        st.set(u0, w, step=1)
        y0 = st.internal_force()[0]
        st.start(u, v0, sf, sg, sf2)
        us, ws, steps_ = st.get()
        exact &= steps_ == 1
        a0, s_a0 = (sf * Fg - y0) / m - eta * v0, (np.abs(sf * Fg) + np.abs(y0)) / m + eta * np.abs(v0)
        w_ref, s_ws = v0 + 0.5 * dt * a0, np.abs(v0) + 0.5 * dt * s_a0
        u_ref, s_us = u0 + dt * w_ref, np.abs(u0) + dt * s_ws
        ud = g * sf2
        u_ref, s_us = np.where(is_d, ud, u_ref), np.where(is_d, np.abs(ud), s_us)
        w_ref, s_ws = np.where(is_d, (ud - u0) / dt, w_ref), np.where(is_d, (np.abs(ud) + np.abs(u0)) / dt, s_ws)
        figs["start w"] = (np.abs(ws - w_ref) / np.maximum(s_ws, 1e-300)).max()
        figs["start u"] = (np.abs(us - u_ref) / np.maximum(s_us, 1e-300)).max()
        exact &= np.array_equal(us[is_d], ud[is_d])
        lines.append("%s %d dofs eta_M = %g: largest |device - numpy| / (sum of absolute terms) per row, in units of 2^-53: %s; energy "
                     "halves against numpy, relative: %.2e" % (model, n, eta, {k: "%.2f" % (f * 2.0 ** 53) for k, f in figs.items()}, e_fig))
        worst, e_worst = max(worst, max(figs.values())), max(e_worst, e_fig)
    # a non-finite field is counted through the energy of its step, and the step is named
    ub = u.copy()
    ub[[1, n - 2]] = np.nan, np.inf
    st.set(ub, w, step=1)
    bad = st.advance([sf, sf], [sg, sg])
    print("\n" + "\n".join(lines))
    assert exact
    assert worst <= ROW_TOL
    assert e_worst <= ENERGY_TOL
    assert bad["n_nonfinite"] == 2 and bad["first_nonfinite_step"] == 0 and bad["step"] == 3
    st.close()


# ---- 3. the march against the reference marcher ------------------------------------------------------------------------------------
def _record_steps(monkeypatch, sf_of):
    """every (n, u_n, w_n, v_n, a_n) the marcher reaches after an advance call, in device order; sf_of() gives the run's load factors"""
    from fenicssolver_amd import backend
    states = []
    advance = backend.HyperelasticDynamicsState.advance

    def recording(self, *a, **k):
        out = advance(self, *a, **k)
        u, w, n = self.get()
        v, acc = self.full_step(sf_of()[n])
        states.append((n, u, w, v, acc))
        return out
    monkeypatch.setattr(backend.HyperelasticDynamicsState, "advance", recording)
    return states


@functools.lru_cache(maxsize=None)
def _critical_step(kind, model):
    s, sub = hc.march_case(kind, model, 1e-9, 1)
    solver = hc.solver_of(s, sub)
    dtc = solver.critical_time_step()
    solver.close()
    return dtc


@pytest.mark.parametrize("kind,model", [("cantilever", "neo_hookean"), ("cantilever", "st_venant_kirchhoff"), ("rectangle", "mooney_rivlin"),
                                        ("xml", "yeoh")])
def test_solver_matches_the_reference_marcher_step_by_step(monkeypatch, kind, model):
    steps = 40
    dt = 0.5 * _critical_step(kind, model)
    s, sub = hc.march_case(kind, model, dt, steps, dynamics={'batch_steps': 1})
    solver = hc.solver_of(s, sub)
    sf, sg = solver.time_factors()
    states = _record_steps(monkeypatch, lambda: sf)
    u_last = solver.solve().vector()._values().copy()
    assert solver.function_space.localizer() is None and solver.operator_assemblies == 1
    u0, v0 = solver.initial_fields()
    dofs, vals = solver._dirichlet
    body, m = hc.body_of(solver)
    mass_err = np.abs(solver._mass - m).max() / m.max()
    ref = dr.march(body, m, solver._load, u0, v0, dt, steps, eta_m=0.4, sf=sf, dofs=dofs, g=vals, sg=sg)
    assert [st[0] for st in states] == list(range(2, steps + 1)) and len(ref) == steps + 1
    d = solver.dimension
    worst = {"u": 0.0, "v": 0.0, "a": 0.0}
    for n, u, w, v, a in states:
        for k, field in (("u", u), ("v", v), ("a", a)):
            worst[k] = max(worst[k], np.abs(field - ref[n][k]).max() / np.abs(ref[n][k]).max())
    rv = solver.receiver_vertices
    rdofs = (rv[:, None] * d + np.arange(d)[None, :]).ravel()
    tr_ref = np.stack([st['u'][rdofs].reshape(-1, d) for st in ref])
    tr = solver.receiver_traces()
    worst["traces"] = np.abs(tr - tr_ref).max() / np.abs(tr_ref).max()
    strain = max(np.abs(body.deformation_gradients(st['u']) - np.eye(d)[None]).max() for st in ref)
    print("\n%s against the reference marcher, %s (%d dofs, dt = %.4g): largest relative difference over %d steps %s; lumped mass %.2e; "
          "largest |grad u| on the way %.3f, smallest J %.3f" % (model, kind, len(u0), dt, steps, {k: "%.2e" % v for k, v in worst.items()},
                                                                mass_err, strain, min(st['min_J'] for st in ref)))
    assert tr.shape == (steps + 1, 3, d) and np.array_equal(tr[0], tr_ref[0])
    assert strain > 0.01 and min(st['min_J'] for st in ref) > 0.0          # finite amplitude, nothing inverted
    assert mass_err <= 1e-13                                               # row sums of about a hundred terms each
    assert np.array_equal(u_last, states[-1][1])
    assert np.array_equal(solver.velocity().vector()._values(), states[-1][3])
    assert np.array_equal(solver.acceleration().vector()._values(), states[-1][4])
    f_last = solver.internal_force().vector()._values()
    f_host = body.force_energy(u_last)[0]
    assert np.abs(f_last - f_host).max() <= FORCE_TOL * np.abs(f_host).max()
    # the Cauchy stress of the final state is that of the static class's kernel for the same displacement
    sig = solver.cauchy_stress()
    assert sig.shape == (solver.mesh.num_cells(), 6 if d == 3 else 4) and np.all(np.isfinite(sig)) and np.abs(sig).max() > 0.0
    # one batch for the whole run gives the same bits as 39 batches of one step
    monkeypatch.undo()
    monkeypatch.setenv("FS_RENUMBER", "0")
    s, sub = hc.march_case(kind, model, dt, steps)
    whole = hc.solver_of(s, sub)
    assert np.array_equal(whole.solve().vector()._values(), u_last) and np.array_equal(whole.receiver_traces(), tr)
    assert np.array_equal(whole.velocity().vector()._values(), states[-1][3])
    assert [(b['first_step'], b['steps']) for b in whole.step_stats] == [(1, steps - 1)]
    for k in worst:
        assert worst[k] <= MARCH_TOL[k], (k, worst[k])
    solver.close()
    whole.close()


# ---- 4. split invariance and repeatability -----------------------------------------------------------------------------------------
def test_a_march_gives_the_same_bits_however_it_is_split_into_calls():
    """70 steps cross FS_MARCH_CHUNK = 64: as one call, as 1 + 69 and as 33 + 37, and once more as one call.  The odd pieces also pin
    the parity of the buffer swap across calls."""
    from fenicssolver_amd import backend
    mesh = _cube(4)
    V, dV = _device(mesh)
    n = dV.n_owned
    assert n == 375
    model = "mooney_rivlin"
    rows = 40.0 * _random_rows(model, mesh.num_cells(), 21)                # per-cell rows; wave speed about 20
    m = dr.Body(mesh.coordinates(), mesh.cells(), model, rows).lumped_mass(1.0)
    rng = np.random.default_rng(17)
    u, w, F = rng.standard_normal(n) * 2e-3, rng.standard_normal(n) * 0.5, 0.2 * rng.standard_normal(n)
    dofs = np.array([0, 1, 2, 30, 31, 0], dtype=np.int32)
    rec = np.array([0, 5, n - 1, 5], dtype=np.int32)
    steps = 70
    sf, sg = np.cos(0.1 * np.arange(steps)), 1.0 + 0.2 * np.sin(0.07 * np.arange(steps))
    st = backend.HyperelasticDynamicsState(dV, **_args(model, rows))
    st.configure(1e-3, 0.3, m, load=F, dirichlet_dofs=dofs, dirichlet_values=1e-3 * np.arange(1.0, 7.0))

    def run(cuts):
        st.set(u, w, step=1)
        outs = [st.advance(sf[a:b], sg[a:b], receivers=rec) for a, b in zip(cuts[:-1], cuts[1:])]
        uu, ww, step = st.get()
        assert step == steps + 1 and not any(o["n_nonfinite"] for o in outs)
        return uu, ww, np.concatenate([o["traces"] for o in outs]), np.concatenate([o["energy"] for o in outs])
    runs = [run(c) for c in ([0, 70], [0, 1, 70], [0, 33, 70], [0, 70])]
    whole = runs[0]
    assert np.all(np.isfinite(whole[0])) and np.abs(whole[0] - u).max() > 1e-3 and whole[2].shape == (steps, 4) and whole[3].shape == (steps, 2)
    assert np.array_equal(whole[2][:, 1], whole[2][:, 3])                  # a dof named twice is sampled twice
    assert np.all(whole[3] > 0.0)
    for other in runs[1:]:
        assert all(np.array_equal(a, b) for a, b in zip(whole, other))
    st.close()


# ---- 5. finite rotation ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_a_rotated_rest_state_stays_at_rest(model):
    """u_0 = (R - I) X + c with R a rotation by 90 degrees about a skew axis, v_0 = 0, no load, no Dirichlet rows: nothing moves and
    both energy halves vanish, relative to the energy the linear operator gives for the same u - of order one: the linear marcher
    fails this by construction"""
    from fenicssolver_amd import backend
    mesh = _cube(3)
    V, dV = _device(mesh)
    n = dV.n_owned
    rows = hc.row(model)
    body = dr.Body(mesh.coordinates(), mesh.cells(), model, rows)
    m = body.lumped_mass(hc.RHO_)
    u0 = dr.rigid_motion(body.X, (1.0, 2.0, -0.5), 0.5 * np.pi, (0.3, -0.2, 0.7))
    K = backend.DeviceMatrix(dV)
    K.assemble(lame=(hc.MU_, hc.LM_))
    rp, ci, va, shape = K.to_csr()
    e_lin = 0.5 * float(u0 @ (sp.csr_matrix((va, ci, rp), shape=shape) @ u0))
    st = backend.HyperelasticDynamicsState(dV, **_args(model, rows))
    st.configure(2e-3, 0.0, m)
    st.start(u0, np.zeros(n))
    out = st.advance(np.ones(9), np.ones(9))
    u, w, step = st.get()
    figs = (np.abs(u - u0).max() / np.abs(u0).max(), np.abs(out["energy"][:, 0]).max() / e_lin, np.abs(out["energy"][:, 1]).max() / e_lin)
    print("\n%s: after 10 steps |u - u_0| / max |u_0| %.2e, E_kin / E_lin %.2e, Pi / E_lin %.2e (E_lin = %.3g)" % ((model,) + figs + (e_lin,)))
    assert step == 10 and out["n_nonfinite"] == 0 and e_lin > 1.0
    assert max(figs) <= ROTATION_TOL
    st.close()
    K.close()


# ---- 6. the energy: second order in dt, no drift -----------------------------------------------------------------------------------
def _energy_run(model, dt, eta_m=0.0, T=0.4):
    steps = int(round(T / dt))
    solver = hc.solver_of(hc.cube_case(model, 4.0, dt, steps, eta_m=eta_m, dynamics={'energy_freq': 1}))
    solver.solve()
    rows = solver.energy()
    assert rows.shape == (steps, 3) and np.array_equal(rows[:, 0], np.arange(1, steps + 1))
    u_max = np.abs(solver.w_current.vector()._values()).max()
    solver.close()
    return dr.half_step_energy(rows[:, 1:]), rows, u_max


@pytest.mark.parametrize("model", MODELS)
def test_energy_is_second_order_in_dt_and_decreases_with_damping(model):
    """unit cube 3 x 3 x 3, E = 200, nu = 0.3, rho = 1 (or the rows with those small-strain moduli), x = 0 clamped,
    v_0 = (0, A x, A x^2 / 2) with A = 4, T = 0.4: with E_{n+1/2} = E_kin(w_{n+1/2}) + (Pi(u_n) + Pi(u_{n+1})) / 2 the largest
    |E - E_first| / E_first falls by >= 3.5 when dt is halved (the host test holds the reference marcher to the same)"""
    (E1, rows1, _), (E2, _, _) = _energy_run(model, 0.004), _energy_run(model, 0.002)
    e1, e2 = np.abs(E1 - E1[0]).max() / E1[0], np.abs(E2 - E2[0]).max() / E2[0]
    body, m, ref = hc.cube_reference(model, 4.0, 0.004, 100)
    en_ref = dr.step_energies(m, ref)
    e_fig = np.abs(rows1[:, 1:] - en_ref).max() / en_ref.max()
    Ed, _, _ = _energy_run(model, 0.004, eta_m=0.5)
    print("\n%s: max |E - E_first| / E_first %.3e (dt = 0.004) -> %.3e (dt = 0.002), ratio %.2f; energy rows against the reference "
          "marcher %.2e; damped: largest step-to-step change %.3e" % (model, e1, e2, e1 / e2, e_fig, np.diff(Ed).max()))
    assert e1 / e2 >= 3.5
    assert e_fig <= 1e-11                                                  # the same march: the issue's threshold for the march tests
    assert np.all(np.diff(Ed) < 0.0)


# ---- 7. the small-amplitude limit --------------------------------------------------------------------------------------------------
def _linear_cube(A, dt, steps):
    from fenicssolver_amd.ElastodynamicsSolver import ElastodynamicsSolver
    case = hc.cube_case("neo_hookean", A, dt, steps, dynamics={'scheme': 'explicit'})
    del case['material']['hyperelastic_model']
    return ElastodynamicsSolver(case)


@pytest.mark.parametrize("model", MODELS)
def test_small_amplitudes_approach_the_linear_marcher(model):
    """against ElastodynamicsSolver (explicit) with small_strain_moduli() and the same mass: the difference is second order in the
    amplitude, the field first order, so max |u_nl - u_lin| / max |u_lin| falls tenfold (within [8, 12]) for a tenfold smaller A"""
    dt, steps = 0.002, 100
    diffs = []
    for A in (0.04, 0.004):
        nl = hc.solver_of(hc.cube_case(model, A, dt, steps))
        mu0, lm0 = nl.small_strain_moduli()
        assert np.allclose(mu0, hc.MU_, rtol=1e-13) and np.allclose(lm0, hc.LM_, rtol=1e-13)
        u_nl = nl.solve().vector()._values().copy()
        lin = _linear_cube(A, dt, steps)
        u_lin = lin.solve().vector()._values().copy()
        assert np.abs(nl._mass - lin._mass).max() <= 1e-15 * lin._mass.max()
        diffs.append(np.abs(u_nl - u_lin).max() / np.abs(u_lin).max())
        nl.close()
        lin.close()
    print("\n%s: max |u_nl - u_lin| / max |u_lin| %.3e (A = 0.04) -> %.3e (A = 0.004), ratio %.2f" % (model, diffs[0], diffs[1], diffs[0] / diffs[1]))
    assert 8.0 <= diffs[0] / diffs[1] <= 12.0


# ---- 8. an inverted cell is reported -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("model", MODELS)
def test_an_inverted_cell_is_reported_with_its_step(model):
    """the face x = 1 driven through the face x = 0: the layer of cells behind it inverts at a time point known from the reference
    marcher.  Arithmetic only - no gather index depends on u.  St Venant-Kirchhoff stays finite there and is reported all the same."""
    from fenicssolver_amd.SolverBase import SolverError
    dt, steps = 0.004, 10
    k = dr.first_inverted_step(hc.crush_reference(model, dt, steps))
    assert k is not None and 2 <= k <= steps - 2
    solver = hc.solver_of(hc.crush_case(model, dt, steps))
    with pytest.raises(SolverError, match=r"a cell is inverted \(J <= 0\), in steps %d \.\. %d .*2/sqrt\(lambda_G\) = .*2/sqrt\(lambda_P\) = " % (k, steps)) as e:
        solver.solve()
    bounds = solver.time_step_bounds()
    print("\n%s: %s; the library counted %s" % (model, e.value, solver.nonfinite_steps))
    assert "%.6g" % bounds[0] in str(e.value) and "%.6g" % bounds[1] in str(e.value)
    assert solver.nonfinite_steps[0] > 0 and solver.nonfinite_steps[1] == k
    solver.close()


# ---- 9. the step bounds and the refusals -------------------------------------------------------------------------------------------
def test_step_bounds_are_those_of_the_tangent_at_the_initial_state(monkeypatch):
    from fenicssolver_amd import backend, time_marching
    from fenicssolver_amd.SolverBase import SolverError
    model, dt, steps = "mooney_rivlin", 0.004, 25
    solver = hc.solver_of(hc.cube_case(model, 4.0, dt, steps))
    bounds = solver.time_step_bounds()
    assert solver.critical_time_step() == bounds[0] and 0.0 < bounds[0] <= bounds[1] and solver.operator_assemblies == 1
    dV = solver.function_space.device()
    lame, name, params = solver._hyper
    K = backend.DeviceMatrix(dV)
    info = backend.assemble_hyperelastic(dV, backend.DeviceVector(dV.n_local, np.zeros(dV.n_local)), lame, K=K, model=name, params=params)
    assert info["n_inverted"] == 0
    assert time_marching.step_bounds(solver, K, solver._mass, solver._dirichlet[0]) == bounds
    K.close()
    # after a run at finite amplitude the tangent has changed, and only the bounds touch a matrix
    solver.solve()
    assert solver.operator_assemblies == 1 and solver.time_step_bounds() == bounds
    now = solver.time_step_bounds(at='current')
    print("\nstep bounds at u_0 %s, at the final state %s" % (bounds, now))
    assert solver.operator_assemblies == 2 and now != bounds and 0.0 < now[0] <= now[1]
    solver.close()
    # a step above the second bound is refused before any step
    def no_start(*a, **k):
        raise AssertionError("a step was taken")
    monkeypatch.setattr(backend.HyperelasticDynamicsState, "start", no_start)
    late = hc.solver_of(hc.cube_case(model, 4.0, 1.01 * bounds[1], 3))
    with pytest.raises(SolverError, match=r"time_step .* exceeds 2/sqrt\(lambda_P\)"):
        late.solve()
    late.close()


def test_library_refusals():
    from fenicssolver_amd import backend, _lib as L
    import ctypes as C
    backend.init()
    mesh = backend.DeviceMesh.box(2, 2, 2)
    V, V1, V2 = backend.DeviceSpace(mesh, 3, 1), backend.DeviceSpace(mesh, 1, 1), backend.DeviceSpace(mesh, 3, 2)
    n = V.n_owned
    h = C.c_void_p()
    for space, msg in ((V1, "vector CG1 spaces on tetrahedra or triangles only"), (V2, "vector CG1 spaces on tetrahedra or triangles only"),
                       (backend.DeviceDGSpace(mesh), "DG")):
        rc = L.load().fs_hyper_dyn_state_create(space.h, C.byref(h))
        assert rc == -1 and msg in L.load().fs_last_error().decode(), (rc, L.load().fs_last_error())
    rng = np.random.default_rng(1)
    u, w, F = (1e-2 * rng.standard_normal(n) for _ in range(3))
    m = rng.uniform(0.5, 2.0, n)

    def refused(call, msg):
        with pytest.raises(backend.BackendError, match=msg) as e:
            call()
        assert e.value.rc == -1                                             # FS_ERR_INVALID

    st = backend.HyperelasticDynamicsState(V, (1.0, 2.0))
    refused(lambda: st.start(u, w), "was not configured")
    refused(lambda: st.advance([1.0], [1.0]), "was not configured")
    refused(lambda: st.full_step(1.0), "was not configured")
    refused(st.internal_force, "was not configured")
    dt = 1e-3
    st.configure(dt, 0.1, m, load=F, dirichlet_dofs=[0, 4], dirichlet_values=[1e-3, 2e-3])
    refused(lambda: st.advance([1.0], [1.0]), "holds no")
    refused(lambda: st.full_step(1.0), "holds no")
    refused(st.internal_force, "holds no")
    st.set(u, w, step=2)
    first = st.advance([0.5, 0.6], [0.25, 0.3], receivers=[3, n - 1])
    before = st.get()
    for bad_dt in (0.0, -0.1, float('inf'), float('nan')):
        refused(lambda: st.configure(bad_dt, 0.1, m), "dt > 0 and finite")
    refused(lambda: st.configure(dt, -0.1, m), "must be >= 0")
    for bad_m in (0.0, -1.0, float('nan')):
        mb = m.copy()
        mb[5] = bad_m
        refused(lambda: st.configure(dt, 0.1, mb), "lumped mass of row 5 .* m_i > 0 is required")
    refused(lambda: st.configure(dt, 0.1, m, dirichlet_dofs=[0, n], dirichlet_values=[1.0, 1.0]), "outside the space")
    refused(lambda: st.advance([1.0], [1.0], receivers=[0, n]), "receiver dof")
    refused(lambda: st.advance([float('nan')], [1.0]), "not finite")
    refused(lambda: st.start(u, w, float('inf')), "not finite")
    refused(lambda: st.full_step(float('nan')), "not finite")
    refused(lambda: st.set(u, w, step=0), "n >= 1")
    after = st.get()
    assert before[2] == after[2] == 4 and np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    st.set(u, w, step=2)
    second = st.advance([0.5, 0.6], [0.25, 0.3], receivers=[3, n - 1])
    assert np.array_equal(first["traces"], second["traces"]) and np.array_equal(first["energy"], second["energy"])
    st.close()
    # a parameter row its model refuses, constant or per cell (the message names the cell), at the first call that reads the material
    nc = mesh.info()[1]
    for kw, msg in (({"lame": (-1.0, 2.0)}, "mu > 0 and lambda >= 0 are required"),
                    ({"lame": None, "model": "yeoh", "params": (1.0, 0.0, 0.0, 0.0)}, "kappa > 0 are required"),
                    ({"lame": None, "model": "mooney_rivlin", "params": (0.0, 0.0, 1.0)}, "c10 . c01 > 0"),
                    ({"lame": ("cell", np.tile([1.0, float('nan')], (nc, 1))), "model": "st_venant_kirchhoff"}, r"cell 0 \(device order\)")):
        bad = backend.HyperelasticDynamicsState(V, **kw)
        bad.configure(dt, 0.0, m)
        refused(lambda: bad.start(u, w), msg)
        bad.close()
