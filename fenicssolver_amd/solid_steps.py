"""The solve steps of the elasticity family (NonlinearElasticitySolver, PlasticitySolver, ViscoelasticitySolver and the loads of the two
dynamics classes): functions that take the solver, as time_marching's do.  damped_newton and what it needs import no back end, so the
loop that decides about convergence, halving and the commit of a history runs on the host with numpy callables
(tests/test_solid_newton_host.py); every other function imports the back end when it is called."""

from __future__ import annotations

from collections import namedtuple

import numpy as np

from .fem import SolverError
from . import forms

# solver_parameters['newton_solver'] as SolverBase._newton_settings parses it (DOLFIN's NewtonSolver defaults)
NewtonSettings = namedtuple('NewtonSettings', 'rtol atol max_it relax monitor')

# What differs between the callers of damped_newton.  name: 'hyperelastic' / 'plastic'; hint: the advice its errors end with;
# hint_always: the 'did not converge' and 'correction is not finite' errors carry the hint too; rejected(info): what a rejected state
# does, or None for "gives a non-finite residual"; monitor_tail(info): the end of the monitor line; breakdown: the CG-breakdown error
# (iteration, hint); cut_reason: what the log line of a cut step blames.
NewtonTexts = namedtuple('NewtonTexts', 'name hint hint_always rejected monitor_tail breakdown cut_reason')

HYPERELASTIC_TEXTS = NewtonTexts(
    'hyperelastic',
    'apply the load in steps: transient_settings with boundary values and loads that change from step to step '
    '(a per-step sequence or a callable of time - constant values repeat the full load at every step)',
    False,
    lambda info: ('inverts {} cell(s), first cell {}'.format(info['n_inverted'], info['first_inverted_cell'])
                  if info['n_inverted'] else None),
    lambda info: '',
    'hyperelastic Newton: CG broke down at iteration {} - the tangent is not positive definite there '
    '(a material instability, or a load step too large: {})',
    'inverted cells')

PLASTIC_TEXTS = NewtonTexts(
    'plastic',
    'apply the load in smaller steps (transient_settings with boundary values and loads that change from step to '
    'step), or give the material a hardening_modulus > 0',
    True,
    lambda info: None,
    lambda info: ', %d cells yielding' % info['n_yielded'],
    'plastic Newton: CG broke down at iteration {} - the consistent tangent is singular there (a limit '
    'load with hardening_modulus = 0): {}',
    'non-finite residual')


class NewtonRun:
    """What a damped Newton solve has done so far.  The lists grow as it goes: after an error they tell how far it got."""

    def __init__(self):
        self.iterations, self.history, self.steps, self.stats = 0, [], [], []   # steps: the step length of each iteration
        self.x = self.info = None                                                # set when the iteration has converged


def damped_newton(x0, evaluate, solve_step, settings, texts, log, on_converged=None, run=None):
    """Newton on r(x) = 0 with DOLFIN's NewtonSolver stopping test (the residual norm, absolute or relative to the first) and a step
    that is halved, at most 10 times, while the trial state is rejected.  evaluate(x) -> (info, ||r||), the norm None for a rejected
    state; it is called once for x0 and once per trial, and the last call was at the iterate returned.  solve_step(it) ->
    (correction at the last accepted state, a host array; that solve's stats entry) and may raise.  settings: NewtonSettings, texts:
    NewtonTexts, log: a logger.  on_converged(info) runs once, after convergence only.  Returns the NewtonRun (``run``, or a new one)."""
    rtol, atol, max_it, relax, monitor = settings
    run = NewtonRun() if run is None else run
    x = x0
    info, rnorm = evaluate(x)
    if rnorm is None:
        if texts.rejected(info):
            raise SolverError('{} Newton: the initial iterate (previous solution with the boundary values imposed) {}: {}'.format(
                texts.name, texts.rejected(info), texts.hint))
        raise SolverError('{} Newton: the residual of the initial iterate is not finite'.format(texts.name))
    r0 = rnorm
    run.history.append(rnorm)
    hint = ': ' + texts.hint if texts.hint_always else ''
    for it in range(max_it + 1):
        if monitor:
            log.info("Newton iteration %d: r (abs) = %.3e (tol = %.3e) r (rel) = %.3e (tol = %.3e)%s",
                     it, rnorm, atol, rnorm / r0 if r0 > 0 else 0.0, rtol, texts.monitor_tail(info))
        if rnorm < atol or (r0 > 0 and rnorm / r0 < rtol):
            break
        if it == max_it:
            raise SolverError('Newton solver did not converge in {} iterations (residual {:.3e}){}'.format(max_it, rnorm, hint))
        d, stats = solve_step(it)
        run.stats.append(stats)
        if not np.all(np.isfinite(d)):
            raise SolverError('{} Newton: the correction of iteration {} is not finite{}'.format(texts.name, it, hint))
        step = relax
        for cut in range(11):
            x_try = x + step * d
            info, rn_try = evaluate(x_try)
            if rn_try is not None:
                break
            if cut == 10:
                raise SolverError('{} Newton: at iteration {} the step, halved 10 times, still {}: {}'.format(
                    texts.name, it, texts.rejected(info) or 'gives a non-finite residual', texts.hint))
            step *= 0.5
        if step != relax:
            log.info('%s Newton: step of iteration %d cut to %g (%s at the full step)', texts.name, it, step, texts.cut_reason)
        x, rnorm = x_try, rn_try
        run.steps.append(step)
        run.history.append(rnorm)
        run.iterations = it + 1
    if on_converged is not None:
        on_converged(info)
    run.x, run.info = x, info
    return run


# ---- helpers of the device side ---------------------------------------------------------------------------------------------------
def to_device_dofs(V, loc, xh):
    """host dof values in the device's dof order (through the localizer of a mesh uploaded in locality order), padded to V.n_local"""
    xd = xh if loc is None else loc.nodes(xh)
    return np.concatenate([xd, np.zeros(V.n_local - len(xd))]) if len(xd) < V.n_local else xd


def localized(spec, loc):
    """a per-cell material spec ('cell', array in host cell order) in device cell order; any other spec, and None, as it is"""
    if spec is None or loc is None or not isinstance(spec[0], str):
        return spec
    return ('cell', loc.cells(spec[1]))


def rigid_body_solve(solver, K, rhs, u, label, operator_key=None):
    """K u = rhs for an elasticity operator: CG + AMG with the rigid-body near-null space in 3-D (the hierarchy kept under
    operator_key, None: one per call), Jacobi-CG in 2-D"""
    if solver.dimension == 3:
        solver._device_solve(K, rhs, u, label, amg=True, near_nullspace="rigid_body", operator_key=operator_key)
    else:
        solver._device_solve(K, rhs, u, label)


def refuse_unsupported(solver, who, thermal, sources=(), space_check=None):
    """The refusals the solid-mechanics classes share, in the order they fire: several ranks, periodic spaces, then the class's own
    space_check(), temperature_distribution (thermal: the class's reason, from the separator on) and the source settings named."""
    from . import parallel
    V = solver.function_space
    if parallel.world()[1] > 1:
        raise SolverError(who + ' runs on one rank')
    if (hasattr(V, 'periodic_pairs') and V.periodic_pairs() is not None) or solver.settings.get('periodic_boundary'):
        raise SolverError(who + ': periodic spaces are not supported')
    if space_check is not None:
        space_check()
    T = getattr(solver, 'temperature_distribution', None) or solver.settings.get('temperature_distribution')
    if T is not None and not (isinstance(T, (int, float)) and T == 0):
        raise SolverError(who + ': temperature_distribution is not supported' + thermal)
    for key in sources:
        if solver.settings.get(key):
            raise SolverError('{}: {} is not supported'.format(who, key))


def external_loads(solver, F, V, loc):
    """f_ext = int B.v dx + the boundary loads (dead loads, physical sign) on the device: assembled once per load step."""
    from . import backend
    b = backend.DeviceVector(V.n_owned)
    b.fill(0.0)
    if F.body_force is not None:
        backend.assemble_vector(V, b, vector_value=list(F.body_force))
    if F.body_force_nodal is not None:
        Mb = backend.DeviceMatrix(V)
        Mb.assemble(lame=(0.0, 0.0), mass=1.0)
        fh = np.ascontiguousarray(F.body_force_nodal, dtype=np.float64).reshape(-1)
        fd = backend.DeviceVector(V.n_local, to_device_dofs(V, loc, fh))
        tmp = backend.DeviceVector(V.n_owned)
        Mb.spmv(fd, tmp)
        b.axpy(1.0, tmp)
    # boundary loads: summed per dof on the host in a fixed order and added once per dof - the facet kernels scatter with atomics,
    # whose order would make f_ext, and with it every Newton iterate, differ in the last bits from run to run
    d = solver.dimension
    n_dofs = F.space.dim()
    co = solver.mesh.coordinates()[:, :d]
    dof_l, val_l = [], []
    for t in F.tractions:
        if isinstance(t, forms.NodalLoad):
            dof_l.append(np.asarray(t.dofs, dtype=np.int64))
            val_l.append(np.asarray(t.values, dtype=np.float64))
            continue
        tri = np.asarray(solver._facets_of(t.marker_id), dtype=np.int64)
        if not len(tri):
            continue
        p = co[tri]
        if tri.shape[1] == 2:                       # boundary edges of a triangle mesh
            size = np.linalg.norm(p[:, 1] - p[:, 0], axis=1)
        else:
            size = 0.5 * np.linalg.norm(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0]), axis=1)
        g = np.broadcast_to(np.asarray(t.g, dtype=np.float64), (len(tri), d))
        w = size / tri.shape[1]                     # int lambda_a ds = |facet| / (number of its vertices)
        dof_l.append((tri[:, :, None] * d + np.arange(d)[None, None, :]).ravel())
        val_l.append(np.broadcast_to((w[:, None] * g)[:, None, :], (len(tri), tri.shape[1], d)).ravel())
    if dof_l:
        total = np.bincount(np.concatenate(dof_l), weights=np.concatenate(val_l), minlength=n_dofs)
        nd_ = np.nonzero(total)[0]
        nv_ = total[nd_]
        if loc is not None:
            nd_, nv_ = loc.dofs(nd_, nv_)
        if len(nd_):
            b.add_entries(nd_, nv_)
    return b


# ---- the Newton solves ------------------------------------------------------------------------------------------------------------
def _newton_solve(solver, F, u_current, bcs, texts, assemble, rejected_count, on_converged=None):
    """Newton on r(u) = f_int(u) - f_ext = 0 by damped_newton with DOLFIN's NewtonSolver defaults and stopping test (the norm of r with
    the Dirichlet rows zeroed, absolute 1e-10 / relative 1e-9, 50 iterations, relaxation 1).  The boundary values are imposed on the
    first iterate; every correction is zero on the Dirichlet dofs.  assemble(ud, K, r) -> info evaluates tangent and internal force at
    the device vector ud in ONE call per iterate (the tangent of the converged iterate is the one unused assembly); a state with
    info[rejected_count] != 0 or a non-finite residual is rejected.  Each linear step is rigid_body_solve with a hierarchy per
    tangent.  The solver's newton_* attributes describe the solve, also one that ended in an error after its first evaluation."""
    from . import backend, parallel
    from .fem import Function
    if parallel.world()[1] > 1:
        raise SolverError('{} Newton solves run on one rank'.format(texts.name))
    V = F.space.device()
    loc = F.space.localizer()          # a mesh file uploaded in locality order: host arrays map through it
    gdofs, gvals = solver._bc_arrays(bcs)
    dofs = gdofs if loc is None else loc.dofs(gdofs, gvals)[0]
    f_ext = external_loads(solver, F, V, loc)
    K = backend.DeviceMatrix(V)
    r = backend.DeviceVector(V.n_owned)
    ud = backend.DeviceVector(V.n_local)
    du = Function(solver.function_space)

    def evaluate(xh):
        """K and r then belong to the last state evaluated: the tangent of a rejected trial is overwritten by the next one"""
        ud.set(to_device_dofs(V, loc, xh))
        info = assemble(ud, K, r)
        if info[rejected_count]:
            return info, None
        r.axpy(-1.0, f_ext)
        if dofs.size:
            backend.set_dirichlet_values(r, dofs, 0.0)
        rn = float(np.sqrt(r.dot(r)))
        return info, (rn if np.isfinite(rn) else None)

    def solve_step(it):
        rhs = backend.DeviceVector(V.n_owned)
        rhs.axpy(-1.0, r)
        if dofs.size:
            K.apply_dirichlet(rhs, dofs, 0.0, symmetric=True)     # the correction is zero on the Dirichlet boundary
        try:
            rigid_body_solve(solver, K, rhs, du, texts.name + ' Newton step')
        except (SolverError, backend.BackendError) as e:
            st = solver.last_solve_stats or {}
            if isinstance(e, backend.BackendError) and getattr(e, 'rc', None) == -6 or \
                    (isinstance(e, SolverError) and st.get('converged', 0) < 0):      # FS_ERR_NUMERIC: CG breakdown
                raise SolverError(texts.breakdown.format(it, texts.hint)) from e
            raise
        st = solver.last_solve_stats
        return du.vector()._values(), {'krylov_iterations': st['iterations'], 'solve_ms': st['solve_ms'],
                                       'amg_setup_ms': st.get('amg_setup_ms', 0.0)}

    x = u_current.vector()._values().copy()
    if gdofs.size:
        x[gdofs] = gvals                                # the first iterate carries the boundary values
    run = NewtonRun()
    try:
        damped_newton(x, evaluate, solve_step, solver._newton_settings(), texts, solver.logger, on_converged, run)
    finally:
        if run.history:                                 # (a rejected first iterate leaves the record of the solve before)
            solver.newton_iterations, solver.newton_history = run.iterations, run.history
            solver.newton_steps, solver.newton_stats = run.steps, run.stats
    u_current.vector().set_local(run.x)
    return u_current


def hyperelastic_newton(solver, F, u_current, bcs):
    """solve(F == 0, u, bcs, J=J) of NonlinearElasticitySolver (:90-98).  Tangent, internal force and inverted cells come from
    fs_assemble_hyperelastic (a per-cell material is uploaded once per iterate); a trial iterate with an inverted cell (J <= 0) or a
    non-finite residual is halved."""
    from . import backend
    V, loc = F.space.device(), F.space.localizer()
    model, lame, params = F.model_spec()             # the energy and its material: Lame parameters or a parameter table
    lame, params = localized(lame, loc), localized(params, loc)
    return _newton_solve(solver, F, u_current, bcs, HYPERELASTIC_TEXTS, lambda ud, K, r: backend.assemble_hyperelastic(
        V, ud, lame, K=K, r=r, model=model, params=params), 'n_inverted')


def plastic_newton(solver, F, u_current, bcs):
    """One load step of PlasticitySolver: r(u) = f_int(u; committed history) - f_ext.  Return mapping, consistent tangent and internal
    force are evaluated on the device in one call per iterate (fs_assemble_plasticity) from the history committed by the previous
    step, and the trial history belongs to the last state evaluated; the loop only decides about convergence.  A trial iterate with a
    non-finite residual is halved.  The history is committed when the step has converged and not otherwise: an error leaves the
    committed state as it was."""
    from . import backend
    V, history = F.space.device(), F.history
    material = localized(F.material_spec(), F.space.localizer())

    def commit(info):                                   # the last evaluation was at the converged iterate
        history.commit()
        solver.yielded_last_step = info['n_yielded']

    return _newton_solve(solver, F, u_current, bcs, PLASTIC_TEXTS,
                         lambda ud, K, r: backend.assemble_plasticity(V, ud, history, material, K=K, r=r), 'n_nonfinite', commit)


# ---- Prony-series viscoelasticity (ViscoelasticitySolver) -------------------------------------------------------------------------
def viscoelastic_step(solver, F, u_current, bcs):
    """One step of ViscoelasticitySolver, a single linear solve: (1) the history load -int B^T s_hist dx from the COMMITTED
    history (fs_assemble_viscoelastic), (2) K(mu_eff, lambda_eff) u = f_ext + history load with the Dirichlet values imposed -
    rigid_body_solve, (3) the per-cell update at u, (4) commit.  A solve that does not converge raises before (3): the committed
    history stays as it was.  The effective operator depends on the step length and the material only, so it is assembled once and
    kept while both (and the set of Dirichlet dofs) are unchanged, and with it the AMG hierarchy (the operator key of _device_solve):
    ``operator_assemblies`` and ``amg_setups`` count the builds.  F.steady: the long-term equilibrium - the same solve with
    mu = G0 g_inf and no history load."""
    from . import backend, parallel
    if parallel.world()[1] > 1:
        raise SolverError('viscoelastic steps run on one rank')
    V = F.space.device()
    loc = F.space.localizer()
    gdofs, gvals = solver._bc_arrays(bcs)
    dofs, vals = (gdofs, gvals) if loc is None else loc.dofs(gdofs, gvals)
    dt = 1.0 if F.steady else float(F.dt)
    history = F.history
    # the effective operator and everything derived from the material: once per (dt, material, Dirichlet set).  Forms of one
    # solve() carry the material under one token, so a step that changes nothing costs no host work per cell here.
    dof_bytes = np.asarray(dofs, dtype=np.int64).tobytes()
    ctx = getattr(solver, '_visco_ctx', None)
    token = getattr(F, 'material_token', None)
    if ctx is None or token is None or ctx['token'] is not token or ctx['steady'] != bool(F.steady) or ctx['dt'] != dt \
            or ctx['dofs'] != dof_bytes or ctx['space'] is not V:
        mu_e, lm_e = F.effective_lame(None if F.steady else F.dt)
        cellwise = np.ndim(mu_e) > 0 or np.ndim(lm_e) > 0
        lame_host = np.stack(np.broadcast_arrays(np.asarray(mu_e, dtype=np.float64), np.asarray(lm_e, dtype=np.float64)), axis=-1)
        if F.steady:                                # an elastic material with the long-term moduli, no series
            material = ('cell', lame_host) if cellwise else (float(mu_e), float(lm_e), [])
        else:
            material = F.material_spec()
        K_raw = backend.DeviceMatrix(V)
        K_raw.assemble(lame=localized(('cell', lame_host), loc) if cellwise else (float(mu_e), float(lm_e)))
        solver.operator_assemblies = getattr(solver, 'operator_assemblies', 0) + 1
        solver._visco_serial = getattr(solver, '_visco_serial', 0) + 1          # never reused: the key of the AMG hierarchy
        ctx = {'token': token, 'steady': bool(F.steady), 'dt': dt, 'dofs': dof_bytes, 'space': V, 'material': localized(material, loc),
               'K_raw': K_raw, 'K': backend.DeviceMatrix(V), 'key': ('viscoelastic', solver._visco_serial)}
        solver._visco_ctx = ctx
    material = ctx['material']
    # 1. right-hand side: loads plus the history load
    rhs = external_loads(solver, F, V, loc)
    times = {'history_load_ms': 0.0}
    if not F.steady and history.n_terms:
        info = backend.assemble_viscoelastic(V, history, material, dt, load=rhs, add=True)
        times['history_load_ms'] = info['load_ms']
    # 2. the solve; the Dirichlet rows and the lifting of their values go into a copy of the kept operator
    K = ctx['K']
    K.copy_from(ctx['K_raw'])
    if len(dofs):
        K.apply_dirichlet(rhs, dofs, vals, symmetric=True)
    rigid_body_solve(solver, K, rhs, u_current, 'viscoelastic step', operator_key=ctx['key'])
    st = solver.last_solve_stats
    if 'amg_reused' in st and not st['amg_reused']:
        solver.amg_setups = getattr(solver, 'amg_setups', 0) + 1
    x = u_current.vector()._values()
    if not np.all(np.isfinite(x)):
        raise SolverError('viscoelastic step: the displacement is not finite')
    # 3. the update, 4. commit
    ud = backend.DeviceVector(V.n_local, to_device_dofs(V, loc, x))
    info = backend.assemble_viscoelastic(V, history, material, dt, u=ud)
    if info['n_nonfinite']:
        raise SolverError('viscoelastic step: the updated stress is not finite in {} cell(s), first cell {}'.format(
            info['n_nonfinite'], info['first_nonfinite_cell']))
    history.commit()
    times.update({'update_ms': info['update_ms'], 'solve_ms': st['solve_ms'], 'krylov_iterations': st['iterations'],
                  'amg_setup_ms': st.get('amg_setup_ms', 0.0) if not st.get('amg_reused', True) else 0.0})
    solver.step_stats.append(times)
    return u_current
