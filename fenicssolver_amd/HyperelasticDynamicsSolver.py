"""HyperelasticDynamicsSolver — explicit finite-strain dynamics on vector P1, GPU back end.

Joins the two halves the package already had: the four hyperelastic energies of NonlinearElasticitySolver (neo-Hookean,
St Venant-Kirchhoff, Mooney-Rivlin, Yeoh; quasi-static there) and the central-difference marcher of ElastodynamicsSolver
('scheme': 'explicit'; linear, not invariant under finite rotations).  The reference has neither: its NonlinearElasticitySolver
carries ``# todo: transient`` and a kinetic term with an undefined ``dt``.  The independent check is the numpy restatement
tests/hyperelastic_dynamics_reference.py.

Model: M a + C v + f_int(u) = s_f(t) F with f_int = dPi/du, Pi = int psi(F) dx, the LUMPED mass m = M 1 of the reference
configuration (``material['density']``) and C = eta_M diag(m).  The state is (u_n, w_n) with w_n = v_{n-1/2}; with alpha = eta_M dt / 2
a step n -> n+1 is, per dof,
    (1 + alpha) w_{n+1/2} = (1 - alpha) w_{n-1/2} + dt (s_f[n] F - f_int(u_n)) / m,   u_{n+1} = u_n + dt w_{n+1/2},
Dirichlet rows take u_{n+1} = g s_g[n+1], w_{n+1/2} = (u_{n+1} - u_n) / dt, and the start is a_0 = (s_f[0] F - f_int(u_0)) / m -
eta_M v_0, w_{1/2} = v_0 + dt/2 a_0.  There is no matrix to multiply: every step evaluates the internal force at the current
displacement, in ONE kernel launch that also applies the update (fs_hyper_dyn_advance; include/fenicssolver_amd.h), and the steps of
a batch run back to back on the device with no host round trip.  Loads are dead loads with their physical sign.

Settings: ``material`` as in NonlinearElasticitySolver (``hyperelastic_model`` by name or dict, numbers or per-region values,
``density``); boundaries, ``load_time_function``, a ``time_function`` on Dirichlet sides, ``initial_values`` / ``initial_velocity``,
``receivers``, ``dynamics_settings`` (``rayleigh_mass``, ``batch_steps``, ``energy_freq``; ``'scheme': 'explicit'`` may be given, nothing
else may) and the report settings as in ElastodynamicsSolver's explicit scheme: both time factors are taken at the time points
t_0 .. t_N, a 'table' holds N + 1 values.

Step bounds: ``critical_time_step()`` = 2/sqrt(lambda_G) and ``time_step_bounds()`` = (2/sqrt(lambda_G), 2/sqrt(lambda_P)) are those of
time_marching.step_bounds for the TANGENT stiffness at the initial state u_0 (fs_assemble_hyperelastic) and the lumped mass: the
tangent is assembled for the bounds only (``operator_assemblies`` counts it) and no matrix is touched during the march.  A
``time_step`` above the second bound raises SolverError before any step.  The tangent stiffens or softens as the body deforms:
``time_step_bounds(at='current')`` re-evaluates both bounds at the state held after a solve.  Nothing re-checks the step during
the march.

Results: ``solve()`` returns the last displacement; ``velocity()``, ``acceleration()`` (the full-step values, as in
ElastodynamicsSolver); ``receiver_traces()``; ``energy()`` [k, 3] = (n + 1, E_kin = 1/2 sum m w_{n+1/2}^2, Pi(u_n)) of the step
n -> n+1 for every ``energy_freq``-th step - THE POTENTIAL HALF IS TAKEN AT t_n, where the force is evaluated (the linear class
reports 1/2 u_{n+1}^T K u_n), so the conserved discrete energy is E_kin(w_{n+1/2}) + (Pi(u_n) + Pi(u_{n+1})) / 2 to second order in
dt; psi = 0 at rest for all four energies in both dimensions (in plane strain the neo-Hookean energy is taken with F33 = 1 like the
other three: the -mu/2 shift of NonlinearElasticitySolver's 2-D energy does not appear); ``internal_force()``; ``cauchy_stress()``
/ ``von_Mises()`` of the final state (fs_hyper_stress); ``step_stats`` one entry per batch: ``first_step``, ``steps``, ``device_ms``,
``ms_per_step``; ``save()`` writes u and v.

A cell that inverts (J <= 0) makes the potential energy of its step NaN on the device for every energy, so an inverted cell and a
blow-up are reported alike: SolverError naming the first bad step and both bounds (``nonfinite_steps`` = the library's count and that
step).  P2 spaces, several ranks, periodic spaces, ``transient: False``, non-uniform steps, the parameters of the implicit scheme,
``rayleigh_stiffness`` != 0, ``temperature_distribution``, ``point_source``, a density <= 0 and a table shorter than the run raise
SolverError before any device call.
"""
from __future__ import annotations

import numpy as np

from .SolverBase import SolverError
from .NonlinearElasticitySolver import NonlinearElasticitySolver
from .ElastodynamicsSolver import ElastodynamicsSolver
from . import solid_steps, time_marching


class HyperelasticDynamicsSolver(NonlinearElasticitySolver, ElastodynamicsSolver):
    _constraint_sides = False
    _not_finite = 'the state or its energy is not finite, or a cell is inverted (J <= 0),'

    def __init__(self, case_settings):
        ElastodynamicsSolver.__init__(self, case_settings)
        self.settings['mixed_variable'] = ('displacement', 'velocity', 'pressure')          # as NonlinearElasticitySolver
        self.nonfinite_steps = None
        self._hyper = None                    # (lame, model, params) in device cell order

    # ------------------------------------------------------------------ settings (host only)
    def scheme(self):
        s = self.dynamics_settings().get('scheme', 'explicit')
        if s != 'explicit':
            raise SolverError("HyperelasticDynamicsSolver: dynamics_settings: 'scheme' = {!r}: only the explicit scheme is offered "
                              "(implicit finite-strain dynamics is not built)".format(s))
        return 'explicit'

    def _refuse_unsupported(self):
        V = self.function_space
        who = 'HyperelasticDynamicsSolver'

        def space_check():
            if V.degree() != 1 or getattr(V, '_ncomp', 1) != self.dimension:
                raise SolverError(who + ': CG{} spaces with {} component(s) are not supported (vector CG1 only: the P2 integrand is not '
                                  'polynomial and a row-sum lumped P2 mass is not positive)'.format(V.degree(), getattr(V, '_ncomp', 1)))
        solid_steps.refuse_unsupported(self, who, ' (the energies have no thermal term)', ('point_source',), space_check)
        rho = self.material_field('density')
        if not (np.all(np.asarray(rho) > 0.0) and np.all(np.isfinite(rho))):
            raise SolverError(who + ": material 'density' must be positive")
        self.scheme()
        self.explicit_parameters()
        self.uniform_step()
        self.energy_freq()
        self.time_factors()               # (the time grid and every table against the length of the run)
        model, _ = self.hyperelastic_model()
        if model in ('neo_hookean', 'st_venant_kirchhoff'):
            self.lame_parameters()

    # ------------------------------------------------------------------ the device side
    def _tangent_bounds(self, u_dev):
        """both step bounds for the tangent stiffness at the displacement u_dev (device dof order) and the lumped mass"""
        from . import backend
        V = self.function_space.device()
        lame, model, params = self._hyper
        ud = backend.DeviceVector(V.n_local, solid_steps.to_device_dofs(V, None, u_dev))      # (u_dev is in device order already)
        K = backend.DeviceMatrix(V)
        try:
            info = backend.assemble_hyperelastic(V, ud, lame, K=K, model=model, params=params)
            self.operator_assemblies += 1
            if info['n_inverted']:
                raise SolverError('HyperelasticDynamicsSolver: the state inverts {} cell(s), first cell {}: its tangent gives no step '
                                  'bound'.format(info['n_inverted'], info['first_inverted_cell']))
            return time_marching.step_bounds(self, K, self._mass, self._dirichlet[0])
        finally:
            K.close()
            ud.close()

    def _setup(self):
        """m, F, the Dirichlet rows, the material, both step bounds at u_0 and the state object.  Everything here is set-up cost."""
        from . import backend
        self._refuse_unsupported()
        par = self.explicit_parameters()
        sf, sg = self.time_factors()
        u0, v0 = self.initial_fields()
        self.snap_receivers()
        form, bcs = self.generate_form(0, None, None, None, None)
        self.close()
        V = self.function_space.device()
        loc = self._loc = self.function_space.localizer()
        if loc is not None and getattr(loc, 'is_local_view', False):
            raise SolverError('HyperelasticDynamicsSolver runs on one rank')
        gdofs, gvals = self._bc_arrays(bcs)
        u0 = u0.copy()
        u0[gdofs.astype(np.int64)] = gvals * sg[0]                # the initial displacement takes the Dirichlet values of t_0
        dofs, vals = (gdofs, gvals) if loc is None else loc.dofs(gdofs, gvals)
        model, lame, params = form.model_spec()
        lame, params = solid_steps.localized(lame, loc), solid_steps.localized(params, loc)
        self._hyper = (lame, model, params)
        rho = self.material_field('density')
        if np.ndim(rho) > 0:
            rho = np.asarray(rho, dtype=np.float64)
            rho = rho if loc is None else loc.cells(rho)
        self._rho = rho
        M = backend.DeviceMatrix(V)
        M.assemble(lame=(0.0, 0.0), mass=self._density_spec(1.0))
        self._mass = self._lumped_mass(V, M)
        b = solid_steps.external_loads(self, form, V, loc)        # per dof in a fixed order: the same bits from run to run
        self._load = b.get()[:V.n_owned]
        b.close()
        self._dirichlet = (np.asarray(dofs, dtype=np.int32), np.asarray(vals, dtype=np.float64))
        self._par = par
        self._bounds = self._tangent_bounds(self._to_dev(u0))
        dt = self.uniform_step()
        self._check_step(dt)
        self.state = backend.HyperelasticDynamicsState(V, lame, model=model, params=params)
        self.state.configure(dt, par['rayleigh_mass'], self._mass, load=self._load, dirichlet_dofs=self._dirichlet[0],
                             dirichlet_values=self._dirichlet[1])
        return V, u0, v0, sf, sg, self._receiver_dofs(loc)

    def time_step_bounds(self, at='initial'):
        """(2 / sqrt(lambda_G), 2 / sqrt(lambda_P)) of the tangent stiffness and the lumped mass: stable below the first, certain to
        blow up above the second.  at='initial': the tangent at u_0 (what solve() checks ``time_step`` against); at='current': at the
        displacement the device state holds after a solve - one more tangent assembly, the state is not changed."""
        if at not in ('initial', 'current'):
            raise SolverError("HyperelasticDynamicsSolver: time_step_bounds: at is 'initial' or 'current', got {!r}".format(at))
        if at == 'current':
            if self.state is None or self.state.get()[2] < 1:
                raise SolverError("HyperelasticDynamicsSolver: time_step_bounds(at='current'): no run has been marched yet")
            return self._tangent_bounds(self.state.get()[0])
        if self._bounds is None:
            self._setup()
        return self._bounds

    # ------------------------------------------------------------------ the march (ElastodynamicsSolver._solve_explicit)
    def _march_start(self, u0d, v0d, sf0, sg0, sg1):
        self._pi0 = None
        if self.energy_freq() == 1:                               # Pi(u_0) for the energy row of the step 0 -> 1
            self.state.set(u0d, np.zeros_like(u0d), 1)
            self._pi0 = self.state.internal_force()[1]
        self.state.start(u0d, v0d, sf0, sg0, sg1)

    def _march_advance(self, sf, sg, rec):
        return self.state.advance(sf, sg, receivers=rec, traces=len(rec) > 0, energy=True, info=True)

    def _first_step_potential(self, u1):
        return float(self._pi0)

    def _publish_explicit(self, sf_n):
        u, _, _ = self.state.get()
        v, a = self.state.full_step(sf_n)
        self.w_current = self.result = self._function(u)
        self._velocity, self._acceleration = self._function(v), self._function(a)

    def solve_transient(self):
        self.nonfinite_steps = None
        return self._solve_explicit()

    def solve(self):
        self.result = self.solve_transient()
        return self.result

    # ------------------------------------------------------------------ results
    def internal_force(self):
        """f_int(u) = dPi/du of the displacement the device state holds (the last one of the run), a Function"""
        if self.state is None or self.state.get()[2] < 1:
            raise SolverError('HyperelasticDynamicsSolver: no run has been marched yet')
        return self._function(self.state.internal_force()[0])
