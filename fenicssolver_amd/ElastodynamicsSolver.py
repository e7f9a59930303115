"""ElastodynamicsSolver — structural dynamics on vector P1 / P2, GPU back end: implicit (generalized-alpha, the default) or explicit
(central differences with a lumped mass, vector P1; the last paragraph).

The reference has no transient structural solver: its ``solving_dynamics`` branch (kept as it is in LinearElasticitySolver) subtracts
rho * a with a lagged finite difference inside a static solve.  This class fills the gap with the textbook model, so there is no
reference counterpart to diff against; the independent check is the numpy / scipy restatement
tests/elastodynamics_reference.py.

Model: M a + C v + K u = s_f(t) F on a vector CG1 or CG2 space (tetrahedra, or triangles in plane strain) with the isotropic
elasticity operator K of ``lame_parameters()``, the consistent mass M of ``material_field('density')`` and Rayleigh damping
C = eta_M M + eta_K K.  The scheme is Chung-Hulbert generalized-alpha: with x_{n+1-alpha} = (1 - alpha) x_{n+1} + alpha x_n,
    M a_{n+1-am} + C v_{n+1-af} + K u_{n+1-af} = s_f(t_n + (1 - af) dt) F,
    u~ = u_n + dt v_n + dt^2 (1/2 - beta) a_n,   v~ = v_n + dt (1 - gamma) a_n,
    a_{n+1} = (u_{n+1} - u~) / (beta dt^2),       v_{n+1} = v~ + gamma dt a_{n+1}.
One number ``spectral_radius`` = rho_inf in [0, 1] sets am = (2 rho_inf - 1)/(rho_inf + 1), af = rho_inf/(rho_inf + 1),
gamma = 1/2 - am + af, beta = (1 - am + af)^2 / 4 (rho_inf = 1: the trapezoidal rule); or all four of ``alpha_m, alpha_f, beta,
gamma`` are given (Newmark: am = af = 0; HHT: am = 0).  A set outside am <= af <= 1/2, beta >= 1/4 + (af - am)/2 is not
unconditionally stable and is refused.  Solved for u_{n+1} a step is ONE linear solve with the fixed operator
    K_eff = c_M M + c_K K,   c_M = (1 - am)/(beta dt^2) + (1 - af) gamma eta_M/(beta dt),   c_K = (1 - af)(1 + gamma eta_K/(beta dt)),
whose right-hand side the device forms from (u_n, v_n, a_n) with two products (fs_dyn_predict; the formulas are in
include/fenicssolver_amd.h); fs_dyn_correct then forms a_{n+1} and v_{n+1}.  K_eff is assembled in one form, gets its Dirichlet
rows and columns eliminated once per step length, and its AMG hierarchy is built once on it (``operator_assemblies``,
``amg_setups``); no step copies or re-eliminates a matrix, and between steps u, v and a never visit the host.  The march starts from
M a_0 = s_f(t_0) F - C v_0 - K u_0 on the free rows, a_0 = 0 on the Dirichlet rows (Jacobi-CG on the eliminated M).  Each solve is
CG + AMG with the rigid-body near-null space in 3-D and Jacobi-CG in 2-D.

Settings: the material keys of LinearElasticitySolver (numbers, per region or per cell), ``density`` included;
``solver_settings['dynamics_settings']`` (or ``dynamics_settings`` at the top level) = {``spectral_radius`` (default 1.0) OR the four
explicit parameters, ``rayleigh_mass`` eta_M, ``rayleigh_stiffness`` eta_K (default 0), ``energy_freq`` (0: never)};
``initial_values['displacement']`` and ``initial_velocity``: a number, a tuple, an expression or a nodal array;
``load_time_function`` and a per-boundary ``time_function`` on Dirichlet boundaries in the spec of
WaveSolver.tabulate_time_function - loads are evaluated at t_n + (1 - af) dt (a 'table' holds one value per step), Dirichlet values
at t_{n+1} (one value per time point), and Dirichlet boundaries with non-zero values share one time function; ``receivers``: points,
each snapped to the nearest vertex, all components sampled; ``transient_settings`` with a uniform step or a ``time_series``.
Loads have their physical sign.

Results: ``solve()`` returns the last displacement; ``velocity()``, ``acceleration()``; ``receiver_traces()`` [n_steps + 1,
n_receivers, dim]; ``energy()`` [k, 3] = (step, E_kin = 1/2 v^T M v, E_pot = 1/2 u^T K u), step 0 included; ``step_stats`` per step
``predict_ms``, ``solve_ms``, ``correct_ms`` and the iterations; ``generalized_alpha_parameters()``; ``save()`` writes u and v.
Several ranks, periodic spaces, ``transient: False``, ``temperature_distribution``, ``point_source``, ``surface_source``, a density
<= 0, an unstable parameter set, both ``spectral_radius`` and explicit parameters and a table shorter than the run raise SolverError
before any device call; a non-finite state after a step raises SolverError naming the step.

``dynamics_settings['scheme']`` = ``'implicit'`` (the default: everything above) or ``'explicit'``: central differences with the
LUMPED mass m = M 1 (the row sums of the consistent mass above, formed by one product with a vector of ones; > 0 on CG1) and
C = eta_M diag(m), for impact, stress waves and short transients, where accuracy bounds the step anyway.  The state is (u_n, w_n)
with w_n = v_{n-1/2}; with y_n = K u_n and alpha = eta_M dt / 2 a step n -> n+1 is
    (1 + alpha) w_{n+1/2} = (1 - alpha) w_{n-1/2} + dt (s_f[n] F - y_n) / m,   u_{n+1} = u_n + dt w_{n+1/2},
Dirichlet rows take u_{n+1} = g s_g[n+1], w_{n+1/2} = (u_{n+1} - u_n) / dt, and the start is a_0 = (s_f[0] F - y_0) / m - eta_M v_0,
w_{1/2} = v_0 + dt/2 a_0.  A step is not a solve: one product with K and one pointwise update, and the steps of a batch run back to
back on the device with no host round trip (fs_dyn_explicit_advance; include/fenicssolver_amd.h).  There is no K_eff and no AMG:
``operator_assemblies`` and ``amg_setups`` stay 0.  Vector CG1 only (a row-sum lumped P2 mass is not positive), uniform steps only.
Keys: ``rayleigh_mass`` eta_M, ``energy_freq``, ``batch_steps`` (caps the steps of one device call; a batch also ends at the next
plot, save or energy step); ``spectral_radius``, the four generalized-alpha parameters and a ``rayleigh_stiffness`` != 0 are
refused - stiffness-proportional damping is not offered by the explicit scheme.  TIME FACTORS DIFFER FROM THE IMPLICIT SCHEME: both
s_f and s_g are taken at the time points t_0 .. t_N, so a 'table' for either holds N + 1 values, one per time POINT (the implicit
scheme keeps one value per STEP for loads).  Step bounds as in WaveSolver: ``critical_time_step()`` = 2/sqrt(lambda_G), lambda_G =
max_i sum_j |K_ij| / m_i, below which the march is stable; ``time_step_bounds()`` adds 2/sqrt(lambda_P) from 40 power iterations of
x <- diag(1/m) K x on the rows that are not Dirichlet (products on the device): a ``time_step`` above it raises SolverError before any
marching call, one between the two logs a warning; neither bound depends on eta_M.  Results: ``velocity()`` and ``acceleration()`` are
the full-step v_N = (w_{N-1/2} + w+)/2 and a_N = (w+ - w_{N-1/2})/dt with w+ the recurrence's next half-step velocity under s_f[N]
(one more product; the state is not changed; Dirichlet rows: v = w_{N-1/2}, a = 0), refreshed whenever a frame is published for plot
or save; ``receiver_traces()`` as above; ``energy()`` [k, 3] = (n + 1, E_kin = 1/2 sum m w_{n+1/2}^2, E_pot = 1/2 u_{n+1}^T K u_n) of
the step n -> n+1 for every ``energy_freq``-th step - the discrete energy lives on the half steps, so there is NO step-0 row under
this scheme; ``step_stats`` one entry per batch: ``first_step``, ``steps``, ``device_ms``, ``ms_per_step``.  A non-finite step raises
SolverError naming the step range and both step bounds.
"""
from __future__ import annotations

import math
import numbers
import os

import numpy as np

from .fem import Constant, Expression, Function, interpolate
from .SolverBase import SolverError, write_vtu
from .LinearElasticitySolver import LinearElasticitySolver
from .WaveSolver import tabulate_time_function, nearest_vertices
from . import solid_steps, time_marching

_EXPLICIT = ('alpha_m', 'alpha_f', 'beta', 'gamma')
_DYNAMICS_KEYS = set(_EXPLICIT) | {'spectral_radius', 'rayleigh_mass', 'rayleigh_stiffness', 'energy_freq', 'scheme', 'batch_steps'}
_SCHEMES = ('implicit', 'explicit')


def generalized_alpha(spectral_radius):
    """(alpha_m, alpha_f, beta, gamma) of the Chung-Hulbert scheme with the high-frequency spectral radius rho_inf in [0, 1]"""
    r = float(spectral_radius)
    if not 0.0 <= r <= 1.0:
        raise SolverError('ElastodynamicsSolver: spectral_radius must lie in [0, 1], got {}'.format(spectral_radius))
    am, af = (2.0 * r - 1.0) / (r + 1.0), r / (r + 1.0)
    return am, af, 0.25 * (1.0 - am + af) ** 2, 0.5 - am + af


def unconditionally_stable(alpha_m, alpha_f, beta, gamma):
    return bool(all(math.isfinite(x) for x in (alpha_m, alpha_f, beta, gamma)) and alpha_m <= alpha_f <= 0.5
                and beta >= 0.25 + 0.5 * (alpha_f - alpha_m))


def effective_coefficients(alpha_m, alpha_f, beta, gamma, dt, eta_m=0.0, eta_k=0.0):
    """(c_M, c_K) of K_eff = c_M M + c_K K"""
    return ((1.0 - alpha_m) / (beta * dt * dt) + (1.0 - alpha_f) * gamma * eta_m / (beta * dt),
            (1.0 - alpha_f) * (1.0 + gamma * eta_k / (beta * dt)))


class ElastodynamicsSolver(LinearElasticitySolver):
    _constraint_sides = False          # 'contact' / 'sliding' sides stay with the static linear solver

    def __init__(self, case_settings):
        LinearElasticitySolver.__init__(self, case_settings)
        self.reference_load_sign = False          # loads with their physical sign, as in PlasticitySolver
        self.operator_assemblies = 0
        self.amg_setups = 0
        self.step_stats = []
        self.state = None
        self.receiver_vertices = np.zeros(0, dtype=np.int32)
        self._dyn_ctx = None
        self._dyn_serial = 0
        self._K = self._M = None
        self._traces = self._energy = self._velocity = self._acceleration = None
        self._bounds = self._mass = None          # explicit scheme: (2/sqrt(lambda_G), 2/sqrt(lambda_P)), the lumped mass
        self.nonfinite_steps = None               # explicit scheme, after a march that failed: (steps the library counted, the first)

    # ------------------------------------------------------------------ settings (host only)
    def dynamics_settings(self):
        given = self.solver_settings.get('dynamics_settings') or self.settings.get('dynamics_settings') or {}
        unknown = set(given) - _DYNAMICS_KEYS
        if unknown:
            raise SolverError('ElastodynamicsSolver: dynamics_settings: unknown key(s) {}'.format(sorted(unknown)))
        return given

    def scheme(self):
        """'implicit' (generalized-alpha, the default) or 'explicit' (central differences with a lumped mass)"""
        ds = self.dynamics_settings()
        s = ds.get('scheme', 'implicit')
        if s not in _SCHEMES:
            raise SolverError("ElastodynamicsSolver: dynamics_settings: 'scheme' must be 'implicit' or 'explicit', got {!r}".format(s))
        if s == 'implicit' and 'batch_steps' in ds:
            raise SolverError("ElastodynamicsSolver: dynamics_settings: 'batch_steps' belongs to the explicit scheme (the implicit one "
                              "solves step by step)")
        return s

    def explicit_parameters(self):
        """{'rayleigh_mass', 'batch_steps'} of the explicit scheme, checked (SolverError on a key the scheme does not take)"""
        ds = self.dynamics_settings()
        taken = [k for k in ('spectral_radius',) + _EXPLICIT if k in ds]
        if taken:
            raise SolverError("ElastodynamicsSolver: dynamics_settings: {} belong(s) to the generalized-alpha scheme and mean(s) nothing "
                              "under 'scheme': 'explicit'".format(taken))
        for k in ('rayleigh_mass', 'rayleigh_stiffness'):
            if k in ds and (isinstance(ds[k], bool) or not isinstance(ds[k], numbers.Real)):
                raise SolverError('ElastodynamicsSolver: dynamics_settings: {} must be a number, got {!r}'.format(k, ds[k]))
        if float(ds.get('rayleigh_stiffness', 0.0)) != 0.0:
            raise SolverError("ElastodynamicsSolver: dynamics_settings: 'rayleigh_stiffness' = {}: stiffness-proportional damping is not "
                              "offered by the explicit scheme (a lagged treatment needs a second field per product and changes the step "
                              "bound); use 'rayleigh_mass' or 'scheme': 'implicit'".format(ds['rayleigh_stiffness']))
        eta_m = float(ds.get('rayleigh_mass', 0.0))
        if not (eta_m >= 0.0 and math.isfinite(eta_m)):
            raise SolverError('ElastodynamicsSolver: rayleigh_mass must be >= 0, got {}'.format(eta_m))
        bs = ds.get('batch_steps')
        if bs is not None and (isinstance(bs, bool) or not isinstance(bs, numbers.Integral) or bs < 1):
            raise SolverError("ElastodynamicsSolver: dynamics_settings: 'batch_steps' must be a positive number of steps, got {!r}".format(bs))
        return {'rayleigh_mass': eta_m, 'batch_steps': None if bs is None else int(bs)}

    def generalized_alpha_parameters(self):
        """{'alpha_m', 'alpha_f', 'beta', 'gamma', 'rayleigh_mass', 'rayleigh_stiffness'}, checked (SolverError on a bad set)"""
        ds = self.dynamics_settings()
        explicit = [k for k in _EXPLICIT if k in ds]
        if explicit and 'spectral_radius' in ds:
            raise SolverError("ElastodynamicsSolver: dynamics_settings: give 'spectral_radius' or the four of {}, not both".format(_EXPLICIT))
        if explicit and len(explicit) != 4:
            raise SolverError('ElastodynamicsSolver: dynamics_settings: all four of {} are needed, got {}'.format(_EXPLICIT, explicit))
        for k in explicit + ['rayleigh_mass', 'rayleigh_stiffness', 'spectral_radius']:
            if k in ds and (isinstance(ds[k], bool) or not isinstance(ds[k], numbers.Real)):
                raise SolverError('ElastodynamicsSolver: dynamics_settings: {} must be a number, got {!r}'.format(k, ds[k]))
        am, af, beta, gamma = [float(ds[k]) for k in _EXPLICIT] if explicit else generalized_alpha(ds.get('spectral_radius', 1.0))
        if not unconditionally_stable(am, af, beta, gamma):
            raise SolverError('ElastodynamicsSolver: (alpha_m, alpha_f, beta, gamma) = ({}, {}, {}, {}) is outside alpha_m <= alpha_f <= 1/2, '
                              'beta >= 1/4 + (alpha_f - alpha_m)/2: the scheme is not unconditionally stable'.format(am, af, beta, gamma))
        eta_m, eta_k = float(ds.get('rayleigh_mass', 0.0)), float(ds.get('rayleigh_stiffness', 0.0))
        if not (eta_m >= 0.0 and eta_k >= 0.0 and math.isfinite(eta_m) and math.isfinite(eta_k)):
            raise SolverError('ElastodynamicsSolver: rayleigh_mass and rayleigh_stiffness must be >= 0, got {} and {}'.format(eta_m, eta_k))
        return {'alpha_m': am, 'alpha_f': af, 'beta': beta, 'gamma': gamma, 'rayleigh_mass': eta_m, 'rayleigh_stiffness': eta_k}

    def energy_freq(self):
        f = self.dynamics_settings().get('energy_freq', 0) or 0
        if isinstance(f, bool) or not isinstance(f, numbers.Integral) or f < 0:
            raise SolverError("ElastodynamicsSolver: dynamics_settings: 'energy_freq' must be an integer >= 0, got {!r}".format(f))
        return int(f)

    def time_points(self):
        """t_0 .. t_N: the run is N steps, uniform ('time_step') or along 'time_series'"""
        ts = self.transient_settings
        if not ts.get('transient'):
            raise SolverError("ElastodynamicsSolver: 'transient': False - structural dynamics has no steady form here (LinearElasticitySolver "
                              "solves the static problem)")
        series = ts.get('time_series')
        if series is not None:
            t = np.asarray(series, dtype=np.float64).ravel()
            t_end = float(ts.get('ending_time', t[-1] if len(t) else 0.0))
            n = int(np.count_nonzero(t[:-1] < t_end)) if len(t) > 1 else 0
            t = t[:n + 1]
            if n < 1 or not (np.all(np.diff(t) > 0.0) and np.all(np.isfinite(t))):
                raise SolverError("ElastodynamicsSolver: 'time_series' must hold increasing time points with at least one step before "
                                  "'ending_time'")
            return t
        t0, dt, t1 = float(ts['starting_time']), float(ts['time_step']), float(ts['ending_time'])
        if not (dt > 0.0 and np.isfinite(dt)) or not t1 > t0:
            raise SolverError('ElastodynamicsSolver: time_step {} and the interval [{}, {}] do not make a run'.format(dt, t0, t1))
        n = max(int(math.ceil((t1 - t0) / dt - 1e-9)), 1)
        return t0 + dt * np.arange(n + 1)

    def step_lengths(self):
        ts = self.transient_settings
        t = self.time_points()
        if ts.get('time_series') is None:
            return np.full(len(t) - 1, float(ts['time_step']))
        return np.diff(t)

    @staticmethod
    def _is_zero_value(v):
        if v is None:
            return True
        if isinstance(v, numbers.Number):
            return float(v) == 0.0
        if isinstance(v, Constant):
            return not np.any(v.values())
        if isinstance(v, (tuple, list)):
            return all(ElastodynamicsSolver._is_zero_value(c) for c in v)
        return False

    def uniform_step(self):
        """dt of the explicit scheme: every step of the run has this length"""
        dts = self.step_lengths()
        dt = float(dts[0])
        if np.any(np.abs(dts - dt) > 1e-9 * dt):
            raise SolverError("ElastodynamicsSolver: non-uniform steps ('time_series') are not supported by the explicit scheme: a uniform "
                              "'time_step' only")
        return dt

    def time_factors(self):
        """implicit: (s_f [N] at t_n + (1 - alpha_f) dt_n, s_g [N + 1] at the time points); explicit: (s_f [N + 1], s_g [N + 1]), both
        at the time points"""
        t, dts = self.time_points(), self.step_lengths()
        if self.scheme() == 'explicit':
            sf = tabulate_time_function(self.settings.get('load_time_function'), t, 'load_time_function')
        else:
            af = self.generalized_alpha_parameters()['alpha_f']
            sf = tabulate_time_function(self.settings.get('load_time_function'), t[:-1] + (1.0 - af) * dts, 'load_time_function')
        sg, owner = None, None
        for name, bc_settings in (self.boundary_conditions or {}).items():
            bc = self.get_boundary_variable(bc_settings)
            if bc['type'] not in ('Dirichlet', 'displacement'):
                continue
            tf = bc.get('time_function')
            if tf is None and self._is_zero_value(bc.get('value', 0.0)):
                continue                  # a homogeneous side takes any factor
            tab = tabulate_time_function(tf, t, "boundary '{}': time_function".format(name))
            if sg is not None and not np.array_equal(tab, sg):
                raise SolverError("ElastodynamicsSolver: boundaries '{}' and '{}' have different time functions: the Dirichlet values "
                                  "share one factor per time point".format(owner, name))
            sg, owner = tab, name
        return sf, (np.ones(len(t)) if sg is None else sg)

    def _load_factor_at_start(self, sf):
        """s_f(t_0) for the initial acceleration; a 'table' holds one value per step and none for t_0: its first entry"""
        spec = self.settings.get('load_time_function')
        if isinstance(spec, dict) and spec.get('type') == 'table':
            return float(sf[0])
        return float(tabulate_time_function(spec, self.time_points()[:1], 'load_time_function')[0])

    def _refuse_unsupported(self):
        V = self.function_space

        def space_check():
            if V.degree() not in (1, 2) or getattr(V, '_ncomp', 1) != self.dimension:
                raise SolverError('ElastodynamicsSolver: vector CG1 or CG2 spaces only')
        solid_steps.refuse_unsupported(self, 'ElastodynamicsSolver', ' (no thermal strain in the model)',
                                       ('point_source', 'surface_source'), space_check)
        rho = self.material_field('density')
        if not (np.all(np.asarray(rho) > 0.0) and np.all(np.isfinite(rho))):
            raise SolverError("ElastodynamicsSolver: material 'density' must be positive")
        if self.scheme() == 'explicit':
            self.explicit_parameters()
            if V.degree() != 1:
                raise SolverError("ElastodynamicsSolver: CG{} spaces are not supported by the explicit scheme (vector CG1 only: a row-sum "
                                  "lumped P2 mass is not positive)".format(V.degree()))
            self.uniform_step()
        else:
            self.generalized_alpha_parameters()
        self.energy_freq()
        self.time_factors()               # (the time grid and every table against the length of the run)
        self.lame_parameters()

    def _vector_field(self, v, what):
        """a number, a tuple, an expression or a nodal array -> dof values (node-major)"""
        V, d = self.function_space, self.dimension
        n = V.dim()
        if v is None:
            return np.zeros(n)
        if isinstance(v, numbers.Number):
            return np.full(n, float(v))
        if isinstance(v, (tuple, list)) and len(v) == d and all(isinstance(c, (str, numbers.Number)) for c in v):
            if all(isinstance(c, numbers.Number) for c in v):
                return np.tile(np.asarray(v, dtype=np.float64), n // d)
            return np.asarray(interpolate(Expression(tuple(str(c) for c in v), degree=V.degree()), V).vector()._values(), dtype=np.float64).copy()
        if isinstance(v, Constant):
            return np.tile(np.asarray(v.values(), dtype=np.float64), n // d)
        if isinstance(v, Expression):
            return np.asarray(interpolate(v, V).vector()._values(), dtype=np.float64).copy()
        if isinstance(v, Function):
            v = v.vector()._values()
        a = np.asarray(v, dtype=np.float64).ravel()
        if a.size != n:
            raise SolverError('ElastodynamicsSolver: {} holds {} values, the space has {} dofs'.format(what, a.size, n))
        return a.copy()

    def initial_fields(self):
        """(u_0, v_0) as dof arrays in the caller's numbering"""
        iv = self.initial_values or {}
        u0 = self._vector_field(iv.get(self.get_variable_name()), 'initial_values')
        v0 = self._vector_field(self.settings.get('initial_velocity', iv.get('velocity')), 'initial_velocity')
        if not (np.all(np.isfinite(u0)) and np.all(np.isfinite(v0))):
            raise SolverError('ElastodynamicsSolver: the initial displacement or velocity is not finite')
        return u0, v0

    def snap_receivers(self):
        pts = self.settings.get('receivers') or []
        self.receiver_vertices = nearest_vertices(self.mesh.coordinates(), pts) if len(pts) else np.zeros(0, dtype=np.int32)
        return self.receiver_vertices

    # ------------------------------------------------------------------ the device side
    def _to_dev(self, a):
        return a if self._loc is None else self._loc.nodes(a)

    def _to_host(self, a):
        if self._loc is None:
            return a
        out = np.empty_like(a)
        out.reshape(self._loc.n_global, -1)[np.asarray(self._loc.l2g)] = a.reshape(self._loc.n_global, -1)
        return out

    def close(self):
        """free the device state, the operators and the hierarchy"""
        cached = getattr(self, '_amg_cache', None)
        if cached is not None:
            cached[1].close()
            self._amg_cache = None
        if self._dyn_ctx is not None:
            self._dyn_ctx['K_eff'].close()
            self._dyn_ctx = None
        for name in ('_K', '_M', 'state'):
            obj = getattr(self, name, None)
            if obj is not None:
                obj.close()
                setattr(self, name, None)

    def _setup(self):
        """K, M, F, the Dirichlet rows and the state object on the device.  Everything here is set-up cost."""
        from . import backend
        self._refuse_unsupported()
        explicit = self.scheme() == 'explicit'
        par = self.explicit_parameters() if explicit else self.generalized_alpha_parameters()
        sf, sg = self.time_factors()
        u0, v0 = self.initial_fields()
        self.snap_receivers()
        form, bcs = LinearElasticitySolver.generate_form(self, 0, None, None, None, None)
        self.close()
        V = self.function_space.device()
        loc = self._loc = self.function_space.localizer()
        if loc is not None and getattr(loc, 'is_local_view', False):
            raise SolverError('ElastodynamicsSolver runs on one rank')
        gdofs, gvals = self._bc_arrays(bcs)
        u0 = u0.copy()
        u0[gdofs.astype(np.int64)] = gvals * sg[0]                # the initial displacement takes the Dirichlet values of t_0
        dofs, vals = (gdofs, gvals) if loc is None else loc.dofs(gdofs, gvals)
        lame = solid_steps.localized(form.lame_spec(), loc)
        rho = self.material_field('density')
        if np.ndim(rho) > 0:
            rho = np.asarray(rho, dtype=np.float64)
            rho = rho if loc is None else loc.cells(rho)
        self._lame, self._rho = lame, rho
        K = backend.DeviceMatrix(V)
        K.assemble(lame=lame)
        M = backend.DeviceMatrix(V)
        M.assemble(lame=(0.0, 0.0), mass=self._density_spec(1.0))
        if self.function_space.degree() == 1:
            b = solid_steps.external_loads(self, form, V, loc)    # per dof in a fixed order: the same bits from run to run
        else:
            A_, b = self.assemble_system(form, [])                # (CG2 facet loads: the consistent P2 weights)
            A_.close()
        load = b.get()[:V.n_owned]
        b.close()
        rec = self._receiver_dofs(loc)
        self._K, self._M = K, M
        self._dirichlet = (np.asarray(dofs, dtype=np.int32), np.asarray(vals, dtype=np.float64))
        self._load, self._par = load, par
        if explicit:
            self._setup_explicit(V)
        else:
            self.state = backend.DynamicsState(V)
        return V, u0, v0, sf, sg, rec

    def _receiver_dofs(self, loc):
        """the dofs (device order, every component) of the snapped receiver vertices"""
        d = self.dimension
        rv = np.asarray(self.receiver_vertices, dtype=np.int64)
        rec = (rv[:, None] * d + np.arange(d)[None, :]).ravel()
        if loc is not None and len(rec):
            rec = loc.dofs(rec, np.zeros(len(rec)))[0]
        return rec.astype(np.int32)

    # ------------------------------------------------------------------ the explicit scheme
    def _lumped_mass(self, V, M):
        """m = M 1 (device dof order); M is closed: the consistent mass has done its work"""
        from . import backend
        n = V.n_owned
        ones, md = backend.DeviceVector(V.n_local, np.ones(V.n_local)), backend.DeviceVector(n)
        M.spmv(ones, md)
        m = md.get()[:n].copy()
        ones.close()
        md.close()
        M.close()
        if not (np.all(m > 0.0) and np.all(np.isfinite(m))):
            raise SolverError('{}: the lumped mass M 1 is not positive on every row (smallest entry {})'.format(type(self).__name__, m.min()))
        return m

    def _check_step(self, dt):
        """a step above the second bound is refused, one between the two is logged"""
        time_marching.check_step(type(self).__name__, dt, self._bounds, self.logger, march='the explicit march')

    def _setup_explicit(self, V):
        """m = M 1, both step bounds and the state object of the central-difference marcher"""
        from . import backend
        m = self._lumped_mass(V, self._M)
        self._M = None
        dofs, vals = self._dirichlet
        self._mass, self._bounds = m, time_marching.step_bounds(self, self._K, m, dofs)
        dt = self.uniform_step()
        self._check_step(dt)
        self.state = backend.ExplicitDynamicsState(V)
        self.state.configure(dt, self._par['rayleigh_mass'], m, load=self._load, dirichlet_dofs=dofs, dirichlet_values=vals)

    def _power_iteration(self, K, m, bc_dofs):
        """lambda_P, a lower bound on the largest eigenvalue of diag(1/m) K on the rows that are not Dirichlet"""
        return time_marching.power_iteration(K, m, bc_dofs, type(self).__name__)

    def _explicit_only(self, what):
        if self.scheme() != 'explicit':
            raise SolverError("ElastodynamicsSolver: {} belongs to 'scheme': 'explicit' (the implicit scheme is unconditionally "
                              "stable)".format(what))

    def critical_time_step(self):
        """explicit scheme: 2 / sqrt(lambda_G), lambda_G = max_i sum_j |K_ij| / m_i: the step below which the march is stable"""
        return self.time_step_bounds()[0]

    def time_step_bounds(self):
        """explicit scheme: (2 / sqrt(lambda_G), 2 / sqrt(lambda_P)): stable below the first, certain to blow up above the second.
        Neither depends on eta_M.  A ``time_step`` above the second raises SolverError here as it does in solve()."""
        self._explicit_only('a step bound')
        if self._bounds is None:
            self._setup()
        return self._bounds

    def _batch_end(self, n, N):
        """the step at which the batch that starts at step n ends: the next plot / save / energy step, at most batch_steps away"""
        freqs = (self.report_settings.get('plotting_freq', 0), self.report_settings.get('saving_freq', 0), self.energy_freq())
        return time_marching.batch_end(n, N, freqs, self._par['batch_steps'])

    _not_finite = 'the state or its energy is not finite'

    def _blow_up_message(self, first, end):
        return ('{}: {} in steps {} .. {} (time_step {:.6g}; stable below '
                '2/sqrt(lambda_G) = {:.6g}, certain to blow up above 2/sqrt(lambda_P) = {:.6g})'.format(
                    type(self).__name__, self._not_finite, first, end, self.uniform_step(), self._bounds[0], self._bounds[1]))

    # what a step of the explicit march asks of the device state: the subclass with another force term overrides these four
    def _march_start(self, u0d, v0d, sf0, sg0, sg1):
        self.state.start(self._K, u0d, v0d, sf0, sg0, sg1)

    def _march_advance(self, sf, sg, rec):
        return self.state.advance(self._K, sf, sg, receivers=rec, traces=len(rec) > 0, energy=True, info=True)

    def _first_step_potential(self, u1):
        """the potential half of the energy row of the step 0 -> 1"""
        return 0.5 * float(u1 @ self.state.work())

    def _publish_explicit(self, sf_n):
        u, _, _ = self.state.get()
        v, a = self.state.full_step(self._K, sf_n)
        self.w_current = self.result = self._function(u)
        self._velocity, self._acceleration = self._function(v), self._function(a)

    def _solve_explicit(self):
        self.operator_assemblies = self.amg_setups = 0
        V, u0, v0, sf, sg, rec = self._setup()
        t = self.time_points()
        dt = self.uniform_step()
        N, d = len(t) - 1, self.dimension
        st, m = self.state, self._mass
        efreq = self.energy_freq()
        self.step_stats = []
        self._saved_frames = []
        traces = np.zeros((N + 1, len(rec) // d, d))
        energy = []
        # step 0 -> 1 on the device; its energy from the fields and the product of the start (set-up cost)
        u0d = self._to_dev(u0)
        self._march_start(u0d, self._to_dev(v0), sf[0], sg[0], sg[1])
        u1, w1, _ = st.get()
        if not (np.all(np.isfinite(u1)) and np.all(np.isfinite(w1))):
            raise SolverError(self._blow_up_message(0, 1))
        if len(rec):
            traces[0], traces[1] = u0d[rec].reshape(-1, d), u1[rec].reshape(-1, d)
        if efreq == 1:
            energy.append((1, 0.5 * float(np.sum(m * w1 * w1)), self._first_step_potential(u1)))
        pvd = self.report_settings.get('result_filename') or 'result_file.pvd'
        n = 1                       # the state holds (u_n, w_n)
        self.current_step, self.current_time = 1, float(t[1])
        while True:
            published = self._due('plotting_freq') or self._due('saving_freq')
            if published:
                self._publish_explicit(sf[n])
                if self._due('plotting_freq'):
                    self.plot()
                if self._due('saving_freq'):
                    self.save(pvd)
            if n >= N:
                break
            end = self._batch_end(n, N)
            k = end - n
            out = self._march_advance(sf[n:end], sg[n + 1:end + 1], rec)
            self.step_stats.append({'first_step': n, 'steps': k, 'device_ms': out['device_ms'], 'ms_per_step': out['device_ms'] / k})
            if out['n_nonfinite']:
                self.nonfinite_steps = (out['n_nonfinite'], n + out['first_nonfinite_step'])      # what the library counted
                raise SolverError(self._blow_up_message(n + out['first_nonfinite_step'], end))
            if len(rec):
                traces[n + 1:end + 1] = out['traces'].reshape(k, -1, d)
            if efreq:
                for j in range(n, end):
                    if (j + 1) % efreq == 0:
                        energy.append((j + 1, float(out['energy'][j - n, 0]), float(out['energy'][j - n, 1])))
            n = end
            self.current_step, self.current_time = n, float(t[n])
            if efreq and n % efreq == 0:
                self.logger.info('ElastodynamicsSolver: step %d time %g energy %.12g (%.3f ms per step)', n, self.current_time,
                                 energy[-1][1] + energy[-1][2], self.step_stats[-1]['ms_per_step'])
        if not published:
            self._publish_explicit(sf[N])
        self._traces, self._energy = traces, np.asarray(energy, dtype=np.float64).reshape(-1, 3)
        return self.w_current

    def _density_spec(self, c):
        return c * float(self._rho) if np.ndim(self._rho) == 0 else ('cell', c * self._rho)

    def _operator_context(self, V, dt):
        """K_eff = c_M M + c_K K with its Dirichlet rows and columns eliminated and the state's constants: once per step length"""
        from . import backend
        ctx = self._dyn_ctx
        if ctx is not None and abs(ctx['dt'] - dt) <= 1e-12 * dt:
            return ctx
        if ctx is not None:
            cached = getattr(self, '_amg_cache', None)
            if cached is not None:                               # the hierarchy of the operator that goes
                cached[1].close()
                self._amg_cache = None
            ctx['K_eff'].close()
        p = self._par
        cm, ck = effective_coefficients(p['alpha_m'], p['alpha_f'], p['beta'], p['gamma'], dt, p['rayleigh_mass'], p['rayleigh_stiffness'])
        lame = self._lame
        lame = ('cell', ck * np.asarray(lame[1])) if isinstance(lame[0], str) else (ck * lame[0], ck * lame[1])
        K_eff = backend.DeviceMatrix(V)
        K_eff.assemble(lame=lame, mass=self._density_spec(cm))    # c_K K + c_M M: one form
        dofs, vals = self._dirichlet
        if len(dofs):
            K_eff.apply_dirichlet(None, dofs, np.zeros(len(dofs)), symmetric=True)
        self.operator_assemblies += 1
        self._dyn_serial += 1                                     # never reused: the key of the AMG hierarchy
        self.state.configure(dt, p['alpha_m'], p['alpha_f'], p['beta'], p['gamma'], p['rayleigh_mass'], p['rayleigh_stiffness'],
                             load=self._load, dirichlet_dofs=dofs, dirichlet_values=vals)
        ctx = self._dyn_ctx = {'dt': dt, 'K_eff': K_eff, 'key': ('elastodynamics', self._dyn_serial)}
        return ctx

    def _start(self, V, u0, v0, sf0, rhs, x):
        """a_0 from M a_0 = s_f(t_0) F - C v_0 - K u_0 on the free rows: Jacobi-CG on the eliminated M"""
        from . import backend
        st = self.state
        st.start_rhs(self._K, self._M, self._to_dev(u0), self._to_dev(v0), sf0, rhs)
        x.fill(0.0)
        if rhs.dot(rhs) > 0.0:
            dofs, _ = self._dirichlet
            M_el = backend.DeviceMatrix(V)
            M_el.copy_from(self._M)
            if len(dofs):
                M_el.apply_dirichlet(None, dofs, np.zeros(len(dofs)), symmetric=True)
            try:
                self._device_solve_vectors(M_el, rhs, x, 'initial acceleration')
            finally:
                M_el.close()
        st.start(x)

    # ------------------------------------------------------------------ the march
    def _function(self, dev_values):
        f = Function(self.function_space)
        f.vector().set_local(self._to_host(np.asarray(dev_values)))
        return f

    def _publish(self):
        u, v, a, _ = self.state.get()
        self.w_current = self.result = self._function(u)
        self._velocity, self._acceleration = self._function(v), self._function(a)

    def solve_transient(self):
        from . import backend
        if self.scheme() == 'explicit':
            return self._solve_explicit()
        V, u0, v0, sf, sg, rec = self._setup()
        t, dts = self.time_points(), self.step_lengths()
        N, d = len(dts), self.dimension
        st, K, M = self.state, self._K, self._M
        efreq = self.energy_freq()
        self.operator_assemblies = self.amg_setups = 0
        self.step_stats = []
        self._saved_frames = []
        rhs, x = backend.DeviceVector(V.n_owned), backend.DeviceVector(V.n_local)
        traces = np.zeros((N + 1, len(rec) // d, d))
        energy = []
        self._operator_context(V, float(dts[0]))
        s0 = self._load_factor_at_start(sf)
        self._start(V, u0, v0, s0, rhs, x)
        if len(rec):
            traces[0] = self._to_dev(u0)[rec].reshape(-1, d)
        if efreq:
            energy.append((0,) + st.energy(K, M))
        pvd = self.report_settings.get('result_filename') or 'result_file.pvd'
        for n in range(N):
            ctx = self._operator_context(V, float(dts[n]))
            st.predict(K, M, sf[n], sg[n + 1], rhs)
            if d == 3:
                stats = self._device_solve_vectors(ctx['K_eff'], rhs, x, 'elastodynamics step', amg=True, near_nullspace="rigid_body",
                                                   operator_key=ctx['key'])
                if not stats['amg_reused']:
                    self.amg_setups += 1
            else:
                stats = self._device_solve_vectors(ctx['K_eff'], rhs, x, 'elastodynamics step')
            samples = st.correct(x, rec if len(rec) else None)
            info = st.info()
            if info['n_nonfinite']:
                raise SolverError('ElastodynamicsSolver: the state is not finite after step {} ({} rows)'.format(
                    info['first_nonfinite_step'], info['n_nonfinite']))
            if samples is not None:
                traces[n + 1] = samples.reshape(-1, d)
            self.step_stats.append({'predict_ms': info['predict_ms'], 'predict_pointwise_ms': info['predict_pointwise_ms'],
                                    'solve_ms': stats['solve_ms'], 'correct_ms': info['correct_ms'], 'iterations': stats['iterations'],
                                    'amg_setup_ms': 0.0 if stats.get('amg_reused', True) else stats['amg_setup_ms']})
            self.current_step, self.current_time = n + 1, float(t[n + 1])
            if efreq and (n + 1) % efreq == 0:
                energy.append((n + 1,) + st.energy(K, M))
                self.logger.info('ElastodynamicsSolver: step %d time %g energy %.12g', n + 1, self.current_time, energy[-1][1] + energy[-1][2])
            if self._due('plotting_freq') or self._due('saving_freq'):
                self._publish()
                if self._due('plotting_freq'):
                    self.plot()
                if self._due('saving_freq'):
                    self.save(pvd)
        self._publish()
        rhs.close()
        x.close()
        self._traces, self._energy = traces, np.asarray(energy, dtype=np.float64).reshape(-1, 3)
        return self.w_current

    def solve(self):
        self.result = self.solve_transient()
        return self.result

    def save(self, result_filename):
        """PVD collection + one VTU per call with the displacement and the velocity"""
        assert result_filename[-4:] == '.pvd'
        root = result_filename[:-4]
        if not hasattr(self, '_saved_frames'):
            self._saved_frames = []
        vtu = "%s%06d.vtu" % (root, len(self._saved_frames))
        extra = [(self._velocity, 'velocity')] if self._velocity is not None else []
        write_vtu(vtu, self.mesh, self.w_current, self.get_variable_name(), extra=extra)
        self._saved_frames.append((getattr(self, 'current_time', 0.0), os.path.basename(vtu)))
        with open(result_filename, "w") as fh:
            fh.write('<?xml version="1.0"?>\n<VTKFile type="Collection" version="0.1">\n  <Collection>\n')
            for tm, f in self._saved_frames:
                fh.write('    <DataSet timestep="%g" part="0" file="%s" />\n' % (tm, f))
            fh.write('  </Collection>\n</VTKFile>\n')

    # ------------------------------------------------------------------ results
    def _need(self, what):
        if what is None:
            raise SolverError('ElastodynamicsSolver: no run has been marched yet')
        return what

    def velocity(self):
        """v of the last step, a Function (explicit scheme: the full-step v_N = (w_{N-1/2} + w+) / 2)"""
        return self._need(self._velocity)

    def acceleration(self):
        """a of the last step, a Function (explicit scheme: the full-step a_N = (w+ - w_{N-1/2}) / dt)"""
        return self._need(self._acceleration)

    def receiver_traces(self):
        """[n_steps + 1, n_receivers, dim]: the displacement at the receiver vertices at every time point, t_0 included"""
        return self._need(self._traces)

    def energy(self):
        """[k, 3]: (step, E_kin, E_pot) at step 0 and every energy_freq-th step; explicit scheme: (n + 1, E_kin, E_pot) of the step
        n -> n+1 for every energy_freq-th step, and no step-0 row (the discrete energy lives on the half steps)"""
        return self._need(self._energy)
