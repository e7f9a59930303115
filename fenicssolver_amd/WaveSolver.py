"""WaveSolver — explicit scalar wave propagation on scalar P1 (triangles, tetrahedra), GPU back end.

The reference lists "wave propagation" among its solvers under development (Readme.md) and has no such class; this one fills the gap
with the textbook model, so there is no reference counterpart to diff against; the independent check is the numpy
restatement tests/wave_reference.py.

Model: u_tt = div(c^2 grad u) + f, central differences in time with a lumped mass.  K is the scalar stiffness with coefficient c^2,
m_i = int phi_i dx the lumped mass, d_i the lumped first-order absorbing boundary (the sum over the absorbing facets F around node i of
c(cell of F) |F| / dim: c^2 du/dn = -c u_t), F the load (body source + flux facets, c^2 du/dn = g, + point sources).  All loads share
one time factor, f^n = s_f[n] F, and Dirichlet dofs take g_i s_g[n]; the host tabulates both per step.  Step n -> n+1, with y = K u^n:
    (m/dt^2 + d/(2 dt)) u^{n+1} = s_f[n] F - y + (2 m/dt^2) u^n - (m/dt^2 - d/(2 dt)) u^{n-1},   then the Dirichlet dofs: g s_g[n+1];
the start is a^0 = (s_f[0] F - K u^0 - d v^0) / m, u^1 = u^0 + dt v^0 + dt^2/2 a^0.  A step is not a solve: one product with K and one
pointwise update, and the steps of a batch run back to back on the device with no host round trip (fs_wave_advance).  The discrete
energy of step n -> n+1 is E = 1/2 sum m ((u^{n+1} - u^n)/dt)^2 + 1/2 (u^{n+1})^T K u^n: constant without loads, damping and moving
Dirichlet values, non-increasing with an absorbing side.

Time step: lambda_G = max_i sum_j |K_ij| / m_i bounds lambda_max(M_L^-1 K) from above, so dt <= 2 / sqrt(lambda_G) =
``critical_time_step()`` is stable; a few dozen power iterations on the device give a Rayleigh quotient lambda_P <= lambda_max (of the
rows that are not Dirichlet): a dt above 2 / sqrt(lambda_P) is certain to blow up and raises SolverError before any marching call,
a dt between the two bounds runs with a logged warning.

Settings: material ``wave_speed`` (a positive number or a per-region dict); boundary types ``Dirichlet`` (optional ``time_function``),
``flux`` and ``absorbing``, unlisted facets natural; ``body_source`` and ``point_source`` as ScalarTransportSolver takes them;
``source_time_function`` = {'type': 'ricker', 'frequency', 'delay'} | {'type': 'table', 'values': [one per step]} | a callable of t |
absent (1); ``initial_values[<scalar_name>]`` and ``initial_velocity``: a number, an expression string or a nodal array;
``receivers``: points, each snapped to the nearest vertex (``receiver_vertices``); ``transient_settings`` with a uniform ``time_step``;
``batch_steps`` caps the steps of one device call and ``energy_freq`` ends a batch (and logs the energy) every that many steps - by
default a batch runs to the next plot / save step of the time loop.  Dirichlet boundaries with non-zero values share one time function
(the device scales all Dirichlet values by one factor per step); a 'table' for them holds one value per time POINT (steps + 1).

Results: ``solve()`` returns the last field; ``velocity()`` (u^{n+1} - u^{n-1}) / (2 dt) of the last step; ``receiver_traces()``
[n_steps + 1, n_receivers] from t0 on; ``energy()`` [n_steps, 2] = (kinetic, potential) per step; ``step_stats`` the device
milliseconds per batch and per step.  P2 spaces (a lumped P2 mass has non-positive vertex weights), several ranks, periodic spaces,
``transient: False``, non-uniform steps, ``wave_speed`` <= 0, an advection velocity and a table shorter than the run raise SolverError
before any device call; a non-finite field at the end of a batch raises SolverError naming the step range and both step bounds.
"""
from __future__ import annotations

import math
import numbers

import numpy as np

from .fem import Constant, Expression, Function, DirichletBC, PointSource, Point, nodal_values, is_constant_value
from .SolverBase import SolverBase, SolverError
from . import case, time_marching


def ricker(t, frequency, delay):
    """(1 - 2 a) exp(-a), a = (pi f (t - delay))^2"""
    a = (math.pi * float(frequency) * (np.asarray(t, dtype=np.float64) - float(delay))) ** 2
    return (1.0 - 2.0 * a) * np.exp(-a)


def tabulate_time_function(spec, times, what='source_time_function'):
    """The factor at every entry of ``times`` (uniform time points from the starting time on): None -> 1; a callable of t; {'type':
    'ricker', 'frequency', 'delay'}; {'type': 'table', 'values'} - entry k belongs to times[k], and a table shorter than ``times`` is
    an error."""
    times = np.asarray(times, dtype=np.float64)
    if spec is None:
        return np.ones(len(times))
    if callable(spec):
        out = np.array([float(spec(float(t))) for t in times])
    elif isinstance(spec, dict) and spec.get('type') == 'ricker':
        if 'frequency' not in spec or not float(spec['frequency']) > 0.0:
            raise SolverError("WaveSolver: {}: a 'ricker' wavelet needs a positive 'frequency'".format(what))
        out = ricker(times, spec['frequency'], spec.get('delay', 0.0))
    elif isinstance(spec, dict) and spec.get('type') == 'table':
        vals = np.asarray(spec.get('values', ()), dtype=np.float64).ravel()
        if len(vals) < len(times):
            raise SolverError("WaveSolver: {}: the table holds {} values, the run needs {}".format(what, len(vals), len(times)))
        out = vals[:len(times)].copy()
    else:
        raise SolverError("WaveSolver: {} must be {{'type': 'ricker' | 'table', ...}}, a callable of t or absent, got {!r}".format(what, spec))
    if not np.all(np.isfinite(out)):
        raise SolverError("WaveSolver: {} is not finite at every step".format(what))
    return out


def nearest_vertices(coords, points):
    """index of the vertex nearest to every point (the lowest index among equally near ones)"""
    co = np.asarray(coords, dtype=np.float64)
    out = []
    for p in points:
        q = np.zeros(co.shape[1])
        xs = p.array() if isinstance(p, Point) else np.asarray(p, dtype=np.float64).ravel()
        k = min(len(xs), co.shape[1])
        q[:k] = xs[:k]
        out.append(int(np.argmin(((co - q) ** 2).sum(axis=1))))
    return np.asarray(out, dtype=np.int32)


class WaveSolver(SolverBase):
    def __init__(self, case_settings):
        if isinstance(case_settings, dict):
            case_settings.setdefault('scalar_name', 'displacement')
        SolverBase.__init__(self, case_settings)
        self.step_stats = []
        self.state = None
        self.receiver_vertices = np.zeros(0, dtype=np.int32)
        self._traces = self._energy = self._velocity = None
        self._bounds = None

    # ------------------------------------------------------------------ settings (host only)
    def _refuse_unsupported(self):
        from . import parallel
        V = self.function_space
        if V.degree() != 1 or getattr(V, '_ncomp', 1) != 1:
            raise SolverError('WaveSolver: CG{} spaces with {} component(s) are not supported (scalar CG1 only: a lumped P2 mass has '
                              'non-positive vertex weights)'.format(V.degree(), getattr(V, '_ncomp', 1)))
        if parallel.world()[1] > 1:
            raise SolverError('WaveSolver runs on one rank')
        if (hasattr(V, 'periodic_pairs') and V.periodic_pairs() is not None) or self.settings.get('periodic_boundary'):
            raise SolverError('WaveSolver: periodic spaces are not supported')
        ts = self.transient_settings
        if not ts.get('transient'):
            raise SolverError("WaveSolver: 'transient': False - the wave equation has no steady form here")
        if ts.get('time_series') is not None or case.TimeGrid(ts)._constant_step() is None:
            raise SolverError("WaveSolver: non-uniform steps ('time_series') are not supported: a uniform 'time_step' only")
        if self.settings.get('convective_velocity') or getattr(self, 'convective_velocity', None):
            raise SolverError('WaveSolver: an advection velocity (convective_velocity) is not supported')
        if self.settings.get('surface_source'):
            raise SolverError('WaveSolver: surface_source is not supported')
        self.wave_speed()
        self.time_grid()

    def wave_speed(self):
        """c: a number, or an array [n_cells] where it is given per region"""
        c = self.material.get('wave_speed')
        if isinstance(c, numbers.Number) and not isinstance(c, bool):
            c = float(c)
        elif isinstance(c, dict):
            c = case.cellwise_from_regions(c, self.subdomains)
        else:
            raise SolverError("WaveSolver: material 'wave_speed' must be a positive number or a per-region dict, got {!r}".format(c))
        if not (np.all(np.asarray(c) > 0.0) and np.all(np.isfinite(c))):
            raise SolverError("WaveSolver: material 'wave_speed' must be positive")
        return c

    def time_grid(self):
        """(t0, dt, N): the run is N uniform steps from t0"""
        ts = self.transient_settings
        t0, dt, t1 = float(ts['starting_time']), float(ts['time_step']), float(ts['ending_time'])
        if not (dt > 0.0 and np.isfinite(dt)) or not t1 > t0:
            raise SolverError('WaveSolver: time_step {} and the interval [{}, {}] do not make a run'.format(dt, t0, t1))
        N = int(math.ceil((t1 - t0) / dt - 1e-9))
        return t0, dt, max(N, 1)

    def time_factors(self):
        """(s_f [N], s_g [N + 1]): the load factor of every step and the Dirichlet factor of every time point"""
        t0, dt, N = self.time_grid()
        t = t0 + dt * np.arange(N + 1)
        sf = tabulate_time_function(self.settings.get('source_time_function'), t[:N], 'source_time_function')
        sg, owner = None, None
        for name, bc_settings in (self.boundary_conditions or {}).items():
            bc = self.get_boundary_variable(bc_settings)
            if bc['type'] not in ('Dirichlet', 'fixedValue'):
                continue
            tf = bc.get('time_function')
            v = bc.get('value', 0.0)
            if tf is None and isinstance(v, numbers.Number) and float(v) == 0.0:
                continue                  # a homogeneous side takes any factor
            tab = tabulate_time_function(tf, t, "boundary '{}': time_function".format(name))
            if sg is not None and not np.array_equal(tab, sg):
                raise SolverError("WaveSolver: boundaries '{}' and '{}' have different time functions: the Dirichlet values share one "
                                  "factor per step".format(owner, name))
            sg, owner = tab, name
        return sf, (np.ones(N + 1) if sg is None else sg)

    def _nodal_field(self, v, what):
        """a number, an expression string or a nodal array -> nodal values"""
        n = self.function_space.dim()
        if v is None:
            return np.zeros(n)
        if isinstance(v, numbers.Number):
            return np.full(n, float(v))
        if isinstance(v, (str, Constant, Expression, Function)):
            v = Expression(v, degree=1) if isinstance(v, str) else v
            return np.asarray(nodal_values(v, self.function_space), dtype=np.float64).reshape(-1).copy()
        a = np.asarray(v, dtype=np.float64).ravel()
        if a.size != n:
            raise SolverError('WaveSolver: {} holds {} values, the space has {} dofs'.format(what, a.size, n))
        return a.copy()

    def initial_fields(self):
        """(u^0, v^0) as nodal arrays"""
        iv = self.initial_values or {}
        u0 = self._nodal_field(iv.get(self.get_variable_name()), 'initial_values')
        v0 = self._nodal_field(self.settings.get('initial_velocity', iv.get('velocity')), 'initial_velocity')
        if not (np.all(np.isfinite(u0)) and np.all(np.isfinite(v0))):
            raise SolverError('WaveSolver: the initial field or velocity is not finite')
        return u0, v0

    def snap_receivers(self):
        pts = self.settings.get('receivers') or []
        self.receiver_vertices = nearest_vertices(self.mesh.coordinates(), pts) if len(pts) else np.zeros(0, dtype=np.int32)
        if len(pts):
            self.logger.info('WaveSolver: receivers snapped to vertices %s', self.receiver_vertices.tolist())
        return self.receiver_vertices

    def _boundaries(self):
        """(Dirichlet dofs, values, [(marker, flux g)], [absorbing markers]) from the boundary conditions"""
        bcs, flux, absorbing = [], [], []
        for name, bc_settings in (self.boundary_conditions or {}).items():
            i = bc_settings['boundary_id']
            bc = self.get_boundary_variable(bc_settings)
            btype = bc['type']
            if btype in ('Dirichlet', 'fixedValue'):
                bcs.append(DirichletBC(self.function_space, self.translate_value(bc.get('value', 0.0)), self.boundary_facets, i))
            elif btype.lower().find('flux') >= 0:
                g = self.translate_value(bc['value'])
                if is_constant_value(g):
                    g = float(g)
                else:       # a varying flux by the mean of its vertex values on every facet
                    g = np.asarray(nodal_values(g, self.function_space))[self._facets_of(i).astype(np.int64)].mean(axis=1)
                flux.append((i, g))
            elif btype == 'absorbing':
                absorbing.append(i)
            elif btype in ('symmetry', 'natural'):
                pass
            else:
                raise SolverError("WaveSolver: boundary type '{}' is not supported (Dirichlet, flux, absorbing)".format(btype))
        dofs, vals = self._bc_arrays(bcs)
        return dofs, vals, flux, absorbing

    # ------------------------------------------------------------------ the device side
    def _local_facets(self, marker_id, per_facet=None):
        tri = self._facets_of(marker_id)
        loc = self.function_space.localizer()
        if loc is None:
            return tri, per_facet
        ltri, mask = loc.facets(tri)
        if per_facet is not None and np.ndim(per_facet) >= 1:
            per_facet = np.asarray(per_facet)[mask]
        return ltri, per_facet

    def _setup(self):
        """K, m, d, F and the Dirichlet rows on the device, both step bounds, the state object.  Everything here is set-up cost."""
        from . import backend
        self._refuse_unsupported()
        u0, v0 = self.initial_fields()
        sf, sg = self.time_factors()
        dofs, vals, flux, absorbing = self._boundaries()
        self.snap_receivers()
        V = self.function_space.device()
        loc = self.function_space.localizer()
        self._l2g = None if loc is None else np.asarray(loc.l2g, dtype=np.int64)
        n = V.n_owned
        c = self.wave_speed()
        c_cell = None if np.ndim(c) == 0 else (np.asarray(c) if loc is None else loc.cells(c))
        if self.state is not None:
            self.close()
        K = backend.DeviceMatrix(V)
        K.assemble(stiffness=float(c) ** 2 if c_cell is None else ('cell', np.ascontiguousarray(c_cell ** 2)))
        vec = backend.DeviceVector(n)
        backend.assemble_vector(V, vec, source=1.0)                 # the lumped P1 mass: int phi_i dx
        m = vec.get()
        vec.fill(0.0)
        for i in absorbing:
            cells_, _, _ = self._marked_facet_cells(i)
            cf = np.full(len(cells_), float(c)) if c_cell is None else np.asarray(c)[cells_]
            tri, cf = self._local_facets(i, cf)
            if len(tri):
                backend.assemble_facet_vector(V, vec, tri, cf)
        d = vec.get() if absorbing else np.zeros(n)
        vec.fill(0.0)
        for spec in self._source_specs():
            if isinstance(spec, tuple) and loc is not None:
                spec = loc.spec(spec)
            backend.assemble_vector(V, vec, source=spec, add=True)
        for i, g in flux:
            tri, g = self._local_facets(i, g)
            if len(tri):
                backend.assemble_facet_vector(V, vec, tri, g)
        for ps in self._point_source_items():
            pd, pw = (ps.dofs, ps.weights) if loc is None else loc.dofs(ps.dofs, ps.weights)
            vec.add_entries(pd, pw)
        F = vec.get()
        vec.close()
        if loc is not None:
            dofs, vals = loc.dofs(dofs, vals)
        # the two step bounds
        self._bounds = time_marching.step_bounds(self, K, m, dofs)
        t0, dt, N = self.time_grid()
        try:
            time_marching.check_step('WaveSolver', dt, self._bounds, self.logger)
        except SolverError:
            K.close()
            raise
        self._K = K
        self.state = backend.WaveState(V)
        self.state.configure(dt, m, d, F, dofs, vals)
        self._mass = m
        return self._dev(u0), self._dev(v0), sf, sg, dofs, vals

    def _dev(self, a):
        return a if self._l2g is None else np.asarray(a)[self._l2g]

    def _host(self, a):
        if self._l2g is None:
            return a
        out = np.empty_like(a)
        out[self._l2g] = a
        return out

    def _source_specs(self):
        bs = self.get_body_source()
        if not bs:
            return []
        if isinstance(bs, dict):
            cells = self.subdomains.array()
            out = []
            for k, v in bs.items():
                if not is_constant_value(v['value']):
                    raise SolverError("WaveSolver: body source '{}': per-subdomain values must be constants".format(k))
                out.append(('cell', np.where(cells == v['subdomain_id'], float(v['value']), 0.0)))
            return out
        if is_constant_value(bs):
            return [float(bs)]
        if isinstance(bs, (Expression, Function)):
            return [('nodal', np.asarray(nodal_values(bs, self.function_space), dtype=np.float64))]
        raise SolverError('WaveSolver: body source of type {} is not supported'.format(type(bs)))

    def _point_source_items(self):
        ps = self.settings.get('point_source')
        if not ps:
            return []
        if isinstance(ps, PointSource):
            return [ps]
        return [p if isinstance(p, PointSource) else
                PointSource(self.function_space, p[0] if isinstance(p[0], Point) else Point(*np.ravel(p[0])), p[1]) for p in ps]

    def _power_iteration(self, K, m, bc_dofs):
        """lambda_P, a lower bound on the largest eigenvalue of diag(1/m) K on the rows that are not Dirichlet"""
        return time_marching.power_iteration(K, m, bc_dofs, 'WaveSolver')

    def critical_time_step(self):
        """2 / sqrt(lambda_G), lambda_G = max_i sum_j |K_ij| / m_i: the step below which the march is stable"""
        if self._bounds is None:
            self._setup()
        return self._bounds[0]

    def time_step_bounds(self):
        """(2 / sqrt(lambda_G), 2 / sqrt(lambda_P)): stable below the first, certain to blow up above the second"""
        if self._bounds is None:
            self._setup()
        return self._bounds

    def close(self):
        """free the device state and the stiffness"""
        if self.state is not None:
            self.state.close()
            self.state = None
        if getattr(self, '_K', None) is not None:
            self._K.close()
            self._K = None

    # ------------------------------------------------------------------ the march
    def _batch_end(self, n, N):
        """the step at which the batch that starts at step n ends: the next plot / save / energy step, at most batch_steps away"""
        bs = self.settings.get('batch_steps')
        if bs and int(bs) < 1:
            raise SolverError("WaveSolver: 'batch_steps' must be a positive number of steps")
        freqs = (self.report_settings.get('plotting_freq', 0), self.report_settings.get('saving_freq', 0), self.settings.get('energy_freq', 0))
        return time_marching.batch_end(n, N, freqs, int(bs) if bs else None)

    def _publish(self, u_dev):
        self.w_current.vector().set_local(self._host(u_dev))
        self.result = self.w_current

    def solve_transient(self):
        from . import backend
        u0, v0, sf, sg, _, _ = self._setup()
        t0, dt, N = self.time_grid()
        st, K, m = self.state, self._K, self._mass
        rec = self._dev_receivers()
        self.step_stats = []
        self.w_current = Function(self.function_space)
        traces, energy = np.zeros((N + 1, len(rec))), np.zeros((N, 2))
        # step 0 -> 1 on the device; its energy from the two fields (set-up cost: one product)
        st.start(K, u0, v0, sf[0], sg[1])
        _, u1, _ = st.get()
        xd, yd = backend.DeviceVector(len(m), u0), backend.DeviceVector(len(m))
        K.spmv(xd, yd)
        energy[0] = 0.5 * float(np.sum(m * ((u1 - u0) / dt) ** 2)), 0.5 * float(u1 @ yd.get())
        xd.close()
        yd.close()
        traces[0], traces[1] = u0[rec], u1[rec]
        if not np.all(np.isfinite(u1)):
            raise SolverError(self._blow_up_message(0, 1))
        u_before_last = u0
        n = 1                       # the state holds (u^{n-1}, u^n)
        pvd = self.report_settings.get('result_filename') or 'result_file.pvd'
        self.current_step, self.current_time = 1, t0 + dt
        while n < N:
            end = self._batch_end(n, N)
            if end == N and N - n > 1:
                end = N - 1         # the last step runs on its own: velocity() needs u^{N-2}
            k = end - n
            if end == N:
                u_before_last = st.get()[0]
            out = st.advance(K, sf[n:end], sg[n + 1:end + 1], receivers=rec, traces=len(rec) > 0, energy=True, info=True)
            self.step_stats.append({'first_step': n, 'steps': k, 'device_ms': out['device_ms'], 'ms_per_step': out['device_ms'] / k})
            if out['n_nonfinite']:
                raise SolverError(self._blow_up_message(n + out['first_nonfinite_step'], end))
            energy[n:end] = out['energy']
            if len(rec):
                traces[n + 1:end + 1] = out['traces']
            n = end
            self.current_step, self.current_time = n, t0 + n * dt
            if self.settings.get('energy_freq'):
                self.logger.info('WaveSolver: step %d time %g energy %.12g (%.3f ms per step)', n, self.current_time, energy[n - 1].sum(),
                                 self.step_stats[-1]['ms_per_step'])
            if self._due('plotting_freq') or self._due('saving_freq'):
                self._publish(st.get()[1])
                if self._due('plotting_freq'):
                    self.plot()
                if self._due('saving_freq'):
                    self.save(pvd)
        _, uN, _ = st.get()
        self._publish(uN)
        self._velocity = self._host((uN - u_before_last) / (2.0 * dt)) if N > 1 else self._host((uN - u0) / dt)
        self._traces, self._energy = traces, energy
        return self.w_current

    def _dev_receivers(self):
        r = np.asarray(self.receiver_vertices, dtype=np.int64)
        if self._l2g is None or not len(r):
            return r.astype(np.int32)
        g2l = np.empty(len(self._l2g), dtype=np.int64)
        g2l[self._l2g] = np.arange(len(self._l2g))
        return g2l[r].astype(np.int32)

    def _blow_up_message(self, first, end):
        return ('WaveSolver: the field or its energy is not finite in steps {} .. {} (time_step {:.6g}; stable below 2/sqrt(lambda_G) = {:.6g}, certain to '
                'blow up above 2/sqrt(lambda_P) = {:.6g})'.format(first, end, self.time_grid()[1], self._bounds[0], self._bounds[1]))

    def solve(self):
        self.result = self.solve_transient()
        return self.result

    # ------------------------------------------------------------------ results
    def _need(self, what):
        if what is None:
            raise SolverError('WaveSolver: no run has been marched yet')
        return what

    def velocity(self):
        """(u^{n+1} - u^{n-1}) / (2 dt) of the last step, nodal values"""
        return self._need(self._velocity)

    def receiver_traces(self):
        """[n_steps + 1, n_receivers]: the field at the receiver vertices at every time point, t0 included"""
        return self._need(self._traces)

    def energy(self):
        """[n_steps, 2]: (kinetic, potential) halves of the discrete energy of every step"""
        return self._need(self._energy)
