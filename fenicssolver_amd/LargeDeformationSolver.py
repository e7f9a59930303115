"""LargeDeformationSolver — transient large-deformation elasticity with mixed CG1 (u, v, p), GPU back end.

Counterpart of FenicsSolver/LargeDeformationSolver.py: a subclass of NonlinearElasticitySolver on MixedElement([V, V, Q])
(:47-56) with the Crank-Nicolson (q = 1/2) forms of :80-135 - F = I + grad u, J = det F, S = J (-p I + mu (B - I)) F^-T,
pp = p / lambda + J^2 - 1 -
    F1 = (1/dt) <u - u0, _u> - q <v, _u> - (1-q) <v0, _u>
    F2 = (1/dt) <v - v0, _v> + q (<S, grad _v> + <pp, _p>) + (1-q) (<S0, grad _v> + <pp0, _p>)
plus the boundary integrals of update_boundary_conditions with the follower flux get_flux(u, g) = J F^-T g (:58-62), added with
the sign as written (reference_load_sign), and <body_source, _v>.  solve(F == 0, w, bcs, J) with Newton absolute 1e-9 /
relative 1e-7 (:137-140) and DOLFIN's other defaults (50 iterations, relaxation 1).

Every Newton iterate is ONE device assembly (fs_assemble_large_deformation): the u rows are linear, so du = dt (q dv - r_u) is
eliminated exactly and the device assembles the (v, p) system on a CG1 block-4 space, its right-hand side and the norm of the full
(u, v, p) residual.  The step is FGMRES (fs_saddle_solve, block_upper) to 1e-10 relative, right-preconditioned by [A J_vp; 0 S]^-1
with A ~ M/dt + q^2 dt K(mu, lambda = 0) (one AMG V-cycle in 3-D, built once per time step size; Jacobi-CG in 2-D) and
S = q (1/lambda + 1/mu) M_p.

Differences from the reference:
  * save() writes one VTU per call with the point fields displacement, velocity and pressure (the reference's save() only prints);
  * refused with SolverError before any device call: steady settings (as the reference), nu >= 0.5 (equal-order P1/P1 is not
    inf-sup stable; the reference leans on MUMPS), fe_degree != 1, several ranks, periodic spaces, non-constant E or nu,
    point_source, surface_source, temperature_distribution, an unknown 'variable', loads that vary over a boundary, and the
    Neumann / symmetry types (as the reference);
  * the elimination of du reproduces the monolithic Newton step only where every Dirichlet displacement dof also has a prescribed
    velocity with u_D = u0 + dt (q v_D + (1-q) v0) (a clamp, or a displacement moved with its velocity); other displacement
    conditions - 'variable': 'displacement' alone among them - raise SolverError before the step's first device call.
"""
from __future__ import annotations

import numbers
import os

import numpy as np

from .fem import Constant, Function, is_constant_value
from .SolverBase import SolverError, write_vtu
from .LinearElasticitySolver import LinearElasticitySolver
from .NonlinearElasticitySolver import NonlinearElasticitySolver
from .mixed import LargeDeformationSpace, split_large_deformation


class LargeDeformationForm:
    """What generate_form hands to solve_form: the step's coefficients, Dirichlet sets and follower loads."""

    def __init__(self, dt, q, mu, lmbda):
        self.dt, self.q, self.mu, self.lmbda = float(dt), float(q), float(mu), float(lmbda)
        self.body_force = None
        self.loads = []              # (facet ids, g [n_facets, d]) - integrated as J F^-T g . _v ds


class LargeDeformationSolver(NonlinearElasticitySolver):
    SCHUR_SCALE = 1.0                # S = SCHUR_SCALE * q (1/lambda + 1/mu) M_p
    NEWTON_ATOL, NEWTON_RTOL, NEWTON_MAX_IT = 1e-9, 1e-7, 50
    KRYLOV_RTOL = 1e-10
    KRYLOV_MAX_IT = 600
    KRYLOV_STALL_RTOL = 1e-8
    von_Mises = LinearElasticitySolver.von_Mises      # as before: the Cauchy-stress results of the parent read a plain displacement space

    def __init__(self, case_settings):
        NonlinearElasticitySolver.__init__(self, case_settings)
        case_settings['vector_name'] = 'displacement'
        self.reference_load_sign = True
        self.amg_setups = 0
        self.step_newton_iterations = []     # Newton iterations of every time step
        self.step_krylov_iterations = []     # FGMRES iterations of every Newton step, per time step
        self.step_history = []               # (u, v, p) host copies after every step (only with keep_history)
        self.keep_history = False
        self._dev = None

    # ------------------------------------------------------------------ space
    def generate_function_space(self, periodic_boundary):
        self.is_mixed_function_space = True
        if periodic_boundary:
            raise SolverError('LargeDeformationSolver: periodic spaces are not supported')
        if int(self.settings.get('fe_degree', 1)) != 1:
            raise SolverError('LargeDeformationSolver: fe_degree {} is not supported (CG1 only: the P2 integrands are not '
                              'polynomial)'.format(self.settings.get('fe_degree')))
        if self.settings.get('fe_family', 'CG') not in ('CG', 'P', 'Lagrange'):
            raise SolverError("fe_family '{}' is not supported".format(self.settings.get('fe_family')))
        self.settings['periodic_boundary'] = None
        self.function_space = LargeDeformationSpace(self.mesh)

    def _refuse_unsupported(self):
        from . import parallel
        if not self.transient_settings['transient']:
            raise SolverError('large deformation solver must be solved in a transient way')
        if parallel.world()[1] > 1:
            raise SolverError('LargeDeformationSolver runs on one rank')
        if self.settings.get('periodic_boundary'):
            raise SolverError('LargeDeformationSolver: periodic spaces are not supported')
        if int(self.settings.get('fe_degree', 1)) != 1:
            raise SolverError('LargeDeformationSolver: CG1 only')
        for key in ('point_source', 'surface_source', 'temperature_distribution'):
            if self.settings.get(key):
                raise SolverError('LargeDeformationSolver: {} is not supported'.format(key))
        if getattr(self, 'temperature_distribution', None):
            raise SolverError('LargeDeformationSolver: temperature_distribution is not supported')

    def material_constants(self):
        E, nu = self.material_field('elastic_modulus'), self.material_field('poisson_ratio')
        if np.ndim(E) != 0 or np.ndim(nu) != 0:
            raise SolverError('LargeDeformationSolver: elastic_modulus and poisson_ratio must be constants')
        E, nu = float(E), float(nu)
        if not (E > 0.0):
            raise SolverError('LargeDeformationSolver: elastic_modulus must be positive')
        if not (-1.0 < nu < 0.5):
            raise SolverError('LargeDeformationSolver: poisson_ratio {} is not supported (nu < 0.5: the equal-order P1/P1 pair is not '
                              'inf-sup stable, the pressure block of an incompressible material is singular)'.format(nu))
        return E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))

    # ------------------------------------------------------------------ boundary conditions (LinearElasticitySolver.py:135-200)
    def _bc_value(self, value, size, name):
        """A constant vector of `size` numbers (None entries kept as None)."""
        if isinstance(value, Constant):
            v = list(value.values())
        elif isinstance(value, numbers.Number):
            v = [float(value)]
        elif isinstance(value, (tuple, list, np.ndarray)):
            v = list(value)
        else:
            raise SolverError("boundary '{}': a constant value is required, got {}".format(name, type(value).__name__))
        out = []
        for c in v:
            if c is None:
                out.append(None)
                continue
            c = self.translate_value(c) if isinstance(c, str) else c
            if isinstance(c, Constant):
                c = float(c)
            if not isinstance(c, numbers.Number):
                raise SolverError("boundary '{}': a constant value is required".format(name))
            out.append(float(c))
        if len(out) != size:
            raise SolverError("boundary '{}': {} values expected, got {}".format(name, size, len(out)))
        return out

    def update_boundary_conditions(self, time_iter_, u, v, ds):
        """(Dirichlet list [(field, component, vertices, value)], loads [(facet ids, g[nf, d])])."""
        d = self.dimension
        bcs, loads = [], []
        for name, bc_settings in self.boundary_conditions.items():
            i = bc_settings['boundary_id']
            bc = self.get_boundary_variable(bc_settings)
            btype = bc['type']
            facets = self.boundary_facets.where(i)
            if btype in ('Dirichlet', 'displacement'):
                verts = np.unique(self.mesh.facets()[facets].astype(np.int64).ravel())
                var = bc.get('variable', 'displacement')
                if var == 'displacement':
                    vals = self._bc_value(bc['value'], d, name)
                    bcs.extend(('u', k, verts, c) for k, c in enumerate(vals) if c is not None)
                elif var == 'velocity':
                    vals = self._bc_value(bc['value'], d, name)
                    bcs.extend(('v', k, verts, c) for k, c in enumerate(vals) if c is not None)
                elif var == 'all':
                    vals = self._bc_value(bc['value'], 2 * d + 1, name)
                    bcs.extend(('u', k, verts, vals[k]) for k in range(d))
                    bcs.extend(('v', k, verts, vals[d + k]) for k in range(d))
                    bcs.append(('p', 0, verts, vals[2 * d]))
                else:
                    raise SolverError("boundary '{}': variable '{}' is not supported (displacement, velocity or all)".format(name, var))
            elif btype == 'force':
                val = bc['value']
                tri, nrm, area = self._facet_normals(i)
                if isinstance(val, (tuple, list)) and len(val) == d:
                    g = np.tile(self._vector_of(val, name), (len(tri), 1))          # a traction density (:166-167)
                else:
                    f = self.translate_value(val)
                    if not is_constant_value(f):
                        raise SolverError("boundary '{}': force magnitude must be a constant".format(name))
                    gmag = float(f) / self._total_area(tri, area)                 # spread over the marked area (:170-178)
                    g = (np.tile(self._vector_of(bc['direction'], name), (len(tri), 1)) if bc.get('direction') else nrm) * gmag
                loads.append((facets, g))
            elif btype == 'pressure':
                pv = self.translate_value(bc['value'])
                if not is_constant_value(pv):
                    raise SolverError("boundary '{}': LargeDeformationSolver needs a constant pressure".format(name))
                tri, nrm, area = self._facet_normals(i)
                dirn = np.tile(self._vector_of(bc['direction'], name), (len(tri), 1)) if bc.get('direction') else nrm
                loads.append((facets, dirn * float(pv)))
            elif btype == 'stress':
                g = self.translate_value(bc['value'])
                tri, nrm, area = self._facet_normals(i)
                if isinstance(g, Constant) and g.value_size() == d:
                    loads.append((facets, np.tile(g.values(), (len(tri), 1))))
                elif isinstance(g, Constant) and g.value_size() == d * d:
                    loads.append((facets, nrm @ g.values().reshape(d, d).T))
                else:
                    raise SolverError("boundary '{}': stress must be a constant vector or tensor".format(name))
            elif btype in ('Neumann', 'symmetry'):
                raise SolverError('{} boundary type`{}` is not supported'.format(btype, btype))
            else:
                raise SolverError('boundary type`{}` is not supported'.format(btype))
        return bcs, loads

    # ------------------------------------------------------------------ the form
    def generate_form(self, time_iter_, w_trial, w_test, w_current, w_prev):
        self._refuse_unsupported()
        mu, lmbda = self.material_constants()
        F = LargeDeformationForm(self.get_time_step(time_iter_), 0.5, mu, lmbda)
        bcs, F.loads = self.update_boundary_conditions(time_iter_, None, None, None)
        if self.body_source:
            F.body_force = tuple(float(x) for x in self._vector_of(self.body_source, 'body_source'))
        return F, bcs

    # ------------------------------------------------------------------ device state
    def _device(self):
        if self._dev is None:
            from . import backend
            W = self.function_space
            V = W.displacement_space()
            Vd = V.device()
            loc = V.localizer()
            nv, nc = self.mesh.num_vertices(), self.mesh.num_cells()
            dev = {'V': Vd, 'loc': loc, 'nv': nv}
            if loc is None:
                dev['l2h'] = None
                dev['cell_h2d'] = np.arange(nc)
            else:
                dev['l2h'] = np.asarray(loc.l2g, dtype=np.int64)
                c2h = np.asarray(loc.cells(np.arange(nc)), dtype=np.int64)
                h2d = np.empty(nc, dtype=np.int64)
                h2d[c2h] = np.arange(nc)
                dev['cell_h2d'] = h2d
            dev['W4'] = backend.DeviceSpace(Vd.mesh, 4, 1)
            dev['Q'] = backend.DeviceSpace(Vd.mesh, 1, 1)
            dev['J'] = backend.DeviceMatrix(dev['W4'])
            dev['Mp'] = backend.DeviceMatrix(dev['Q'])
            dev['Mp'].assemble(mass=1.0)
            d = self.dimension
            dev['u'], dev['u0'] = backend.DeviceVector(nv * d), backend.DeviceVector(nv * d)
            dev['w'], dev['w0'] = backend.DeviceVector(nv * 4), backend.DeviceVector(nv * 4)
            dev['rhs'], dev['dx'] = backend.DeviceVector(nv * 4), backend.DeviceVector(nv * 4)
            dev['a0_key'] = None
            self._dev = dev
        return self._dev

    def _to_dev_nodes(self, a):
        l2h = self._dev['l2h']
        return np.ascontiguousarray(a if l2h is None else a[l2h])

    def _to_host_nodes(self, a):
        l2h = self._dev['l2h']
        if l2h is None:
            return a
        out = np.empty_like(a)
        out[l2h] = a
        return out

    def _velocity_operator(self, F, vdofs):
        """A0 = M/dt + q^2 dt K(mu, lambda = 0) with the velocity-Dirichlet dofs eliminated, and its AMG hierarchy (3-D): built
        when dt or the Dirichlet set changes."""
        from . import backend
        dev = self._dev
        key = (F.dt, F.q, F.mu, vdofs.tobytes())
        if dev['a0_key'] == key:
            return dev['A0'], dev['A0_amg']
        A0 = backend.DeviceMatrix(dev['V'])
        A0.assemble(lame=(F.q * F.q * F.dt * F.mu, 0.0), mass=1.0 / F.dt)
        if vdofs.size:
            A0.apply_dirichlet(None, vdofs, 0.0, symmetric=True)
        amg = None
        if self.dimension == 3:
            amg = backend.AMG(A0, nullspace="rigid_body")
            self.amg_setups += 1
        dev['A0'], dev['A0_amg'], dev['a0_key'] = A0, amg, key
        return A0, amg

    # ------------------------------------------------------------------ the solve
    def _refuse_inexact_elimination(self, F, fixed, u, v, u0, v0):
        """The elimination du = dt (q dv - r_u) reproduces the monolithic Newton step only where r_u = 0 at every Dirichlet
        displacement dof: R_u = M r_u with the consistent mass matrix couples the free u rows to the Dirichlet ones, and a non-zero
        r_u there would be spread over the free rows by M_FF^-1 M_FD - no local elimination gives that.  r_u = 0 holds when the
        velocity of the same dof is prescribed too and the values agree with the step: u_D = u0 + dt (q v_D + (1-q) v0) - a clamp,
        or a displacement moved with its prescribed velocity.  Anything else is refused before the step's first device call."""
        d, dt, q = self.dimension, F.dt, F.q
        nv = self.mesh.num_vertices()
        for k in range(d):
            ud = np.zeros(nv, dtype=bool)
            vd = np.zeros(nv, dtype=bool)
            for verts, _ in fixed['u'][k]:
                ud[verts] = True
            for verts, _ in fixed['v'][k]:
                vd[verts] = True
            if not ud.any():
                continue
            if (ud & ~vd).any():
                raise SolverError('LargeDeformationSolver: displacement component {} is prescribed on {} vertices without a prescribed '
                                  'velocity there; the displacement is eliminated from the Newton system, which needs the velocity of '
                                  'every Dirichlet displacement dof too (add a velocity condition on the same boundary, or use '
                                  "'variable': 'all')".format(k, int((ud & ~vd).sum())))
            ru = (u[ud, k] - u0[ud, k]) - dt * (q * v[ud, k] + (1.0 - q) * v0[ud, k])
            scale = 1.0 + np.abs(u[ud, k]).max() + np.abs(u0[ud, k]).max() + dt * (np.abs(v[ud, k]).max() + np.abs(v0[ud, k]).max())
            if np.abs(ru).max() > 1e-12 * scale:
                raise SolverError('LargeDeformationSolver: time step {}: the prescribed displacement of component {} does not follow '
                                  'from the prescribed velocity (u_D - u0 - dt (q v_D + (1-q) v0) = {:.3e}); the displacement is '
                                  'eliminated from the Newton system, which needs u_D = u0 + dt (q v_D + (1-q) v0) at every Dirichlet '
                                  'displacement dof'.format(self.current_step, k, float(np.abs(ru).max())))

    def solve_form(self, F, w_, bcs):
        from . import backend
        d = self.dimension
        nv = self.mesh.num_vertices()
        W = self.function_space
        # Dirichlet sets on host vertices: mask bits (0-2 u, 3-5 v, 6 p) and values
        mask = np.zeros(nv, dtype=np.uint8)
        fixed = {'u': [[] for _ in range(d)], 'v': [[] for _ in range(d)], 'p': [[]]}
        for field, k, verts, val in bcs:
            bit = {'u': k, 'v': 3 + k, 'p': 6}[field]
            mask[verts] |= np.uint8(1 << bit)
            fixed[field][k].append((verts, val))
        u, v, p = (np.array(a, dtype=np.float64) for a in W.blocks(w_))
        u0, v0, p0 = (np.array(a, dtype=np.float64) for a in W.blocks(self.w_prev))
        for field, arr in (('u', u), ('v', v), ('p', p[:, None])):
            for k, lst in enumerate(fixed[field]):
                for verts, val in lst:                     # later conditions win, as later DirichletBCs do
                    arr[verts, k] = val
        u_free = ~((mask[:, None] >> np.arange(d)[None, :]) & 1).astype(bool)
        self._refuse_inexact_elimination(F, fixed, u, v, u0, v0)
        dev = self._device()
        # facets -> (device cell, local opposite vertex, g)
        cf = self.mesh.cell_facets()
        fc_l, fo_l, fg_l = [], [], []
        if F.loads:
            owner = np.full(self.mesh.num_facets(), -1, dtype=np.int64)
            owner_loc = np.full(self.mesh.num_facets(), -1, dtype=np.int64)
            owner[cf.ravel()] = np.repeat(np.arange(len(cf)), cf.shape[1])
            owner_loc[cf.ravel()] = np.tile(np.arange(cf.shape[1]), len(cf))
            for facets, g in F.loads:
                facets = np.asarray(facets, dtype=np.int64)
                fc_l.append(dev['cell_h2d'][owner[facets]])
                fo_l.append(owner_loc[facets])
                fg_l.append(np.asarray(g, dtype=np.float64).reshape(len(facets), d))
        fcell = np.concatenate(fc_l).astype(np.int32) if fc_l else None
        fopp = np.concatenate(fo_l).astype(np.int32) if fo_l else None
        fg = np.concatenate(fg_l) if fg_l else None
        vdofs = np.sort(np.concatenate([self._to_dev_nodes_index(np.asarray(vv, dtype=np.int64)) * d + k
                                        for k in range(d) for vv, _ in fixed['v'][k]] or [np.zeros(0, dtype=np.int64)])).astype(np.int32)
        A0, amg = self._velocity_operator(F, np.unique(vdofs))
        dev['u0'].set(self._to_dev_nodes(u0).reshape(-1))
        dev['w0'].set(self._block(self._to_dev_nodes(v0), self._to_dev_nodes(p0)))
        dmask = self._to_dev_nodes(mask)
        body = F.body_force or (0.0,) * d
        dt, q = F.dt, F.q
        schur = self.SCHUR_SCALE * q * (1.0 / F.lmbda + 1.0 / F.mu)
        r0 = None
        its = []
        self.newton_history = []
        for it in range(self.NEWTON_MAX_IT + 1):
            dev['u'].set(self._to_dev_nodes(u).reshape(-1))
            dev['w'].set(self._block(self._to_dev_nodes(v), self._to_dev_nodes(p)))
            info = backend.assemble_large_deformation(dev['J'], dev['rhs'], dev['u'], dev['w'], dev['u0'], dev['w0'], dt, q, F.mu,
                                                      F.lmbda, dmask, body_force=tuple(body) + (0.0,) * (3 - d),
                                                      facet_cell=fcell, facet_opposite=fopp, facet_g=fg)
            if info['n_bad']:
                raise SolverError('LargeDeformationSolver: time step {}, Newton iteration {}: {} cell(s) with a singular deformation '
                                  'gradient (J = 0 or not finite), first cell {}'.format(self.current_step, it, info['n_bad'],
                                                                                          info['first_bad_cell']))
            rn = info['residual_norm']
            if not np.isfinite(rn):
                raise SolverError('LargeDeformationSolver: time step {}, Newton iteration {}: the residual is not finite'.format(
                    self.current_step, it))
            self.newton_history.append(rn)
            if r0 is None:
                r0 = rn
            if rn < self.NEWTON_ATOL or (r0 > 0 and rn / r0 < self.NEWTON_RTOL):
                break
            if it == self.NEWTON_MAX_IT:
                raise SolverError('LargeDeformationSolver: time step {}: Newton did not converge in {} iterations (residual {:.3e})'.format(
                    self.current_step, self.NEWTON_MAX_IT, rn))
            st = backend.large_deformation_solve(dev['J'], dev['Mp'], dev['rhs'], dev['dx'], A0, schur, a0_amg=amg,
                                                 rtol=self.KRYLOV_RTOL, max_iter=self.KRYLOV_MAX_IT)
            self.last_solve_stats = st
            if st['converged'] == 0 and st['rel_residual'] <= self.KRYLOV_STALL_RTOL:
                # 1e-10 relative is at the edge of what fp64 FGMRES attains on large meshes (it stalls at 1.3e-10 on 730 k vertices);
                # a step this accurate is kept - the Newton test is on the true full residual
                self.logger.info('LargeDeformationSolver: FGMRES stalled at %.2e (target %.0e); step kept', st['rel_residual'],
                                 self.KRYLOV_RTOL)
            elif st['converged'] != 1:
                raise SolverError('LargeDeformationSolver: time step {}, Newton iteration {}: FGMRES did not converge ({} iterations, '
                                  'relative residual {:.3e})'.format(self.current_step, it, st['iterations'], st['rel_residual']))
            its.append(st['iterations'])
            dw = self._to_host_nodes(dev['dx'].get()[:4 * nv].reshape(nv, 4))
            if not np.all(np.isfinite(dw)):
                raise SolverError('LargeDeformationSolver: time step {}: the Newton correction is not finite'.format(self.current_step))
            dv, dp = dw[:, :d], dw[:, 3]
            ru = (u - u0) / dt - q * v - (1.0 - q) * v0
            du = np.where(u_free, dt * (q * dv - ru), 0.0)
            u, v, p = u + du, v + dv, p + dp
        self.newton_iterations = len(its)
        self.step_newton_iterations.append(len(its))
        self.step_krylov_iterations.append(its)
        out = np.concatenate([u, v, p[:, None]], axis=1).reshape(-1)
        w_.vector().set_local(out)
        if self.keep_history:
            self.step_history.append((u.copy(), v.copy(), p.copy()))
        return w_

    def _to_dev_nodes_index(self, host_nodes):
        """device node numbers of host vertices"""
        l2h = self._dev['l2h']
        if l2h is None:
            return host_nodes
        h2l = np.empty(len(l2h), dtype=np.int64)
        h2l[l2h] = np.arange(len(l2h))
        return h2l[host_nodes]

    @staticmethod
    def _block(v, p):
        nv, d = v.shape
        b = np.zeros((nv, 4))
        b[:, :d] = v
        b[:, 3] = p
        return b.reshape(-1)

    # ------------------------------------------------------------------ results
    def split(self, w=None):
        return split_large_deformation(self.w_current if w is None else w)

    def displacement(self):
        return self.split()[0]

    def velocity(self):
        """(u - u0) / dt, as the reference (the velocity unknown itself is split()[1])."""
        W = self.function_space
        dt = self.get_time_step(self.current_step)
        u, _, _ = W.blocks(self.w_current)
        u0, _, _ = W.blocks(self.w_prev)
        out = Function(W.displacement_space())
        out.vector().set_local(((u - u0) / dt).reshape(-1))
        return out

    def save(self, result_filename):
        """One ASCII VTU per call with the point fields displacement, velocity and pressure, and the PVD collection (the reference's
        save() prints an error and writes nothing)."""
        assert result_filename[-4:] == '.pvd'
        root = result_filename[:-4]
        if not hasattr(self, '_saved_frames'):
            self._saved_frames = []
        vtu = "%s%06d.vtu" % (root, len(self._saved_frames))
        u, v, p = self.split()
        write_vtu(vtu, self.mesh, u, 'displacement', extra=[(v, 'velocity'), (p, 'pressure')])
        self._saved_frames.append((getattr(self, 'current_time', 0.0), os.path.basename(vtu)))
        with open(result_filename, "w") as fh:
            fh.write('<?xml version="1.0"?>\n<VTKFile type="Collection" version="0.1">\n  <Collection>\n')
            for t, f in self._saved_frames:
                fh.write('    <DataSet timestep="%g" part="0" file="%s" />\n' % (t, f))
            fh.write('  </Collection>\n</VTKFile>\n')

    def plot(self):
        return None

    def solve_modal(self):
        raise SolverError('LargeDeformationSolver has no modal analysis')


