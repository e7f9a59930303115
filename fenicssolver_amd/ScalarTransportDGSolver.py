"""ScalarTransportDGSolver — upwind interior-penalty (SIPG) discontinuous Galerkin advection-diffusion, GPU back end.

Counterpart of FenicsSolver/ScalarTransportDGSolver.py: same class, constructor (``using_diffusion_form = True``, :36-45) and space
set-up (:47-57: ``function_space`` DG1, ``function_space_CG`` CG1, ``vector_function_space``).  The form is the reference's active
branch (:119-147) with kappa = conductivity / capacity, constant velocity beta, alpha = 500 (3-D) / 5 (2-D) and h = 2 circumradius:

    c a(T, v) - N(T; v) - int f v dx = 0,
    a(T, v) = sum_K int_K (kappa grad v . grad T - T beta . grad v) dx
            + sum_F int_F (kappa alpha / h+ [v][T] - kappa {grad v}.n+ [T] - kappa [v] {grad T}.n+ + [v] (b+ T+ - b- T-)) ds
            + sum_boundary int_F v max(beta . n, 0) T ds,

N the boundary terms of ScalarTransportSolver.update_boundary_conditions with the diffusion form (Neumann g, flux g/c, HTC
h/c (T_a - T), Robin g + its Dirichlet part).  '+' of an interior facet: the cell with the lower number in the caller's numbering,
or with the larger cell-region marker where the markers differ (DOLFIN's interior-facet assembler).  The operator, the boundary
loads and the body source are assembled on the device into cell blocks (fs_assemble_dg_transport) and solved by BiCGStab with the
inverse diagonal blocks as preconditioner; ``solve()`` returns the L2 projection onto CG1 (:194-197), ``w_current`` stays DG.

Differences from the reference:
  * Dirichlet values are imposed strongly with DOLFIN's "geometric" rule: every dof whose vertex lies on a marked facet takes the
    boundary value at that vertex (the later boundary condition wins).  The reference's topological DirichletBC finds no dof of a
    DG space and would impose nothing;
  * transient runs use the theta = 1/2 branch of the reference (:109-117) with the active branch's operator and dt =
    get_time_step(step); the active branch has no time derivative;
  * the linear solve is BiCGStab + block Jacobi run to the LU-equivalent tolerance (KRYLOV_RTOL_CAP), not LU.

Refused with SolverError before any device call: fe_degree other than 1, no convective_velocity (the reference raises too,
:158-160), a velocity that is not a constant vector, a conductivity or capacity that is not a constant number, several ranks,
periodic spaces, point_source, surface_source, radiation_settings, advection_settings with a stabilisation method, vector spaces.
"""
from __future__ import annotations

import numbers

import numpy as np

from .fem import Function, FunctionSpace, VectorFunctionSpace, Constant, Expression, UserExpression, is_constant_value
from .SolverBase import SolverError
from .ScalarTransportSolver import ScalarTransportSolver
from . import forms


class ScalarTransportDGSolver(ScalarTransportSolver):
    """Upwind SIPG discontinuous Galerkin solver for advection-diffusion (DG1)."""

    def __init__(self, s):
        ScalarTransportSolver.__init__(self, s)
        self.using_diffusion_form = True
        self.last_solve_stats = None

    # ------------------------------------------------------------------ spaces (ScalarTransportDGSolver.py:47-57)
    def generate_function_space(self, periodic_boundary):
        self.is_mixed_function_space = False
        self.settings['periodic_boundary'] = periodic_boundary
        if periodic_boundary:
            raise SolverError('ScalarTransportDGSolver: periodic spaces are not supported')
        if 'vector_name' in self.settings:
            raise SolverError('ScalarTransportDGSolver: vector-valued DG spaces are not supported')
        degree = self.settings.get('fe_degree', 1)
        if int(degree) != 1:
            raise SolverError('ScalarTransportDGSolver: fe_degree {} is not supported (DG1 only)'.format(degree))
        self.function_space = FunctionSpace(self.mesh, "DG", 1)
        self.function_space_CG = FunctionSpace(self.mesh, "CG", 1)
        self.vector_function_space = VectorFunctionSpace(self.mesh, "CG", 1)

    # ------------------------------------------------------------------ refusals
    def _refuse_unsupported(self):
        from . import parallel
        if parallel.world()[1] > 1:
            raise SolverError('ScalarTransportDGSolver runs on one rank')
        if self.settings.get('periodic_boundary'):
            raise SolverError('ScalarTransportDGSolver: periodic spaces are not supported')
        if int(self.settings.get('fe_degree', 1)) != 1:
            raise SolverError('ScalarTransportDGSolver: fe_degree {} is not supported (DG1 only)'.format(self.settings.get('fe_degree')))
        if 'vector_name' in self.settings:
            raise SolverError('ScalarTransportDGSolver: vector-valued DG spaces are not supported')
        for key in ('point_source', 'surface_source', 'radiation_settings'):
            if self.settings.get(key) or (key == 'radiation_settings' and getattr(self, 'radiation_settings', None)):
                raise SolverError('ScalarTransportDGSolver: {} is not supported'.format(key))
        self._dg_preconditioner()
        ads = self.settings.get('advection_settings')
        if ads and ads.get('stabilization_method'):
            raise SolverError("ScalarTransportDGSolver: advection_settings['stabilization_method'] = {!r}: DG upwinds by construction, "
                              "no stabilisation is added".format(ads.get('stabilization_method')))

    def _constant_material(self, kind):
        try:
            raw = self._raw_coefficient(kind)
        except (SolverError, KeyError, TypeError):
            raw = None                                                   # derived (conductivity = diffusivity * capacity)
        if callable(raw) and not isinstance(raw, (Constant, Expression, Function)):
            raise SolverError('ScalarTransportDGSolver: {} must be a constant (not a function of T)'.format(kind))
        try:
            v = self._coefficient(kind, None)
        except SolverError as e:                                         # e.g. a function of T called without a field
            raise SolverError('ScalarTransportDGSolver: {} must be a constant ({})'.format(kind, e))
        if isinstance(v, forms.VolumeCoefficient) or isinstance(v, (dict, np.ndarray, Expression, Function)):
            raise SolverError('ScalarTransportDGSolver: {} must be a constant number (tensors, per-region and per-cell values are '
                              'not supported: UFL rejects an unrestricted coefficient in the facet integrals)'.format(kind))
        if isinstance(v, Constant):
            if v.value_size() != 1:
                raise SolverError('ScalarTransportDGSolver: {} must be a scalar constant'.format(kind))
            return float(v)
        if isinstance(v, numbers.Number):
            return float(v)
        raise SolverError('ScalarTransportDGSolver: {} of type {} is not supported'.format(kind, type(v)))

    def _constant_velocity(self):
        v = self.settings.get('convective_velocity') if not getattr(self, 'convective_velocity', None) else self.convective_velocity
        if v is None or (not isinstance(v, (Constant, np.ndarray)) and not v):
            raise SolverError('ScalarTransportDGSolver: convective_velocity is required (the reference raises too)')
        if isinstance(v, Constant):
            vals = np.asarray(v.values(), dtype=np.float64).ravel()
        elif isinstance(v, (tuple, list, np.ndarray)) and all(isinstance(c, numbers.Number) for c in np.ravel(np.asarray(v, dtype=object))):
            vals = np.asarray(v, dtype=np.float64).ravel()
        else:
            raise SolverError('ScalarTransportDGSolver: convective_velocity must be a constant vector (got {})'.format(type(v).__name__))
        if vals.size != self.dimension:
            raise SolverError('ScalarTransportDGSolver: convective_velocity must have {} components'.format(self.dimension))
        return vals

    # ------------------------------------------------------------------ the form
    def generate_form(self, time_iter_, T, T_test, T_current, T_prev):
        self._refuse_unsupported()
        F = forms.DGScalarForm(self.function_space)
        F.conductivity = self._constant_material('conductivity')
        F.capacity = self._constant_material('capacity')
        F.velocity = self._constant_velocity()
        F.alpha = 500.0 if self.dimension == 3 else 5.0
        if self.transient_settings['transient']:
            F.transient = True
            F.dt = float(self.get_time_step(time_iter_))
            F.T_prev = T_prev
        self._material_field = None
        bcs, integrals_N = self.update_boundary_conditions(time_iter_, T, T_test, None)
        for item in integrals_N:
            (F.robin if isinstance(item, forms.FacetRobin) else F.facet_loads).append(item)
        items = self.get_body_source_items(time_iter_, T, T_test, None)
        if items:
            F.sources.extend(items)
        return F, bcs

    # ------------------------------------------------------------------ host-side arrays of the device call
    def _boundary_owner(self):
        """facet id -> (caller cell, local facet) of the boundary facets."""
        if getattr(self, '_owner', None) is None:
            cf = self.mesh.cell_facets().astype(np.int64)
            nc, nl = cf.shape
            owner = np.full(self.mesh.num_facets(), -1, dtype=np.int64)
            owner[cf.ravel()] = np.arange(nc * nl)
            self._owner = owner
        return self._owner

    def _facet_arrays(self, marker_id, g):
        """(caller cells, local facets, g at the cells' local vertices [n, d+1]) of ds(marker_id)."""
        sel = self.boundary_facets.where(marker_id)
        nl = self.mesh.cells().shape[1]
        own = self._boundary_owner()[sel]
        cells, local = own // nl, own % nl
        gv = np.zeros((len(sel), nl))
        if np.ndim(g) == 0:
            gv[:] = float(g)
        else:
            g = np.asarray(g, dtype=np.float64).reshape(len(sel), -1)
            fv = self.mesh.facets()[sel].astype(np.int64)                  # [n, d] ascending vertices
            cv = self.mesh.cells().astype(np.int64)[cells]                 # [n, d+1]
            for j in range(fv.shape[1]):
                gv[cv == fv[:, j:j + 1]] = g[:, j]           # one match per row, rows in order
        return cells, local, gv

    def system_arrays(self, F):
        """Everything fs_assemble_dg_transport takes, in the CALLER's cell numbering: facet_cell, facet_local, facet_h, facet_g and
        the body source at every dof (None where absent)."""
        nc, nl = self.mesh.cells().shape
        fc, fl, fh, fg = [], [], [], []
        for load in F.facet_loads:
            c, l, g = self._facet_arrays(load.marker_id, load.g)
            fc.append(c); fl.append(l); fh.append(np.zeros(len(c))); fg.append(g)
        for rb in F.robin:
            c, l, g = self._facet_arrays(rb.marker_id, rb.ambient)
            fc.append(c); fl.append(l); fh.append(np.full(len(c), float(rb.h))); fg.append(float(rb.h) * g)
        src = None
        for s in F.sources:
            if s.kind == "const":
                v = np.full(nc * nl, float(s.value))
            elif s.kind == "cell":
                v = np.repeat(np.asarray(s.value, dtype=np.float64), nl)
            elif s.kind == "nodal":
                v = np.asarray(s.value, dtype=np.float64).ravel()
                if v.size != nc * nl:
                    raise SolverError('body source: {} values for {} DG dofs'.format(v.size, nc * nl))
            else:
                raise SolverError("body source of kind '{}' is not supported by the DG solver".format(s.kind))
            src = v if src is None else src + v
        if fc:
            return (np.concatenate(fc), np.concatenate(fl), np.concatenate(fh), np.concatenate(fg), src)
        return None, None, None, None, src

    # ------------------------------------------------------------------ the solve
    _AMG_NAMES = ('petsc_amg', 'amg', 'hypre_amg', 'ml_amg')
    _BLOCK_SUBSTITUTES = ('sor', 'ilu', 'icc', 'additive_schwarz', 'hypre_euclid', 'hypre_parasails')

    def _dg_preconditioner(self):
        """solver_parameters['preconditioner'] -> the preconditioner of the DG solve: 'default' / 'bjacobi' the inverse diagonal
        blocks, 'jacobi' point Jacobi, 'none' none; the incomplete factorisations and Schwarz methods DOLFIN names run as block
        Jacobi (logged); AMG is refused (no AMG for DG is built)."""
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        pc = sp.get('preconditioner', 'default')
        if pc in ('default', 'bjacobi'):
            return 'block_jacobi'
        if pc == 'jacobi':
            return 'jacobi'
        if pc in ('none', None):
            return 'none'
        if pc in self._AMG_NAMES:
            raise SolverError("ScalarTransportDGSolver: preconditioner '{}' is not available for DG operators (no AMG for DG is "
                              "built): use 'default' / 'bjacobi' (block Jacobi), 'jacobi' or 'none'".format(pc))
        if pc in self._BLOCK_SUBSTITUTES:
            if not getattr(self, '_warned_pc', False):
                self.logger.info("preconditioner '%s': the DG solve uses block Jacobi (the inverse diagonal blocks)", pc)
                self._warned_pc = True
            return 'block_jacobi'
        raise SolverError("preconditioner '{}' is not supported".format(pc))

    def _facet_value(self, value, marker_id, what):
        """Boundary data of ds(marker_id): a number, or [n_facets, d] values at the facet's vertices (ascending vertex order).  A
        varying value is evaluated at the MESH VERTICES (an Expression, a CG Function), or - a Function on the DG space, e.g. an
        expression string of the settings interpolated into it - taken from the one cell behind the boundary facet."""
        if is_constant_value(value):
            return float(value)
        tri = self._facets_of(marker_id).astype(np.int64)
        if isinstance(value, Function) and value.function_space() is self.function_space:
            nl = self.mesh.cells().shape[1]
            own = self._boundary_owner()[self.boundary_facets.where(marker_id)]
            cv = self.mesh.cells().astype(np.int64)[own // nl]                          # [n, d+1]
            dof = (own // nl)[:, None] * nl + np.argmax(cv[:, None, :] == tri[:, :, None], axis=2)
            return np.asarray(value.vector()._values(), dtype=np.float64)[dof]
        if isinstance(value, Function):
            nod = np.asarray(value.vertex_values(), dtype=np.float64)
        elif isinstance(value, (Expression, UserExpression)):
            nod = np.asarray(value.eval_points(self.mesh.coordinates()), dtype=np.float64).reshape(-1)
        else:
            raise SolverError('{}: boundary value of type {} is not supported'.format(what, type(value)))
        if nod.shape[0] != self.mesh.num_vertices():
            raise SolverError('{}: the boundary value must be scalar'.format(what))
        return nod[tri]

    def solve_form(self, F, T_current, bcs):
        from . import backend
        V = self.function_space
        V.set_cell_markers(self.subdomains)
        rec = V.device()
        nl = self.mesh.cells().shape[1]
        n = V.dim()
        cell_a2d = np.empty(len(rec.cell_order), dtype=np.int64)
        cell_a2d[rec.cell_order.astype(np.int64)] = np.arange(len(rec.cell_order))
        fc, fl, fh, fg, src = self.system_arrays(F)
        A = backend.DeviceDGMatrix(rec.space)
        b = backend.DeviceVector(n)
        op = 0.5 if F.transient else 1.0
        mass = F.capacity / F.dt if F.transient else 0.0
        common = dict(conductivity=F.conductivity, capacity=F.capacity, velocity=F.velocity, alpha=F.alpha, mass_scale=mass)
        A.assemble_transport(b, operator_scale=op, facet_cell=None if fc is None else cell_a2d[fc], facet_local=fl, facet_h=fh,
                             facet_g=fg, source=None if src is None else src[rec.device_to_dof], **common)
        if F.transient:
            B = backend.DeviceDGMatrix(rec.space)
            B.assemble_transport(None, operator_scale=-0.5, **common)
            tp = backend.DeviceVector(n, F.T_prev.vector()._values()[rec.device_to_dof])
            y = backend.DeviceVector(n)
            B.spmv(tp, y)
            b.axpy(1.0, y)
            B.close()
        dofs, vals = self._bc_arrays(bcs)
        if len(dofs):
            A.apply_dirichlet(b, rec.dof_to_device[dofs.astype(np.int64)], vals)
        rtol, max_iter, _ = self._krylov_options()
        x = backend.DeviceVector(n, T_current.vector()._values()[rec.device_to_dof])
        stats = backend.dg_krylov_solve(A, b, x, rtol=rtol, max_iter=max_iter, precond=self._dg_preconditioner(), nonzero_guess=True)
        self.last_solve_stats = stats
        if stats['converged'] != 1:
            raise SolverError('ScalarTransportDGSolver: BiCGStab did not converge in {} iterations (relative residual {:.3e})'.format(
                stats['iterations'], stats['true_rel_residual']))
        out = Function(V)
        out.vector().set_local(x.get(n)[rec.dof_to_device])
        A.close()
        return out

    def project_to_cg1(self, T):
        """L2 projection of the DG1 field T onto CG1 (ScalarTransportDGSolver.py:194-197): consistent mass matrix, no boundary
        conditions; the right-hand side gathered on the device (fs_assemble_dg_projection), Jacobi-CG to KRYLOV_RTOL_CAP."""
        from . import backend
        V = self.function_space
        rec = V.device()
        if rec.cg1 is None:
            rec.cg1 = backend.DeviceSpace(rec.mesh, 1, 1)
        nv = self.mesh.num_vertices()
        x = backend.DeviceVector(V.dim(), T.vector()._values()[rec.device_to_dof])
        b = backend.DeviceVector(nv)
        backend.assemble_dg_projection(rec.space, x, rec.cg1, b)
        M = backend.DeviceMatrix(rec.cg1)
        M.assemble(mass=1.0)
        p = backend.DeviceVector(nv)
        rtol, max_iter, _ = self._krylov_options()
        st = backend.krylov_solve(M, b, p, rtol=rtol, max_iter=max_iter, precond="jacobi", method="cg")
        if st['converged'] != 1:
            raise SolverError('ScalarTransportDGSolver: the CG1 projection did not converge')
        P = Function(self.function_space_CG)
        vals = np.empty(nv)
        vals[rec.vertex_order.astype(np.int64)] = p.get(nv)
        P.vector().set_local(vals)
        M.close()
        return P

    def solve_current_step(self):
        ScalarTransportSolver.solve_current_step(self)
        self.result = self.project_to_cg1(self.w_current)

    def solve(self):
        self.solve_transient()
        return self.result

    def save(self, result_filename):
        """The CG1 projection, through the CG path (the reference saves the projected field as well)."""
        w = self.w_current
        self.w_current = self.result
        try:
            ScalarTransportSolver.save(self, result_filename)
        finally:
            self.w_current = w
