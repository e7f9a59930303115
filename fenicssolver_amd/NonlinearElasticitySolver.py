"""NonlinearElasticitySolver — compressible neo-Hookean hyperelasticity on vector P1, GPU back end.

Counterpart of FenicsSolver/NonlinearElasticitySolver.py: same class / constructor (:36-45), energy
psi = mu/2 (Ic - 3) - mu ln J + lambda/2 (ln J)^2 with F = I + grad u, C = F^T F, Ic = tr C, J = det F (:47-68), total
potential Pi = int psi dx - int B.u dx - the boundary loads of update_boundary_conditions with v = u (:70-88), solved by
Newton on dPi/du = 0 with the tangent d^2 Pi/du^2 (:90-98).  In 2-D (plane strain) the reference's Identity(2) with the
constant 3 is kept: it shifts the energy by -mu/2 per unit area and changes nothing else.

The tangent, the internal force and the energy are assembled on the device at every iterate (fs_assemble_hyperelastic); the
loads are dead loads (force, pressure and stress act on the reference configuration's normals and areas) and are assembled
once per load step.  The Newton loop (SolverBase._hyperelastic_newton) uses DOLFIN's defaults and stopping test; each step is
CG + AMG with the rigid-body near-null space in 3-D and Jacobi-CG in 2-D.  A trial step that inverts a cell is halved.

Differences from the reference:
  * the loads enter Pi with their physical sign (``reference_load_sign`` of the linear class does not apply);
  * transient settings mean quasi-static load stepping: each step solves equilibrium for that step's boundary values and
    loads, starting from the previous step's solution.  The reference's kinetic term uses an undefined ``dt`` and cannot run;
  * ``temperature_distribution`` raises SolverError (the energy has no thermal term; the reference ignores it silently);
  * ``surface_source`` keeps the reference's semantics: with a ``direction`` it adds nothing, without one it adds the normal
    traction value * n on the whole exterior boundary (the linear class refuses it);
  * P2 spaces, several ranks, periodic spaces and ``point_source`` raise SolverError before any device call.
"""
from __future__ import annotations

import numpy as np

from .fem import Measure, is_constant_value
from .SolverBase import SolverError
from .LinearElasticitySolver import LinearElasticitySolver
from . import forms


class NonlinearElasticitySolver(LinearElasticitySolver):
    _constraint_sides = False          # 'contact' / 'sliding' sides stay with the static linear solver

    def __init__(self, case_settings):
        LinearElasticitySolver.__init__(self, case_settings)
        self.settings['mixed_variable'] = ('displacement', 'velocity', 'pressure')
        self.reference_load_sign = False          # the loads of Pi have their physical sign (varying pressure: NodalLoad)
        self.newton_iterations = 0
        self.newton_history = []

    def _refuse_unsupported(self):
        from . import parallel
        V = self.function_space
        if V.degree() != 1:
            raise SolverError('NonlinearElasticitySolver: CG{} displacements are not supported (vector CG1 only: the P2 integrand '
                              'is not polynomial)'.format(V.degree()))
        if parallel.world()[1] > 1:
            raise SolverError('NonlinearElasticitySolver runs on one rank')
        if (hasattr(V, 'periodic_pairs') and V.periodic_pairs() is not None) or self.settings.get('periodic_boundary'):
            raise SolverError('NonlinearElasticitySolver: periodic spaces are not supported')
        T = getattr(self, 'temperature_distribution', None) or self.settings.get('temperature_distribution')
        if T is not None and not (isinstance(T, (int, float)) and T == 0):
            raise SolverError('NonlinearElasticitySolver: temperature_distribution is not supported - the neo-Hookean energy has no '
                              'thermal term (the reference ignores the setting)')

    def update_boundary_conditions(self, time_iter_, u, v, ds):
        """The linear class's boundary conditions (loads without a sign: Pi subtracts them), plus surface_source with the
        reference's semantics (LinearElasticitySolver.py:111-116)."""
        ss = self.settings.get('surface_source')
        if not ss:
            return LinearElasticitySolver.update_boundary_conditions(self, time_iter_, u, v, ds)
        self.settings['surface_source'] = None
        try:
            bcs, integrals = LinearElasticitySolver.update_boundary_conditions(self, time_iter_, u, v, ds)
        finally:
            self.settings['surface_source'] = ss
        load = self._surface_source_load(ss)
        if load is not None:
            integrals.append(load)
        return bcs, integrals

    def _surface_source_load(self, ss):
        value, direction = (ss.get('value'), ss.get('direction')) if isinstance(ss, dict) else (ss, None)
        if direction is not None:
            # the reference's branch with a direction builds the term and never adds it
            self.logger.info('surface_source with a direction adds no load (as in the reference)')
            return None
        g = self.translate_value(value)
        if not is_constant_value(g):
            raise SolverError('surface_source: the value must be a constant')
        mesh = self.mesh
        tri, nrm, area = self._normals_of_facets(np.nonzero(mesh.exterior_facets())[0])
        d = tri.shape[1]
        loads = (float(g) * area / d)[:, None, None] * np.broadcast_to(nrm[:, None, :], (len(tri), d, self.dimension))
        dofs = tri[:, :, None] * self.dimension + np.arange(self.dimension)[None, None, :]
        return forms.NodalLoad(dofs, loads, 'surface_source(normal)')

    def generate_form(self, time_iter_, u, v, u_current, u_prev):
        self._refuse_unsupported()
        F = forms.HyperelasticForm(self.function_space)
        F.mu, F.lmbda = self.lame_parameters()
        bcs, integrals = self.update_boundary_conditions(time_iter_, u, u_current, Measure("ds", subdomain_data=self.boundary_facets))
        F.tractions.extend(integrals)
        if self.body_source:
            self._set_body_force(F)
        return F, bcs

    def solve_form(self, F, u_, bcs):
        return self.solve_nonlinear_problem(F, u_, bcs, None)
