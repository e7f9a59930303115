"""PlasticitySolver — rate-independent small-strain von Mises (J2) plasticity with linear isotropic hardening on vector P1, GPU
back end.

The reference lists "plasticity" among its solvers (Readme.md), its LinearElasticitySolver.py says "plasticity will be implemented
in PlasticitySolver" and examples/run_all_tests.py names a test_plasticity.py; none of them exists.  This class fills the gap
with the textbook model, so there is no reference counterpart to diff against; the independent check is the numpy
restatement tests/plasticity_reference.py.

Model: eps = sym grad u, one integration point per cell (CG1: constant strain); history per cell: the plastic strain eps_p
(symmetric, trace-free; plane strain keeps the zz component: eps_zz = 0 but eps_p,zz and sigma_zz are not) and the cumulative
plastic strain p.  Trial stress sigma_tr = K tr(eps - eps_p) I + 2 G dev(eps - eps_p), q = sqrt(3/2) |dev sigma_tr|,
f = q - (yield_stress + hardening_modulus p); f <= 0 is elastic, f > 0 the radial return with the consistent tangent.  Return
mapping, tangent and internal force are evaluated on the device at every iterate (fs_assemble_plasticity); the Newton loop
(solid_steps.plastic_newton) uses DOLFIN's defaults and stopping test; each step is CG + AMG with the rigid-body near-null space in
3-D and Jacobi-CG in 2-D.  The history is committed when a load step has converged.

Settings: material ``yield_stress`` (> 0, required) and ``hardening_modulus`` (H = d sigma_y / dp >= 0, default 0; the uniaxial
tangent modulus is E H / (E + H)), numbers or per-region dicts like ``elastic_modulus`` and ``poisson_ratio``.  Transient settings
mean quasi-static load steps, as in NonlinearElasticitySolver: boundary values and loads may be per-step sequences or callables of
time.  Loads are dead loads with their physical sign.  P2 spaces, several ranks, periodic spaces, ``temperature_distribution``,
``point_source`` and ``surface_source``, a missing or non-positive yield stress, H < 0 and a Poisson ratio >= 0.5 raise SolverError
before any device call.

Results: ``solve()`` returns the displacement; ``cumulative_plastic_strain()``, ``plastic_strain()`` and ``stress()`` return per-cell
arrays of the last converged step in the caller's cell numbering (tensors as (xx, yy, zz, xy, xz, yz) in 3-D and (xx, yy, zz, xy)
in plane strain); ``von_Mises()`` projects the von Mises value of the RETURNED stress onto CG1.  ``newton_iterations``,
``newton_history`` and ``newton_stats`` describe the last step; ``yielded_cells`` and ``newton_iterations_per_step`` hold one entry
per converged step.
"""
from __future__ import annotations

import numpy as np

from .fem import Measure
from .SolverBase import SolverError
from .LinearElasticitySolver import LinearElasticitySolver
from .stored_stress import StoredStressVonMises
from . import forms, solid_steps


class PlasticitySolver(StoredStressVonMises, LinearElasticitySolver):
    _constraint_sides = False          # 'contact' / 'sliding' sides stay with the static linear solver

    def __init__(self, case_settings):
        LinearElasticitySolver.__init__(self, case_settings)
        self.reference_load_sign = False          # dead loads with their physical sign, as in NonlinearElasticitySolver
        self.newton_iterations = 0
        self.newton_history = []
        self.newton_stats = []
        self.yielded_cells = []
        self.newton_iterations_per_step = []
        self.history = None

    # ------------------------------------------------------------------ settings
    def _refuse_unsupported(self):
        V = self.function_space
        if V.degree() != 1:
            raise SolverError('PlasticitySolver: CG{} displacements are not supported (vector CG1 only: a P2 strain varies over the '
                              'cell and needs a history per quadrature point)'.format(V.degree()))
        solid_steps.refuse_unsupported(self, 'PlasticitySolver', ' (no thermal strain in the model)', ('point_source', 'surface_source'))

    def plastic_parameters(self):
        """(mu, lambda, yield_stress, hardening_modulus): numbers for a homogeneous material, arrays [n_cells] where a value varies
        from cell to cell.  SolverError on a missing or non-positive yield stress, H < 0 or a Poisson ratio >= 0.5."""
        nu = self.material_field('poisson_ratio')
        if not np.all((np.asarray(nu) > -1.0) & (np.asarray(nu) < 0.5)):
            raise SolverError("PlasticitySolver: material 'poisson_ratio' must lie in (-1, 0.5): the bulk modulus of the return mapping "
                              "is infinite at 0.5")
        if not np.all(np.asarray(self.material_field('elastic_modulus')) > 0.0):
            raise SolverError("PlasticitySolver: material 'elastic_modulus' must be positive")
        if self.material.get('yield_stress') is None:
            raise SolverError("PlasticitySolver: material 'yield_stress' is required")
        sy = self.material_field('yield_stress')
        if not np.all(np.asarray(sy) > 0.0):
            raise SolverError("PlasticitySolver: material 'yield_stress' must be positive")
        H = self.material_field('hardening_modulus') if self.material.get('hardening_modulus') is not None else 0.0
        if not np.all(np.asarray(H) >= 0.0):
            raise SolverError("PlasticitySolver: material 'hardening_modulus' must be >= 0 (softening is not supported)")
        mu, lmbda = self.lame_parameters()
        return mu, lmbda, sy, H

    # ------------------------------------------------------------------ the form
    def generate_form(self, time_iter_, u, v, u_current, u_prev):
        self._refuse_unsupported()
        F = forms.PlasticForm(self.function_space)
        F.mu, F.lmbda, F.yield_stress, F.hardening = self.plastic_parameters()
        bcs, integrals = self.update_boundary_conditions(time_iter_, u, u_current, Measure("ds", subdomain_data=self.boundary_facets))
        F.tractions.extend(integrals)
        if self.body_source:
            self._set_body_force(F)
        return F, bcs

    def init_solver(self):
        LinearElasticitySolver.init_solver(self)
        self.yielded_cells = []
        self.newton_iterations_per_step = []
        if self.history is not None:
            self.history.reset()                  # solve() starts from the virgin state

    def _history(self):
        if self.history is None:
            from . import backend
            V = self.function_space
            dV = V.device()
            loc = V.localizer()                   # (known once the device side exists)
            self.history = backend.PlasticHistory(dV, None if loc is None else loc.part.cell_gids)
        return self.history

    def solve_form(self, F, u_, bcs):
        F.history = self._history()
        out = self.solve_nonlinear_problem(F, u_, bcs, None)
        self.yielded_cells.append(self.yielded_last_step)
        self.newton_iterations_per_step.append(self.newton_iterations)
        return out

    # ------------------------------------------------------------------ results
    def _committed(self):
        if self.history is None:
            raise SolverError('PlasticitySolver: no load step has been solved yet')
        return self.history.get()

    def cumulative_plastic_strain(self):
        """p per cell [n_cells] after the last converged step"""
        return self._committed()[1]

    def plastic_strain(self):
        """eps_p per cell [n_cells, 6] (xx, yy, zz, xy, xz, yz), plane strain [n_cells, 4] (xx, yy, zz, xy)"""
        return self._committed()[0]

    def stress(self):
        """The RETURNED stress per cell after the last converged step (same layout as plastic_strain) - not C : eps(u)."""
        return self._committed()[2]
