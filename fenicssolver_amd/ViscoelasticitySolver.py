"""ViscoelasticitySolver — small-strain linear viscoelasticity (generalized Maxwell solid, Prony series) on vector P1, GPU back end.

The reference lists "viscoelastic" among its solvers under development (Readme.md) and has no such class; this one fills the gap
with the textbook model, so there is no reference counterpart to diff against; the independent check is the numpy
restatement tests/viscoelastic_reference.py.

Model: eps = sym grad u, one integration point per cell (CG1: constant strain), e = dev eps.  The bulk response is elastic, the
deviatoric response relaxes:
    sigma(t) = K tr(eps) I + 2 G0 [ g_inf e + sum_k g_k h_k ],   h_k(t) = int_0^t exp(-(t - s)/tau_k) de/ds ds,   g_inf = 1 - sum_k g_k.
A step of length dt uses the recursion that is exact for a strain history linear within the step (x_k = dt/tau_k, a_k = exp(-x_k),
b_k = -expm1(-x_k)/x_k, h_k <- a_k h_k + b_k (e_new - e_old)), so every step is ONE linear solve with the elasticity operator of
the effective moduli mu_eff = G0 (g_inf + sum g_k b_k), lambda_eff = K - 2/3 mu_eff and a history load on the right-hand side
(solid_steps.viscoelastic_step, fs_assemble_viscoelastic).  The history per cell is e, h_k and the stress; it starts from zero at the
starting time, and the first step ramps from the zero state to that step's loads: an "instant" load is a very short first step
through ``time_series``.  The effective operator and its AMG hierarchy are built once per step length (``operator_assemblies``,
``amg_setups``); each solve is CG + AMG with the rigid-body near-null space in 3-D and Jacobi-CG in 2-D (plane strain).

Settings: material ``elastic_modulus`` and ``poisson_ratio`` are the INSTANTANEOUS moduli (G0, lambda0, K = lambda0 + 2/3 G0);
``prony_series`` is a list of {'relative_modulus': g_k, 'relaxation_time': tau_k} with g_k > 0, tau_k > 0, sum g_k < 1, at most 8
terms; each value a number or a per-region dict like ``elastic_modulus`` (every region then has the same number of terms).  A
missing or empty list is an elastic material.  ``transient: False`` solves the long-term equilibrium (mu = G0 g_inf), one solve
without history.  Boundary values and loads may be per-step sequences or callables of time; loads are dead loads with their
physical sign.  P2 spaces, several ranks, periodic spaces, ``temperature_distribution``, ``point_source``, ``surface_source``, a bad
``prony_series`` and a Poisson ratio outside (-1, 0.5) raise SolverError before any device call.

Results: ``solve()`` returns the displacement; ``stress()``, ``deviatoric_strain()`` and ``viscous_strains()`` ([n_cells, n_terms,
n_comp]) return per-cell arrays of the last committed step in the caller's cell numbering (tensors as (xx, yy, zz, xy, xz, yz) in
3-D and (xx, yy, zz, xy) in plane strain); ``von_Mises()`` projects the von Mises value of the STORED stress onto CG1;
``effective_lame(dt)`` and ``relaxation_modulus(t)`` are host helpers; ``step_stats`` holds the device times of every step.
"""
from __future__ import annotations

import numbers

import numpy as np

from .fem import Measure
from .SolverBase import SolverError
from .LinearElasticitySolver import LinearElasticitySolver
from .stored_stress import StoredStressVonMises
from . import case, forms, solid_steps

MAX_TERMS = 8           # FS_VISCO_MAX_TERMS of the library


class ViscoelasticitySolver(StoredStressVonMises, LinearElasticitySolver):
    _constraint_sides = False          # 'contact' / 'sliding' sides stay with the static linear solver

    def __init__(self, case_settings):
        LinearElasticitySolver.__init__(self, case_settings)
        self.reference_load_sign = False          # dead loads with their physical sign, as in PlasticitySolver
        self.operator_assemblies = 0
        self.amg_setups = 0
        self.step_stats = []
        self.history = None
        self._material_cache = None

    # ------------------------------------------------------------------ settings
    def _refuse_unsupported(self):
        V = self.function_space
        if V.degree() != 1:
            raise SolverError('ViscoelasticitySolver: CG{} displacements are not supported (vector CG1 only: a P2 strain varies over '
                              'the cell and needs a history per quadrature point)'.format(V.degree()))
        solid_steps.refuse_unsupported(self, 'ViscoelasticitySolver', ' (no thermal strain in the model)', ('point_source', 'surface_source'))

    def _series_value(self, v, what):
        if isinstance(v, numbers.Number) and not isinstance(v, bool):
            return float(v)
        if isinstance(v, dict):
            if getattr(self, 'subdomains', None) is None:
                raise SolverError("ViscoelasticitySolver: material 'prony_series': {} is given per region, but the case has no "
                                  "subdomains".format(what))
            return case.cellwise_from_regions(v, self.subdomains)
        raise SolverError("ViscoelasticitySolver: material 'prony_series': {} must be a number or a per-region dict, got {}".format(
            what, type(v).__name__))

    def prony_terms(self):
        """[(g_k, tau_k), ...]: numbers, or arrays [n_cells] where a value is given per region.  SolverError on a bad series."""
        series = self.material.get('prony_series')
        if series is None:
            return []
        if not isinstance(series, (list, tuple)):
            raise SolverError("ViscoelasticitySolver: material 'prony_series' must be a list of {'relative_modulus': g, "
                              "'relaxation_time': tau}")
        if len(series) > MAX_TERMS:
            raise SolverError("ViscoelasticitySolver: material 'prony_series' has {} terms, at most {} are supported".format(
                len(series), MAX_TERMS))
        terms = []
        gsum = 0.0
        for k, item in enumerate(series):
            if not isinstance(item, dict) or 'relative_modulus' not in item or 'relaxation_time' not in item:
                raise SolverError("ViscoelasticitySolver: material 'prony_series': term {} must be a dict with 'relative_modulus' and "
                                  "'relaxation_time'".format(k))
            g = self._series_value(item['relative_modulus'], "'relative_modulus' of term {}".format(k))
            tau = self._series_value(item['relaxation_time'], "'relaxation_time' of term {}".format(k))
            if not (np.all(np.asarray(g) > 0.0) and np.all(np.isfinite(g))):
                raise SolverError("ViscoelasticitySolver: material 'prony_series': 'relative_modulus' of term {} must be positive".format(k))
            if not (np.all(np.asarray(tau) > 0.0) and np.all(np.isfinite(tau))):
                raise SolverError("ViscoelasticitySolver: material 'prony_series': 'relaxation_time' of term {} must be positive".format(k))
            gsum = gsum + np.asarray(g)
            terms.append((g, tau))
        if not np.all(gsum < 1.0):
            raise SolverError("ViscoelasticitySolver: material 'prony_series': the relative moduli must sum to less than 1 (the "
                              "long-term fraction g_inf = 1 - sum g_k must be positive), got {}".format(float(np.max(gsum))))
        return terms

    def viscoelastic_parameters(self):
        """(G0, lambda0, terms): the instantaneous Lame parameters and the Prony series, numbers or arrays [n_cells]."""
        nu = self.material_field('poisson_ratio')
        if not np.all((np.asarray(nu) > -1.0) & (np.asarray(nu) < 0.5)):
            raise SolverError("ViscoelasticitySolver: material 'poisson_ratio' must lie in (-1, 0.5): the bulk modulus of the model is "
                              "infinite at 0.5")
        if not np.all(np.asarray(self.material_field('elastic_modulus')) > 0.0):
            raise SolverError("ViscoelasticitySolver: material 'elastic_modulus' must be positive")
        terms = self.prony_terms()
        mu, lmbda = self.lame_parameters()
        return mu, lmbda, terms

    def _form_of_material(self):
        """A form that carries the material.  The regions are resolved once per solve() (init_solver drops the cache); the token tells
        the step routine that the material of two forms is the same object, so that it keeps what it derived from it."""
        cached = getattr(self, '_material_cache', None)
        if cached is None:
            cached = self._material_cache = (self.viscoelastic_parameters(), object())
        F = forms.ViscoelasticForm(self.function_space)
        (F.mu, F.lmbda, F.terms), F.material_token = cached
        return F

    def effective_lame(self, dt=None):
        """(mu_eff, lambda_eff) of the step operator for the step length dt; None: the long-term moduli (G0 g_inf, K - 2/3 G0 g_inf)."""
        return self._form_of_material().effective_lame(dt)

    def relaxation_modulus(self, t):
        """G(t) = G0 (g_inf + sum_k g_k exp(-t / tau_k)): the shear stress per unit of 2 x shear strain a step strain at t = 0 leaves
        at time t.  A number, or an array [n_cells] for a per-cell material."""
        F = self._form_of_material()
        f = F.long_term_fraction()
        for g, tau in F.terms:
            f = f + np.asarray(g, dtype=np.float64) * np.exp(-float(t) / np.asarray(tau, dtype=np.float64))
        G = np.asarray(F.mu, dtype=np.float64) * f
        return float(G) if np.ndim(G) == 0 else G

    # ------------------------------------------------------------------ the form
    def generate_form(self, time_iter_, u, v, u_current, u_prev):
        self._refuse_unsupported()
        F = self._form_of_material()
        F.steady = not self.transient_settings['transient']
        if not F.steady:
            F.dt = float(self.get_time_step(time_iter_))
            if not (F.dt > 0.0 and np.isfinite(F.dt)):
                raise SolverError('ViscoelasticitySolver: the time step of step {} is {}: it must be positive'.format(time_iter_, F.dt))
        bcs, integrals = self.update_boundary_conditions(time_iter_, u, u_current, Measure("ds", subdomain_data=self.boundary_facets))
        F.tractions.extend(integrals)
        if self.body_source:
            self._set_body_force(F)
        return F, bcs

    def init_solver(self):
        LinearElasticitySolver.init_solver(self)
        self.operator_assemblies = 0
        self.amg_setups = 0
        self.step_stats = []
        self._visco_ctx = None                    # the kept operator and the resolved material belong to one solve()
        self._material_cache = None
        if self.history is not None:
            self.history.reset()                  # solve() starts from the zero state

    def _history(self, n_terms):
        if self.history is not None and self.history.n_terms != n_terms:
            self.history.close()
            self.history = None
        if self.history is None:
            from . import backend
            V = self.function_space
            dV = V.device()
            loc = V.localizer()                   # (known once the device side exists)
            self.history = backend.ViscoHistory(dV, n_terms, None if loc is None else loc.part.cell_gids)
        return self.history

    def solve_form(self, F, u_, bcs):
        F.history = self._history(0 if F.steady else len(F.terms))
        return solid_steps.viscoelastic_step(self, F, u_, bcs)

    # ------------------------------------------------------------------ results
    def _committed(self):
        if self.history is None:
            raise SolverError('ViscoelasticitySolver: no step has been solved yet')
        return self.history.get()

    def deviatoric_strain(self):
        """e = dev eps per cell [n_cells, 6] (xx, yy, zz, xy, xz, yz), plane strain [n_cells, 4] (xx, yy, zz, xy)"""
        return self._committed()[0]

    def viscous_strains(self):
        """h_k per cell [n_cells, n_terms, n_comp] after the last committed step (same tensor layout)"""
        return self._committed()[1]

    def stress(self):
        """The stored stress per cell after the last committed step (same layout as deviatoric_strain) - not C : eps(u)."""
        return self._committed()[2]
