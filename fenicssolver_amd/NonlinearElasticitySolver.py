"""NonlinearElasticitySolver — finite-strain hyperelasticity on vector P1 (neo-Hookean, St Venant-Kirchhoff, Mooney-Rivlin, Yeoh), GPU back end.

Counterpart of FenicsSolver/NonlinearElasticitySolver.py: same class / constructor (:36-45), energy
psi = mu/2 (Ic - 3) - mu ln J + lambda/2 (ln J)^2 with F = I + grad u, C = F^T F, Ic = tr C, J = det F (:47-68), total
potential Pi = int psi dx - int B.u dx - the boundary loads of update_boundary_conditions with v = u (:70-88), solved by
Newton on dPi/du = 0 with the tangent d^2 Pi/du^2 (:90-98).  In 2-D (plane strain) the reference's Identity(2) with the
constant 3 is kept: it shifts the energy by -mu/2 per unit area and changes nothing else.

The tangent, the internal force and the energy are assembled on the device at every iterate (fs_assemble_hyperelastic); the
loads are dead loads (force, pressure and stress act on the reference configuration's normals and areas) and are assembled
once per load step.  The Newton loop (solid_steps.hyperelastic_newton) uses DOLFIN's defaults and stopping test; each step is
CG + AMG with the rigid-body near-null space in 3-D and Jacobi-CG in 2-D.  A trial step that inverts a cell is halved.

Energies beyond the reference's (``material['hyperelastic_model']``, one type per solve; none of them exists upstream):
  * ``'st_venant_kirchhoff'``: psi = lambda/2 (tr E)^2 + mu E:E, from elastic_modulus / poisson_ratio like the neo-Hookean one;
  * ``{'type': 'mooney_rivlin', 'c10', 'c01', 'bulk_modulus'}``: psi = c10 (Ibar1 - 3) + c01 (Ibar2 - 3) + kappa/2 (J - 1)^2;
  * ``{'type': 'yeoh', 'c10', 'c20', 'c30', 'bulk_modulus'}``: psi = sum_k ck0 (Ibar1 - 3)^k + kappa/2 (J - 1)^2.
  Every coefficient is a number or a per-region dict; without bulk_modulus, kappa = 2 mu0 (1 + nu) / (3 (1 - 2 nu)) from
  poisson_ratio and the small-strain shear modulus mu0 = 2 (c10 + c01) or 2 c10.  In 2-D these three are true plane strain (F33 = 1,
  3-D invariants, psi = 0 at rest).  cauchy_stress() and von_Mises() give sigma = P F^T / J for all four energies.

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

import numbers

import numpy as np

from .fem import Measure, is_constant_value
from .SolverBase import SolverError
from .LinearElasticitySolver import LinearElasticitySolver
from .stored_stress import StoredStressVonMises
from . import forms, solid_steps

_LAME_MODELS = ('neo_hookean', 'st_venant_kirchhoff')
_MODEL_KEYS = {'neo_hookean': (), 'st_venant_kirchhoff': (), 'mooney_rivlin': ('c10', 'c01', 'bulk_modulus'),
               'yeoh': ('c10', 'c20', 'c30', 'bulk_modulus')}
_REQUIRED = {'mooney_rivlin': ('c10', 'c01'), 'yeoh': ('c10',)}


class NonlinearElasticitySolver(StoredStressVonMises, LinearElasticitySolver):
    _constraint_sides = False          # 'contact' / 'sliding' sides stay with the static linear solver

    def __init__(self, case_settings):
        LinearElasticitySolver.__init__(self, case_settings)
        self.settings['mixed_variable'] = ('displacement', 'velocity', 'pressure')
        self.reference_load_sign = False          # the loads of Pi have their physical sign (varying pressure: NodalLoad)
        self.newton_iterations = 0
        self.newton_history = []

    def _refuse_unsupported(self):
        V = self.function_space
        if V.degree() != 1:
            raise SolverError('NonlinearElasticitySolver: CG{} displacements are not supported (vector CG1 only: the P2 integrand '
                              'is not polynomial)'.format(V.degree()))
        solid_steps.refuse_unsupported(self, 'NonlinearElasticitySolver',
                                       ' - the neo-Hookean energy has no thermal term (the reference ignores the setting)')

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
        F.model, F.params = self.hyperelastic_model()
        if F.model in _LAME_MODELS:
            F.mu, F.lmbda = self.lame_parameters()
        bcs, integrals = self.update_boundary_conditions(time_iter_, u, u_current, Measure("ds", subdomain_data=self.boundary_facets))
        F.tractions.extend(integrals)
        if self.body_source:
            self._set_body_force(F)
        return F, bcs

    def solve_form(self, F, u_, bcs):
        return self.solve_nonlinear_problem(F, u_, bcs, None)

    # ------------------------------------------------------------------ the energy
    def _model_leaves(self):
        """(type, {coefficient: value or per-region dict}) or, for a per-region model, [(region, type, {coefficient: number}, mask)]"""
        v = self.material.get('hyperelastic_model')
        if v is None:
            return 'neo_hookean', {}

        def leaf(x, where=''):
            if isinstance(x, str):
                return x, {}
            if isinstance(x, dict) and 'type' in x:
                return x['type'], {k: c for k, c in x.items() if k != 'type'}
            raise SolverError("material 'hyperelastic_model'{}: a model name or a dict with 'type' is expected".format(where))
        if isinstance(v, str) or (isinstance(v, dict) and 'type' in v):
            return leaf(v)
        if not isinstance(v, dict):
            raise SolverError("material 'hyperelastic_model': a string or a dict is expected, got {}".format(type(v).__name__))
        regions = self._regions_of(v, lambda x: isinstance(x, str) or (isinstance(x, dict) and 'type' in x))
        if regions is None:
            raise SolverError("material 'hyperelastic_model': the dict needs a 'type' (or is a per-region dict {'name': "
                              "{'subdomain_id': i, 'value': model}})")
        out = [(name,) + leaf(item, " of region '{}'".format(name)) + (mask,) for name, item, mask in regions]
        if len({t for _, t, _, _ in out}) > 1:
            raise SolverError("material 'hyperelastic_model': one model type per solve - the regions give {}".format(
                ', '.join("'{}'".format(t) for t in sorted({str(t) for _, t, _, _ in out}))))
        return out

    def _check_model(self, model, coef, where=''):
        what = "material 'hyperelastic_model'" + where
        if model not in _MODEL_KEYS:
            raise SolverError("{}: unknown hyperelastic model '{}' (one of {})".format(what, model, ', '.join(_MODEL_KEYS)))
        unknown = [k for k in coef if k not in _MODEL_KEYS[model]]
        if unknown:
            raise SolverError("{}: unknown key(s) {} for '{}' ({})".format(
                what, ', '.join(unknown), model, ', '.join(_MODEL_KEYS[model]) or 'it takes elastic_modulus / poisson_ratio'))
        if model in _REQUIRED:
            if not coef:
                raise SolverError("{}: '{}' needs its coefficients: {{'type': '{}', {}}}".format(
                    what, model, model, ', '.join("'{}': ..".format(k) for k in _MODEL_KEYS[model])))
            for k in _REQUIRED[model]:
                if k not in coef:
                    raise SolverError("{}: '{}' is missing for '{}'".format(what, k, model))

    def _coefficient_field(self, name, value):
        """a coefficient as a number or an array [n_cells]: a number, or a per-region dict of numbers"""
        what = "material 'hyperelastic_model': '{}'".format(name)
        if isinstance(value, numbers.Number) and not isinstance(value, bool):
            return float(value)
        regions = self._regions_of(value, lambda x: isinstance(x, numbers.Number) and not isinstance(x, bool)) if isinstance(value, dict) else None
        if regions is None or not all(isinstance(x, numbers.Number) and not isinstance(x, bool) for _, x, _ in regions):
            raise SolverError(what + ": a number or a per-region dict {'name': {'subdomain_id': i, 'value': number}} is expected")
        out = np.empty(self.mesh.num_cells())
        for _, x, mask in regions:
            out[mask] = float(x)
        return out

    def hyperelastic_model(self):
        """(model, params) of material['hyperelastic_model'].  params is None for 'neo_hookean' and 'st_venant_kirchhoff' (they
        read lame_parameters()); for 'mooney_rivlin' the row (c10, c01, kappa, 0) and for 'yeoh' (c10, c20, c30, kappa): a tuple of
        four numbers, or an array [n_cells, 4] in host cell order when a coefficient varies from region to region."""
        leaves = self._model_leaves()
        nc = self.mesh.num_cells()
        if isinstance(leaves, list):                       # the whole model per region: the coefficients become per-cell fields
            model = leaves[0][1]
            for name, t, coef, _ in leaves:
                self._check_model(t, coef, " of region '{}'".format(name))
            coef = {}
            for k in _MODEL_KEYS[model]:
                if any(k in c for _, _, c, _ in leaves):
                    if k == 'bulk_modulus' and not all(k in c for _, _, c, _ in leaves):
                        raise SolverError("material 'hyperelastic_model': 'bulk_modulus' is given in some regions only")
                    field = np.empty(nc)
                    for name, _, c, mask in leaves:
                        x = c.get(k, 0.0)                  # (c20, c30: 0 where a region leaves them out)
                        if not (isinstance(x, numbers.Number) and not isinstance(x, bool)):
                            raise SolverError("material 'hyperelastic_model' of region '{}': '{}' must be a number".format(name, k))
                        field[mask] = float(x)
                    coef[k] = field
        else:
            model, raw = leaves
            self._check_model(model, raw)
            coef = {k: self._coefficient_field(k, x) for k, x in raw.items()}
        if model in _LAME_MODELS:
            return model, None
        c10 = coef['c10']
        second = coef.get('c01') if model == 'mooney_rivlin' else coef.get('c20', 0.0)
        c30 = coef.get('c30', 0.0)
        mu0 = 2.0 * (c10 + second) if model == 'mooney_rivlin' else 2.0 * c10
        if 'bulk_modulus' in coef:
            kappa = coef['bulk_modulus']
        else:
            if self.material.get('poisson_ratio') is None:
                raise SolverError("material 'hyperelastic_model': '{}' needs 'bulk_modulus', or material['poisson_ratio'] to derive it "
                                  "from (kappa = 2 mu0 (1 + nu) / (3 (1 - 2 nu)))".format(model))
            nu = self.material_field('poisson_ratio')
            if not np.all((np.asarray(nu) > -1.0) & (np.asarray(nu) < 0.5)):
                raise SolverError("material 'poisson_ratio' must lie in (-1, 0.5) to derive the bulk modulus of '{}' from it".format(model))
            kappa = 2.0 * mu0 * (1.0 + nu) / (3.0 * (1.0 - 2.0 * nu))
        cols = (c10, second, kappa, 0.0) if model == 'mooney_rivlin' else (c10, second, c30, kappa)
        rows = np.stack([np.broadcast_to(np.asarray(x, dtype=np.float64), (nc,)) for x in cols], axis=1)
        names = forms.HYPER_PARAMETER_NAMES[model]
        kap = rows[:, 2] if model == 'mooney_rivlin' else rows[:, 3]
        checks = [('every coefficient must be finite (a value is not finite)', np.isfinite(rows).all(axis=1))]
        if model == 'mooney_rivlin':
            checks += [('c10 >= 0 is required', rows[:, 0] >= 0.0), ('c01 >= 0 is required', rows[:, 1] >= 0.0),
                       ('c10 + c01 > 0 is required', rows[:, 0] + rows[:, 1] > 0.0)]
        else:
            checks += [('c10 > 0 is required (c20 and c30 may have either sign)', rows[:, 0] > 0.0)]
        checks += [('a bulk modulus > 0 is required', kap > 0.0)]
        for msg, ok in checks:
            if not ok.all():
                bad = int(np.argmin(ok))
                raise SolverError("material 'hyperelastic_model' ('{}', {}): {}{}".format(
                    model, ', '.join('{} = {:g}'.format(n, rows[bad, k]) for n, k in zip(names, range(4) if model == 'yeoh' else range(3))),
                    msg, '' if all(np.ndim(x) == 0 for x in cols) else ' - cell {}'.format(bad)))
        if all(np.ndim(x) == 0 for x in cols):
            return model, tuple(float(x) for x in rows[0])
        return model, rows

    def small_strain_moduli(self):
        """(mu0, lambda0) per cell [n_cells] of the linearisation at rest: the Lame parameters for 'neo_hookean' and
        'st_venant_kirchhoff'; mu0 = 2 (c10 + c01) for 'mooney_rivlin', 2 c10 for 'yeoh', and lambda0 = kappa - 2 mu0 / 3."""
        model, params = self.hyperelastic_model()
        nc = self.mesh.num_cells()
        if params is None:
            mu, lmbda = self.lame_parameters()
            return (np.broadcast_to(np.asarray(mu, dtype=np.float64), (nc,)).copy(),
                    np.broadcast_to(np.asarray(lmbda, dtype=np.float64), (nc,)).copy())
        p = np.broadcast_to(np.asarray(params, dtype=np.float64), (nc, 4))
        mu0 = 2.0 * (p[:, 0] + p[:, 1]) if model == 'mooney_rivlin' else 2.0 * p[:, 0]
        kappa = p[:, 2] if model == 'mooney_rivlin' else p[:, 3]
        return mu0, kappa - 2.0 * mu0 / 3.0

    # ------------------------------------------------------------------ results
    def cauchy_stress(self, u=None):
        """sigma = P F^T / J per cell of the displacement u (default: the solution) for the case's energy, on the device
        (fs_hyper_stress): [n_cells, 6] (xx, yy, zz, xy, xz, yz), in plane strain [n_cells, 4] (xx, yy, zz, xy) with sigma_zz kept;
        tensor components, cells in the mesh's numbering.  A state with an inverted cell (J <= 0) is refused."""
        from . import backend
        self._refuse_unsupported()
        if u is None:
            u = getattr(self, 'w_current', None)
            if u is None:
                raise SolverError('cauchy_stress: no displacement given and nothing has been solved yet')
        F = forms.HyperelasticForm(self.function_space)
        F.model, F.params = self.hyperelastic_model()
        if F.model in _LAME_MODELS:
            F.mu, F.lmbda = self.lame_parameters()
        model, lame, params = F.model_spec()
        V = self.function_space
        dV, loc = V.device(), V.localizer()
        lame, params = solid_steps.localized(lame, loc), solid_steps.localized(params, loc)
        ud = backend.DeviceVector(dV.n_local, solid_steps.to_device_dofs(dV, loc, u.vector()._values()))
        try:
            sig = backend.hyperelastic_stress(dV, ud, lame, model=model, params=params)
        except backend.BackendError as e:
            if 'inverted' in str(e):
                raise SolverError('cauchy_stress: the displacement inverts cells - {}'.format(e)) from e
            raise
        if loc is not None:
            out = np.empty_like(sig)
            out[np.asarray(loc.part.cell_gids, dtype=np.int64)] = sig
            sig = out
        return sig

    def stress(self):
        """the Cauchy stress of the solution (what von_Mises_cells() reads)"""
        return self.cauchy_stress()

    def von_Mises(self, u=None):
        """The consistent L2 projection onto CG1 of sqrt(3/2 dev sigma : dev sigma) of the CAUCHY stress of u (default: the
        solution), by the projection the other solid classes use (the linear class's von_Mises means nothing at finite strain)."""
        return self._project_cells(self.von_Mises_cells(self.cauchy_stress(u)))
