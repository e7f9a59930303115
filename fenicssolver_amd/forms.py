"""Operator specifications: what ``generate_form`` returns in place of a UFL form.

The reference builds a UFL expression tree and lets FFC turn it into
tabulate_tensor code (ScalarTransportSolver.py:228-359,
LinearElasticitySolver.py:206-245).  Here the solver classes *recognise* which
integrals the settings ask for and record them, with their coefficients, in one
of the small classes below; ``SolverBase.solve_linear_problem`` / ``solve_amg``
hand them to the HIP kernels.  The classes are plain data — printable and
comparable in tests — and contain no arithmetic.
"""
from __future__ import annotations

import numpy as np


class VolumeCoefficient:
    """kind: 'const' (value float), 'cell' (value array[n_cells]), 'tensor' (value 3x3),
    'nodal' (value array[n_vertices], linear forms only)."""

    def __init__(self, kind, value):
        self.kind = kind
        self.value = value

    def spec(self, scale=1.0):
        """Argument for fenicssolver_amd.backend (None | number | (kind, array))."""
        if self.kind == "const":
            return float(self.value) * scale
        return (self.kind, np.asarray(self.value, dtype=np.float64) * scale)

    def describe(self):
        if self.kind == "const":
            return ("const", float(self.value))
        a = np.asarray(self.value, dtype=np.float64)
        return (self.kind, a.shape, float(a.min()), float(a.max()))

    def __repr__(self):
        return "VolumeCoefficient%r" % (self.describe(),)


class FacetLoad:
    """int g * q ds(marker_id) added to the load vector; g scalar or [ncomp]."""

    def __init__(self, marker_id, g, origin=""):
        self.marker_id = int(marker_id)
        self.g = g
        self.origin = origin

    def __repr__(self):
        return "FacetLoad(ds(%d), g=%r, %s)" % (self.marker_id, self.g, self.origin)


class NodalLoad:
    """b[dofs] += values: load contributions worked out per node on the host (boundary terms with a varying magnitude,
    integrated exactly for its P1 interpolant)."""

    def __init__(self, dofs, values, origin=""):
        self.dofs = np.asarray(dofs, dtype=np.int64).ravel()
        self.values = np.asarray(values, dtype=np.float64).ravel()
        self.origin = origin

    def __repr__(self):
        return "NodalLoad(%d entries, %s)" % (len(self.dofs), self.origin)


class FacetRobin:
    """htc*(Ta - T)*q*ds(i): +h int T q ds on the matrix, +h*Ta int q ds on the load."""

    def __init__(self, marker_id, h, ambient):
        self.marker_id = int(marker_id)
        self.h = float(h)
        self.ambient = float(ambient) if np.ndim(ambient) == 0 else np.asarray(ambient, dtype=np.float64)   # [nf, d]: vertex values

    def __repr__(self):
        return "FacetRobin(ds(%d), h=%g, Ta=%s)" % (self.marker_id, self.h, _plain(self.ambient))


class ScalarForm:
    """F = (1/dt) c (T-T_prev) q dx + theta a_k(T,q) + (1-theta) a_k(T_prev,q) - loads
    with a_k = int k grad T . grad q dx  (ScalarTransportSolver.py:284-303)."""

    def __init__(self, space):
        self.space = space
        self.conductivity = None      # VolumeCoefficient
        self.capacity = None          # VolumeCoefficient (transient only)
        self.transient = False
        self.dt = None
        self.theta = 1.0
        self.T_prev = None            # Function
        self.sources = []             # [VolumeCoefficient]  int S q dx
        self.facet_loads = []         # [FacetLoad]
        self.robin = []               # [FacetRobin]
        self.point_sources = []       # [fem.PointSource]: b[dofs] += weights, before the Dirichlet rows
        self.supg_pe = 0.0            # > 0: every test function is q + tau (v . grad q) ("SPUG", :259-270)
        self.ip_coefficient = 0.0     # alpha * capacity of + alpha avg(h)^2 jump(grad T,n) jump(grad q,n) capacity dS ("IP", :312-315)
        self.advection = None         # (velocity: 3-vector or array[n_cells,3], scale = capacity) -> non-symmetric
        self.symmetric = True
        # nonlinear terms (Newton): radiation  - m (Ta^4 - T^4) q ds over the whole boundary, m = emissivity*sigma
        # (ScalarTransportSolver.py:338-350, 361-376) and material callables re-evaluated every iteration
        self.radiation = None         # (m, T_ambient)
        self.conductivity_fn = None   # callable(T array) -> k
        self.capacity_fn = None       # callable(T array) -> volumetric capacity (transient term; re-evaluated per Newton iterate)
        self.nonlinear = False

    def describe(self):
        """Canonical, order-stable description used by the golden-term tests."""
        return {
            "type": "scalar",
            "conductivity": self.conductivity.describe() if self.conductivity else None,
            "capacity": self.capacity.describe() if self.capacity else None,
            "transient": self.transient, "dt": self.dt, "theta": self.theta,
            "supg_pe": self.supg_pe,
            "ip_coefficient": self.ip_coefficient,
            "sources": [s.describe() for s in self.sources],
            "facet_loads": [(f.marker_id, _plain(f.g), f.origin) for f in self.facet_loads],
            "robin": [(r.marker_id, r.h, _plain(r.ambient)) for r in self.robin],
            "advection": None if self.advection is None else (_plain(self.advection[0]), float(self.advection[1])),
            "radiation": self.radiation, "nonlinear": self.nonlinear,
        }


class ElasticityForm:
    """F = int sigma(u):grad v dx  +/- loads  (LinearElasticitySolver.py:206-245)."""

    def __init__(self, space):
        self.space = space
        self.mu = None                # numbers (homogeneous) or arrays [n_cells] (per-cell material, host cell order)
        self.lmbda = None
        self.body_force = None        # (fx, fy, fz) or None
        self.body_force_nodal = None  # [n_nodes, dim]: a body force FIELD by its nodal values (consistent-mass load)
        self.tractions = []           # [FacetLoad] with vector g
        self.thermal = None           # (coefficient E*alpha/(1-2nu): number or array [n_cells], T nodal array or float, T_ref)
        self.load_sign = -1.0         # reference adds the load terms to F => rhs = -loads (Appendix B-Q3)
        self.inertia = None           # (density: number or ('cell', array), acceleration dof array): rhs += rho M a (:216-220)
        self.anisotropic = None       # AnisotropicElasticity: the operator is int eps(v) : C : eps(u) dx, mu / lmbda stay None

    def cellwise(self):
        return np.ndim(self.mu) > 0 or np.ndim(self.lmbda) > 0

    def lame_spec(self):
        """Lame argument of backend.DeviceMatrix.assemble: (mu, lambda), or ('cell', [n_cells, 2]) in host cell order."""
        if not self.cellwise():
            return (self.mu, self.lmbda)
        n = max(np.size(self.mu), np.size(self.lmbda))
        return ("cell", np.stack([np.broadcast_to(np.asarray(self.mu, dtype=np.float64), (n,)),
                                  np.broadcast_to(np.asarray(self.lmbda, dtype=np.float64), (n,))], axis=1))

    def describe(self):
        d = {
            "type": "elasticity", "mu": _material(self.mu), "lambda": _material(self.lmbda),
            "body_force": None if self.body_force is None else tuple(float(x) for x in self.body_force),
            "tractions": [(t.marker_id, _plain(t.g), t.origin) if isinstance(t, FacetLoad) else ("nodal", len(t.dofs), t.origin)
                          for t in self.tractions],
            "thermal": None if self.thermal is None else (_material(self.thermal[0]), _plain(self.thermal[1]), self.thermal[2]),
            "load_sign": self.load_sign,
        }
        if self.anisotropic is not None:      # (only then: the golden-form tests compare the dict of the isotropic forms)
            d["anisotropic"] = self.anisotropic.describe()
        return d


class AnisotropicElasticity:
    """The anisotropic material of an ElasticityForm, host cell order: ``table`` [n, 6, 6] in the library's tensor order (xx, yy, zz,
    xy, xz, yz; engineering shears), ``index`` [n_cells] table rows (None: one material), ``frames`` [n_cells, 3, 3] rotations with
    the material axes as columns (None: global axes), ``thermal``: None or (eps [n_cells, 6 or 4] = R alpha R^T per unit temperature
    in the tensor storage, T nodal array or float, T_ref)."""

    def __init__(self, table, index=None, frames=None, thermal=None):
        self.table = np.ascontiguousarray(table, dtype=np.float64)
        self.index = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
        self.frames = None if frames is None else np.ascontiguousarray(frames, dtype=np.float64)
        self.thermal = thermal

    def material(self, loc=None):
        """The argument of backend.DeviceMatrix.assemble_anisotropic, in device cell order: ``loc`` is the space's localizer (None:
        the device numbers the cells as the host does; a mesh uploaded in locality order has one that permutes them).  The table
        holds the distinct materials (index None: one of them everywhere) and needs no mapping."""
        cells = (lambda a: a) if loc is None else loc.cells
        return (self.table, None if self.index is None else cells(self.index), None if self.frames is None else cells(self.frames))

    def eigenstrain(self, cells, loc=None):
        """eps* [n_cells, 6 or 4] of the thermal load in device cell order; ``cells``: the host mesh's cell-vertex array (a nodal
        temperature enters by its mean at the cell's vertices)."""
        eps1, T, T_ref = self.thermal
        dT = float(T) - T_ref if np.ndim(T) == 0 else np.asarray(T, dtype=np.float64)[np.asarray(cells, dtype=np.int64)].mean(axis=1) - T_ref
        eps = eps1 * np.reshape(dT, (-1, 1))
        return eps if loc is None else loc.cells(eps)

    def digest(self):
        import zlib
        return tuple(None if a is None else (a.shape, zlib.crc32(a.tobytes())) for a in (self.table, self.index, self.frames))

    def describe(self):
        return {"materials": int(self.table.shape[0]), "table": _plain(self.table), "per_cell_index": self.index is not None,
                "frames": self.frames is not None,
                "thermal": None if self.thermal is None else (_plain(self.thermal[0]), _plain(self.thermal[1]), self.thermal[2])}


HYPER_PARAMETER_NAMES = {"mooney_rivlin": ("c10", "c01", "bulk_modulus"), "yeoh": ("c10", "c20", "c30", "bulk_modulus")}


class HyperelasticForm:
    """Pi = int psi(F) dx - int B.u dx - loads.u ds; the Newton iteration solves dPi/du = 0 (solid_steps.hyperelastic_newton).
    ``model``: 'neo_hookean' (the compressible neo-Hookean energy of NonlinearElasticitySolver.py:41-98) or 'st_venant_kirchhoff',
    both with the Lame parameters mu / lmbda; 'mooney_rivlin' or 'yeoh' with the parameter table ``params``.  Only the first has a
    counterpart upstream.  The loads are dead loads with their PHYSICAL sign (the reference subtracts them from Pi; no
    reversed-sign quirk here)."""

    def __init__(self, space):
        self.space = space
        self.model = "neo_hookean"
        self.mu = None                # numbers (homogeneous) or arrays [n_cells] (per-cell material, host cell order)
        self.lmbda = None
        self.params = None            # mooney_rivlin (c10, c01, kappa, 0) / yeoh (c10, c20, c30, kappa): one row of 4 numbers,
                                      # or an array [n_cells, 4] of rows in host cell order
        self.body_force = None        # (fx, fy[, fz]) or None
        self.body_force_nodal = None  # [n_nodes, dim]: a body force FIELD by its nodal values (consistent-mass load)
        self.tractions = []           # [FacetLoad] with vector g, or [NodalLoad] (surface_source, varying pressure)

    lame_spec = ElasticityForm.lame_spec

    def cellwise(self):
        if self.model in HYPER_PARAMETER_NAMES:
            return np.ndim(self.params) > 1
        return ElasticityForm.cellwise(self)

    def model_spec(self):
        """(model, lame, params) as backend.assemble_hyperelastic takes them, per-cell arrays in HOST cell order: lame = (mu, lambda)
        or ('cell', [n_cells, 2]) and params None for the two Lame models; lame None and params a row of 4 numbers or
        ('cell', [n_cells, 4]) for the others."""
        if self.model not in HYPER_PARAMETER_NAMES:
            return (self.model, self.lame_spec(), None)
        if self.cellwise():
            return (self.model, None, ("cell", np.ascontiguousarray(self.params, dtype=np.float64)))
        return (self.model, None, tuple(float(x) for x in self.params))

    def describe(self):
        d = {
            "type": "hyperelasticity", "model": self.model, "mu": _material(self.mu), "lambda": _material(self.lmbda),
            "body_force": None if self.body_force is None else tuple(float(x) for x in self.body_force),
            "tractions": [(t.marker_id, _plain(t.g), t.origin) if isinstance(t, FacetLoad) else ("nodal", len(t.dofs), t.origin)
                          for t in self.tractions],
        }
        if self.model in HYPER_PARAMETER_NAMES:      # (only then: the neo-Hookean description stays as it was)
            names = HYPER_PARAMETER_NAMES[self.model]
            p = np.asarray(self.params, dtype=np.float64)
            cols = (0, 1, 2) if self.model == "mooney_rivlin" else (0, 1, 2, 3)
            d["parameters"] = {n: _material(p[..., k] if p.ndim > 1 else float(p[k])) for n, k in zip(names, cols)}
        return d


class PlasticForm:
    """r(u) = int sigma(eps(u); history) : grad v dx - int B.v dx - loads.v ds with sigma the radial return of small-strain J2
    plasticity with linear isotropic hardening (PlasticitySolver); solid_steps.plastic_newton solves r = 0 per load step.  Dead
    loads with their physical sign, as in HyperelasticForm.  ``history``: the backend.PlasticHistory the solver keeps across steps."""

    def __init__(self, space):
        self.space = space
        self.mu = None                # numbers (homogeneous) or arrays [n_cells] (per-cell material, host cell order)
        self.lmbda = None
        self.yield_stress = None
        self.hardening = 0.0
        self.body_force = None
        self.body_force_nodal = None
        self.tractions = []
        self.history = None

    def cellwise(self):
        return any(np.ndim(v) > 0 for v in (self.mu, self.lmbda, self.yield_stress, self.hardening))

    def material_spec(self):
        """Material argument of backend.assemble_plasticity: four numbers, or ('cell', [n_cells, 4]) in host cell order."""
        vals = (self.mu, self.lmbda, self.yield_stress, self.hardening)
        if not self.cellwise():
            return tuple(float(v) for v in vals)
        n = max(np.size(v) for v in vals)
        return ("cell", np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in vals], axis=1))

    def describe(self):
        return {
            "type": "plasticity", "mu": _material(self.mu), "lambda": _material(self.lmbda),
            "yield_stress": _material(self.yield_stress), "hardening": _material(self.hardening),
            "body_force": None if self.body_force is None else tuple(float(x) for x in self.body_force),
            "tractions": [(t.marker_id, _plain(t.g), t.origin) if isinstance(t, FacetLoad) else ("nodal", len(t.dofs), t.origin)
                          for t in self.tractions],
        }


PRONY_SERIES_X = 1e-5       # below this dt / tau the series of b_k replaces -expm1(-x) / x (fs_viscoelasticity.hip, FS_VISCO_SERIES_X)


def prony_step_coefficients(x):
    """(a, b) of the one-step recursion h^{n+1} = a h^n + b (e^{n+1} - e^n) for x = dt / tau: a = exp(-x), b = -expm1(-x) / x -
    below PRONY_SERIES_X its series 1 - x/2 + x^2/6 - x^3/24 (dropped term x^4/120 < 1e-22), which covers x -> 0."""
    x = np.asarray(x, dtype=np.float64)
    small = x < PRONY_SERIES_X
    xs = np.where(small, 1.0, x)
    b = np.where(small, 1.0 - x * (0.5 - x * ((1.0 / 6.0) - x * (1.0 / 24.0))), -np.expm1(-xs) / xs)
    return np.exp(-x), b


class ViscoelasticForm:
    """One step of small-strain linear viscoelasticity (generalized Maxwell solid, ViscoelasticitySolver):
    K(mu_eff, lambda_eff) u = int B.v dx + loads.v ds - int B^T s_hist dx, solved by solid_steps.viscoelastic_step.  ``mu``, ``lmbda``:
    the INSTANTANEOUS Lame parameters, ``terms``: the Prony series [(g_k, tau_k), ...]; each value a number or an array [n_cells]
    in host cell order.  ``dt``: the step length; ``steady``: the long-term equilibrium (mu = G0 g_inf, no history).  Dead loads with
    their physical sign, as in PlasticForm.  ``history``: the backend.ViscoHistory the solver keeps across steps."""

    def __init__(self, space):
        self.space = space
        self.mu = None
        self.lmbda = None
        self.terms = []
        self.dt = None
        self.steady = False
        self.body_force = None
        self.body_force_nodal = None
        self.tractions = []
        self.history = None
        self.material_token = None     # forms with the same (not None) token carry the same material

    def cellwise(self):
        return any(np.ndim(v) > 0 for v in [self.mu, self.lmbda] + [x for gt in self.terms for x in gt])

    def material_spec(self):
        """Material argument of backend.assemble_viscoelastic: (mu, lambda, terms), or ('cell', [n_cells, 2 + 2 n_terms]) in host
        cell order."""
        vals = [self.mu, self.lmbda] + [x for gt in self.terms for x in gt]
        if not self.cellwise():
            return (float(self.mu), float(self.lmbda), [(float(g), float(tau)) for g, tau in self.terms])
        n = max(np.size(v) for v in vals)
        return ("cell", np.stack([np.broadcast_to(np.asarray(v, dtype=np.float64), (n,)) for v in vals], axis=1))

    def long_term_fraction(self):
        """g_inf = 1 - sum_k g_k (summed in the order of the series)"""
        gsum = 0.0
        for g, _ in self.terms:
            gsum = gsum + np.asarray(g, dtype=np.float64)
        return 1.0 - gsum

    def effective_lame(self, dt=None):
        """(mu_eff, lambda_eff) of the step operator: mu_eff = G0 (g_inf + sum_k g_k b_k(dt / tau_k)), lambda_eff = K - 2/3 mu_eff
        with the bulk modulus K = lambda0 + 2/3 G0.  dt None: the long-term moduli (b_k = 0)."""
        mu0, lm0 = np.asarray(self.mu, dtype=np.float64), np.asarray(self.lmbda, dtype=np.float64)
        f = self.long_term_fraction()
        if dt is not None:
            for g, tau in self.terms:
                f = f + np.asarray(g, dtype=np.float64) * prony_step_coefficients(float(dt) / np.asarray(tau, dtype=np.float64))[1]
        mu = mu0 * f
        lm = (lm0 + (2.0 / 3.0) * mu0) - (2.0 / 3.0) * mu
        return (float(mu), float(lm)) if np.ndim(mu) == 0 and np.ndim(lm) == 0 else (mu, lm)

    def describe(self):
        return {
            "type": "viscoelasticity", "mu": _material(self.mu), "lambda": _material(self.lmbda),
            "prony_series": [(_material(g), _material(tau)) for g, tau in self.terms], "dt": self.dt, "steady": self.steady,
            "body_force": None if self.body_force is None else tuple(float(x) for x in self.body_force),
            "tractions": [(t.marker_id, _plain(t.g), t.origin) if isinstance(t, FacetLoad) else ("nodal", len(t.dofs), t.origin)
                          for t in self.tractions],
        }


def _material(v):
    """A material value: the number itself, or a per-cell array by its shape and range."""
    if np.ndim(v) == 0:
        return v
    a = np.asarray(v, dtype=np.float64)
    return ("cell", a.shape, float(a.min()), float(a.max()))


def _plain(v):
    a = np.asarray(v, dtype=np.float64)
    if a.ndim == 0:
        return float(a)
    if a.size <= 4:
        return tuple(float(x) for x in a.ravel())
    return ("array", a.shape, float(a.min()), float(a.max()))


class NavierStokesForm:
    """F = 2 nu eps(u):eps(v) - (p/rho) div v + (q/rho) div u - f.v + (grad(u) u0).v [+ (1/dt)(u - u_prev).v]
    with u0 = the velocity of ``w_current`` (CoupledNavierStokesSolver.py:288-381).  ``newton``: the reference's
    action(F, w_current) + derivative (Newton); otherwise the Picard linearisation with u0 frozen."""

    def __init__(self, space):
        self.space = space
        self.nu = None
        self.rho = None
        self.inv_dt = 0.0
        self.body_force = None        # 3 numbers or None
        self.w_current = None         # Function (late bound, like UFL coefficients)
        self.w_prev = None
        self.newton = True
        self.symmetric = False
        self.nonlinear = True
        # pressure boundaries: [(marker_id, value | None)]: + inner(value*n, v)*ds(id) (value given) and
        # - nu*inner((grad(u) + grad(u).T)*n, v)*ds(id)   (CoupledNavierStokesSolver.py:449-453, 459-460)
        self.pressure_boundaries = []
        # ALE frame (reference_frame_settings {'type': 'ALE', 'mesh_velocity': ..}, :321-329): advecting velocity u0 - w
        self.mesh_velocity = None     # 3 numbers or None
        # G2 stabilisation (advection_settings {'stabilization_method': 'G2', 'Re':, 'kappa1':, 'kappa2':}, :334-363):
        # (mode, kappa1) with mode 1 for Re <= 1 (delta1 = kappa1 h^2), 2 otherwise; None = off
        self.g2 = None
        # non-Newtonian law (material 'Newtonian': False, :194-213): (p_ref, exponent) -> nu (p / p_ref)^exponent; None = off
        self.viscosity_law = None

    @staticmethod
    def _value_name(v):
        try:
            return "Constant(%g)" % float(v)
        except (TypeError, ValueError):
            return type(v).__name__

    def describe(self):
        d = self.space.velocity_dim() if hasattr(self.space, "velocity_dim") else 3      # vectors are stored padded to 3 slots
        return {"type": "navier_stokes", "nu": self.nu, "rho": self.rho, "inv_dt": self.inv_dt,
                "pressure_boundaries": [(int(m), None if v is None else self._value_name(v)) for m, v in self.pressure_boundaries],
                "body_force": None if self.body_force is None else [float(x) for x in self.body_force][:d],
                "mesh_velocity": None if self.mesh_velocity is None else [float(x) for x in self.mesh_velocity][:d],
                "g2": None if self.g2 is None else [int(self.g2[0]), float(self.g2[1])],
                "viscosity_law": None if self.viscosity_law is None else [float(self.viscosity_law[0]), float(self.viscosity_law[1])],
                "newton": bool(self.newton)}


class DGScalarForm:
    """Upwind SIPG advection-diffusion on a DG1 space (ScalarTransportDGSolver.py:119-147): c a(T, v) - N(T; v) - int f v dx, with
    constant conductivity (c kappa), capacity c, velocity beta and penalty alpha; transient: the theta = 1/2 scheme
    c/dt int (T - T_prev) v dx + c (a(T, v) + a(T_prev, v)) / 2 - N(T; v) - int f v dx."""

    def __init__(self, space):
        self.space = space
        self.conductivity = None      # c kappa (number)
        self.capacity = None          # c (number)
        self.velocity = None          # beta: d numbers
        self.alpha = None
        self.transient = False
        self.dt = None
        self.T_prev = None            # Function on the DG space
        self.facet_loads = []         # [FacetLoad]: + int g v ds (g: number or [n_facets, d] vertex values)
        self.robin = []               # [FacetRobin]: + int h (T - T_a) v ds
        self.sources = []             # [VolumeCoefficient]: 'const', 'cell' [n_cells] or 'nodal' [n_dofs] (values at every dof)

    def describe(self):
        return {
            "type": "dg_transport", "conductivity": self.conductivity, "capacity": self.capacity,
            "velocity": None if self.velocity is None else tuple(float(x) for x in self.velocity), "alpha": self.alpha,
            "transient": bool(self.transient), "dt": self.dt,
            "facet_loads": [(f.marker_id, _plain(f.g), f.origin) for f in self.facet_loads],
            "robin": [(r.marker_id, float(r.h), _plain(r.ambient)) for r in self.robin],
            "sources": [s.describe() for s in self.sources],
        }
