"""LinearElasticitySolver — small-strain isotropic elasticity on vector P1 / P2, GPU back end.

Counterpart of FenicsSolver/LinearElasticitySolver.py: same class/constructor (forces
vector_name='displacement', :55-60), sigma(u) = 2 mu sym(grad u) + lambda div(u) I
(:62-69), boundary types displacement/Dirichlet (per-component with None = free,
:122-131), force / pressure / stress (:165-196), body force (:227-228), thermal stress
(:78-85, 231-238); 3D problems go through solve_amg (CG), as in the reference (:247-253).

Modal analysis (solve_modal / solve_modal_form, :270-312): the lowest modes of K phi = lambda M phi with the consistent mass
M = int rho phi . psi dx, by LOBPCG on the device (fs_eigen_solve; AMG-preconditioned in 3D, Jacobi in 2D).  The reference's
stub asks SLEPc for the largest eigenvalue of K alone, a mesh-scale number of no engineering use.

Linear buckling (solve_buckling; no counterpart in the reference): the static solve of the case as given, the
geometric stiffness K_G of its per-cell stress (fs_assemble_geometric_stiffness), and the smallest factors lambda > 0 of
(K + lambda K_G) phi = 0 by the same LOBPCG on K_G phi = nu K phi (fs_buckling_solve).  Vector P1, one rank.

Frictionless contact and sliding supports (boundary types 'contact' and 'sliding'; the reference lists the boundary condition as
not implemented): n.u <= g against a rigid obstacle, or n.u = value, at the vertices of the marked facets, by the
primal-dual active-set strategy in per-node Householder frames, where the constraint is a component Dirichlet condition
(solve_contact; fs_matrix_rotate_nodes, fs_contact_update).  Vector P1, one rank, static cases.

Anisotropic materials (the reference lists them as a to-do, "anisotropy needs rank 4 tensor"): ``elasticity_tensor``
(a 6x6 in the standard Voigt order 11, 22, 33, 23, 13, 12 with engineering shears) or ``orthotropic`` (E1..3, nu12 / 13 / 23,
G12 / 13 / 23), each per region as well, with an optional ``material_orientation`` (a rotation whose columns are the material axes,
two axes to orthonormalise, a per-region dict, or a degree-0 Expression with 9 values for per-cell frames) and a
``thermal_expansion_coefficient`` of 3 principal values or a symmetric 3x3 in material axes.  The operator, the stress with its
von Mises load and the eigenstrain load are kernels of their own (fs_assemble_anisotropic, fs_anisotropic_stress,
fs_assemble_anisotropic_load).  Vector P1, one rank; no contact / sliding sides, no solving_dynamics, no buckling.

Reference quirk kept by default (Appendix B-Q3): body forces and tractions are ADDED to
F (:227-228, 242-243), so they act with reversed sign; set
``solver.reference_load_sign = False`` for the physical convention.  The thermal term has
the conventional sign in both.

Vector P2 (the reference's own example, examples/test_linear_elasticity.py:105-106) runs on one GPU; its solve_amg uses
Jacobi-CG (the aggregation hierarchy is built on P1 node patterns).  ``von_Mises`` is the consistent L2 projection onto P1,
assembled and solved on the device (fs_assemble_von_mises + P1 mass matrix + CG).  Elastodynamics
(``solving_dynamics = True``, :216-220) subtracts rho * acceleration with the reference's own finite-difference
acceleration (SolverBase.py:477-482, including its division by 1/dt).

Material: ``elastic_modulus``, ``poisson_ratio``, ``thermal_expansion_coefficient`` and ``density`` may vary from cell to
cell (the reference multiplies in whatever ``material[...]`` holds, :62-85): a per-region dict
{'name': {'subdomain_id': i, 'value': v}}, a degree-0 Expression (at the cell mid-points) or, on CG1 spaces, a scalar
Function / Expression (the mean of its vertex values).  Numbers and scalar Constants keep the homogeneous path.
"""
from __future__ import annotations

import numbers

import numpy as np

from .fem import Measure, Constant, Expression, UserExpression, Function, DirichletBC, nodal_values, is_constant_value
from .SolverBase import SolverBase, SolverError
from . import case, forms


# standard Voigt order (11, 22, 33, 23, 13, 12) -> the library's tensor order (xx, yy, zz, xy, xz, yz)
VOIGT_TO_LIBRARY = [0, 1, 2, 5, 4, 3]
_ANISO_KEYS = ('elasticity_tensor', 'orthotropic')


def isotropic_stiffness(E, nu):
    """The 6x6 stiffness of an isotropic material in the standard Voigt order (11, 22, 33, 23, 13, 12), engineering shears."""
    E, nu = float(E), float(nu)
    mu, lmbda = E / (2.0 * (1.0 + nu)), E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
    C = np.zeros((6, 6))
    C[:3, :3] = lmbda
    C[np.arange(3), np.arange(3)] += 2.0 * mu
    C[np.arange(3, 6), np.arange(3, 6)] = mu
    return C


def orthotropic_stiffness(E, nu, G):
    """The 6x6 stiffness, standard Voigt order (11, 22, 33, 23, 13, 12), of an orthotropic material in its own axes from
    E = (E1, E2, E3), nu = (nu12, nu13, nu23) and G = (G12, G13, G23): the inverse of the compliance with S_11 = 1/E1,
    S_12 = -nu12/E1, S_13 = -nu13/E1, S_23 = -nu23/E2, S_44 = 1/G23, S_55 = 1/G13, S_66 = 1/G12."""
    E, nu, G = (np.asarray(x, dtype=np.float64).ravel() for x in (E, nu, G))
    if E.size != 3 or nu.size != 3 or G.size != 3:
        raise SolverError('orthotropic material: three elastic moduli, three Poisson ratios (nu12, nu13, nu23) and three shear '
                          'moduli (G12, G13, G23) are expected')
    if not (np.all(np.isfinite(np.concatenate([E, nu, G]))) and np.all(E > 0.0) and np.all(G > 0.0)):
        raise SolverError('orthotropic material: the elastic and shear moduli must be positive and finite')
    S = np.zeros((6, 6))
    S[0, 0], S[1, 1], S[2, 2] = 1.0 / E
    S[0, 1] = S[1, 0] = -nu[0] / E[0]
    S[0, 2] = S[2, 0] = -nu[1] / E[0]
    S[1, 2] = S[2, 1] = -nu[2] / E[1]
    S[3, 3], S[4, 4], S[5, 5] = 1.0 / G[2], 1.0 / G[1], 1.0 / G[0]
    if abs(np.linalg.det(S[:3, :3])) == 0.0:
        raise SolverError('orthotropic material: the compliance is singular')
    C = np.linalg.inv(S)
    return 0.5 * (C + C.T)


def _rotation_from(value, what):
    """A proper rotation [3, 3] (columns = material axes in global coordinates) from a 3x3 matrix (2x2: about z) or
    {'axis_1': v, 'axis_2': w} (orthonormalised: e1 = v/|v|, e2 = w less its part along e1, e3 = e1 x e2)."""
    if isinstance(value, dict):
        if 'axis_1' not in value or 'axis_2' not in value:
            raise SolverError("{}: a 3x3 rotation or {{'axis_1': v, 'axis_2': w}} is expected".format(what))
        v, w = (np.asarray(value[k], dtype=np.float64).ravel() for k in ('axis_1', 'axis_2'))
        if v.size == 2 and w.size == 2:
            v, w = np.append(v, 0.0), np.append(w, 0.0)
        if v.size != 3 or w.size != 3 or not np.all(np.isfinite(np.concatenate([v, w]))):
            raise SolverError('{}: axis_1 and axis_2 must be finite vectors of 3 numbers'.format(what))
        if np.linalg.norm(v) == 0.0:
            raise SolverError('{}: axis_1 is a zero vector'.format(what))
        e1 = v / np.linalg.norm(v)
        w = w - (w @ e1) * e1
        if np.linalg.norm(w) <= 1e-12 * max(1.0, np.linalg.norm(value['axis_2'])):
            raise SolverError('{}: axis_2 is parallel to axis_1'.format(what))
        e2 = w / np.linalg.norm(w)
        return np.stack([e1, e2, np.cross(e1, e2)], axis=1)
    try:
        R = np.asarray(value, dtype=np.float64)
    except (TypeError, ValueError):
        raise SolverError('{}: a 3x3 rotation matrix is expected'.format(what))
    if R.shape == (2, 2):
        R3 = np.eye(3)
        R3[:2, :2] = R
        R = R3
    if R.shape == (9,):
        R = R.reshape(3, 3)
    if R.shape != (3, 3):
        raise SolverError('{}: a 3x3 rotation matrix is expected, got shape {}'.format(what, R.shape))
    _check_rotations(R[None], what)
    return R


def _check_rotations(R, what):
    """SolverError unless every R[c] has max|R^T R - I| <= 1e-10 and det > 0."""
    if not np.all(np.isfinite(R)):
        raise SolverError('{}: the rotation is not finite'.format(what))
    err = np.abs(np.einsum('cki,ckj->cij', R, R) - np.eye(3)[None]).max(axis=(1, 2))
    det = np.linalg.det(R)
    bad = (err > 1e-10) | ~(det > 0.0)
    if bad.any():
        c = int(np.argmax(bad))
        where = '' if len(R) == 1 else ' in cell {}'.format(c)
        raise SolverError('{}{}: not a proper rotation (max|R^T R - I| = {:.3e}, det = {:.3g})'.format(what, where, err[c], det[c]))


class LinearElasticitySolver(SolverBase):
    def __init__(self, case_settings):
        case_settings['vector_name'] = 'displacement'
        SolverBase.__init__(self, case_settings)
        self.solving_modal = False
        self.solving_dynamics = False
        self.reference_load_sign = True

    # ------------------------------------------------------------------ anisotropic materials
    def is_anisotropic(self):
        return any(k in self.material and self.material[k] is not None for k in _ANISO_KEYS)

    def _no_lame(self, what):
        return SolverError("{}: {} is defined for an isotropic material (elastic_modulus, poisson_ratio) only; the case gives "
                           "'elasticity_tensor' / 'orthotropic', and this path does not take an anisotropic material".format(
                               type(self).__name__, what))

    def _regions_of(self, value, is_leaf):
        """[(region name or None, leaf value, cell mask or None)] of a material entry that is a leaf or a per-region dict
        {'name': {'subdomain_id': i, 'value': leaf}} (the leaf's own keys may also stand beside 'subdomain_id')."""
        if is_leaf(value):
            return [(None, value, None)]
        if not (isinstance(value, dict) and value and all(isinstance(it, dict) and 'subdomain_id' in it for it in value.values())):
            return None
        if getattr(self, 'subdomains', None) is None:
            raise SolverError('a per-region material needs the subdomain markers of the mesh')
        ids = self.subdomains.array()
        out = []
        for name, item in value.items():
            leaf = item['value'] if 'value' in item else {k: v for k, v in item.items() if k != 'subdomain_id'}
            out.append((name, leaf, ids == item['subdomain_id']))
        covered = np.zeros(len(ids), dtype=bool)
        for _, _, mask in out:
            covered |= mask
        if not covered.all():
            raise SolverError('multi-region value does not cover every subdomain id of the mesh')
        return out

    def _stiffness_of(self, key, leaf, region):
        """One 6x6 in the library order from a leaf of material[key], checked for symmetry and positive definiteness."""
        what = "material '{}'".format(key) + ('' if region is None else " of region '{}'".format(region))
        if key == 'orthotropic':
            if not isinstance(leaf, dict) or not all(k in leaf for k in ('elastic_moduli', 'poisson_ratios', 'shear_moduli')):
                raise SolverError("{}: {{'elastic_moduli': [E1, E2, E3], 'poisson_ratios': [nu12, nu13, nu23], 'shear_moduli': "
                                  "[G12, G13, G23]}} is expected".format(what))
            try:
                Cv = orthotropic_stiffness(leaf['elastic_moduli'], leaf['poisson_ratios'], leaf['shear_moduli'])
            except SolverError as e:
                raise SolverError('{}: {}'.format(what, e))
        else:
            try:
                Cv = np.asarray(leaf, dtype=np.float64)
            except (TypeError, ValueError):
                raise SolverError('{}: a 6x6 matrix of numbers is expected'.format(what))
            if Cv.shape != (6, 6):
                raise SolverError('{}: a 6x6 matrix in Voigt order (11, 22, 33, 23, 13, 12) is expected, got shape {}'.format(what, Cv.shape))
        if not np.all(np.isfinite(Cv)):
            raise SolverError('{}: the stiffness is not finite'.format(what))
        scale = np.abs(Cv).max()
        if not np.abs(Cv - Cv.T).max() <= 1e-12 * scale:
            raise SolverError('{}: the stiffness matrix is not symmetric (max|C - C^T| = {:.3e})'.format(what, np.abs(Cv - Cv.T).max()))
        Cv = 0.5 * (Cv + Cv.T)
        try:
            np.linalg.cholesky(Cv)
        except np.linalg.LinAlgError:
            raise SolverError('{}: the stiffness matrix is not positive definite (smallest eigenvalue {:.3e})'.format(
                what, np.linalg.eigvalsh(Cv).min()))
        D = Cv[np.ix_(VOIGT_TO_LIBRARY, VOIGT_TO_LIBRARY)]
        if self.dimension == 2 and np.abs(D[:4, 4:]).max() > 1e-12 * scale:
            raise SolverError('{}: plane strain needs a material that is monoclinic about z (no coupling between the in-plane '
                              'strains and the out-of-plane shears); rotate the material about z only'.format(what))
        return D

    def _orientation_frames(self):
        """None or the frames [n_cells, 3, 3] of material['material_orientation']."""
        v = self.material.get('material_orientation')
        if v is None:
            return None
        nc = self.mesh.num_cells()
        what = "material 'material_orientation'"
        if isinstance(v, (Expression, UserExpression)):
            if v.value_size() != 9 or getattr(v, 'degree', 0) != 0:
                raise SolverError(what + ': an Expression must have degree 0 and 9 values (the rotation, row-major)')
            co = self.mesh.coordinates()
            R = np.asarray(v.eval_points(co[self.mesh.cells().astype(np.int64)].mean(axis=1)), dtype=np.float64).reshape(nc, 3, 3)
            _check_rotations(R, what)
        else:
            leaf = lambda x: not isinstance(x, dict) or 'axis_1' in x or 'axis_2' in x
            regions = self._regions_of(v, leaf)
            if regions is None:
                raise SolverError(what + ": a 3x3 rotation, {'axis_1': v, 'axis_2': w}, a per-region dict of either or a degree-0 "
                                  "Expression with 9 values is expected")
            R = np.empty((nc, 3, 3))
            for name, item, mask in regions:
                Rr = _rotation_from(item, what + ('' if name is None else " of region '{}'".format(name)))
                R[slice(None) if mask is None else mask] = Rr
        if self.dimension == 2 and (np.abs(R[:, 2, :2]).max() > 1e-12 or np.abs(R[:, :2, 2]).max() > 1e-12 or np.abs(R[:, 2, 2] - 1.0).max() > 1e-12):
            raise SolverError(what + ': plane strain needs rotations about z')
        return R

    def _expansion_tensors(self):
        """alpha per cell [n_cells, 3, 3] in material axes from material['thermal_expansion_coefficient']: a number, 3 principal values
        or a symmetric 3x3, per region as well."""
        v = self.material['thermal_expansion_coefficient']
        what = "material 'thermal_expansion_coefficient'"

        def tensor(x, where):
            if isinstance(x, Constant):
                x = x.values()
            try:
                a = np.asarray(x, dtype=np.float64)
            except (TypeError, ValueError):
                raise SolverError(where + ': a number, 3 principal values or a symmetric 3x3 is expected')
            if a.size == 1:
                a = float(a.ravel()[0]) * np.eye(3)
            elif a.shape == (3,):
                a = np.diag(a)
            if a.shape != (3, 3) or not np.all(np.isfinite(a)) or np.abs(a - a.T).max() > 1e-12 * max(np.abs(a).max(), 1e-300):
                raise SolverError(where + ': a number, 3 principal values or a symmetric 3x3 is expected')
            return 0.5 * (a + a.T)
        nc = self.mesh.num_cells()
        regions = self._regions_of(v, lambda x: not isinstance(x, dict))
        if regions is None:
            raise SolverError(what + ': a number, 3 principal values, a symmetric 3x3 or a per-region dict of these is expected')
        A = np.empty((nc, 3, 3))
        for name, item, mask in regions:
            A[slice(None) if mask is None else mask] = tensor(item, what + ('' if name is None else " of region '{}'".format(name)))
        return A

    def anisotropic_material(self):
        """None for an isotropic case; else the forms.AnisotropicElasticity of material['elasticity_tensor'] / ['orthotropic'] with
        ['material_orientation'] (host only; every distinct material checked for symmetry and positive definiteness)."""
        if not self.is_anisotropic():
            return None
        given = [k for k in _ANISO_KEYS if self.material.get(k) is not None]
        iso = [k for k in ('elastic_modulus', 'poisson_ratio') if self.material.get(k) is not None]
        if len(given) > 1 or iso:
            raise SolverError("material: '{}' is given together with {}; give one description of the stiffness (isotropic regions "
                              "go under 'elasticity_tensor' as isotropic_stiffness(E, nu))".format(
                                  given[0], ', '.join("'{}'".format(k) for k in given[1:] + iso)))
        key = given[0]
        v = self.material[key]
        is_leaf = (lambda x: isinstance(x, dict) and 'elastic_moduli' in x) if key == 'orthotropic' else (lambda x: not isinstance(x, dict))
        regions = self._regions_of(v, is_leaf)
        if regions is None:
            raise SolverError("material '{}': {} or a per-region dict {{'name': {{'subdomain_id': i, 'value': ...}}}} is expected".format(
                key, 'a 6x6 matrix' if key == 'elasticity_tensor' else "{'elastic_moduli', 'poisson_ratios', 'shear_moduli'}"))
        table = np.stack([self._stiffness_of(key, leaf, name) for name, leaf, _ in regions])
        index = None
        if regions[0][2] is not None:
            index = np.zeros(self.mesh.num_cells(), dtype=np.int32)
            for k, (_, _, mask) in enumerate(regions):
                index[mask] = k
        return forms.AnisotropicElasticity(table, index, self._orientation_frames())

    def stiffness_tensor(self):
        """(table [n, 6, 6], material_of_cell [n_cells] or None, frames [n_cells, 3, 3] or None) of an anisotropic case: the distinct
        stiffness matrices in the LIBRARY's order (xx, yy, zz, xy, xz, yz; engineering shears) and material axes, the table row of
        every cell, and the rotations whose columns are the material axes in global coordinates."""
        mat = self.anisotropic_material()
        if mat is None:
            raise SolverError("stiffness_tensor: the material is isotropic (no 'elasticity_tensor' / 'orthotropic'); see lame_parameters")
        return mat.table.copy(), None if mat.index is None else mat.index.copy(), None if mat.frames is None else mat.frames.copy()

    def _refuse_anisotropic_case(self):
        """What the anisotropic operator is written for: vector CG1, one rank, not periodic, no constraint sides, not the
        solving_dynamics branch (no device call is made here)."""
        from . import parallel
        V = self.function_space
        what = 'an anisotropic material'
        if V.degree() != 1:
            raise SolverError(what + ': P2 displacement spaces are not supported - the kernel integrates the constant strain of a '
                              'P1 cell; use a P1 space')
        if parallel.active():                    # (a file mesh that one GPU holds in locality order has a localizer too: that one is served)
            raise SolverError(what + ' runs on one rank')
        if hasattr(V, 'periodic_pairs') and V.periodic_pairs() is not None:
            raise SolverError(what + ' on a periodic space is not supported')
        names = self._constraint_side_names()
        if names:
            raise SolverError(what + ": 'contact' / 'sliding' boundary conditions ({}) are not supported with it".format(', '.join(names)))
        if self.solving_dynamics:
            raise SolverError(what + ': solving_dynamics is not supported with it')

    @staticmethod
    def _tensor_storage(T, d):
        """[n, 3, 3] symmetric tensors -> the tensor storage [n, 6] (xx, yy, zz, xy, xz, yz) or, d == 2, [n, 4] (xx, yy, zz, xy)."""
        cols = [T[:, 0, 0], T[:, 1, 1], T[:, 2, 2], T[:, 0, 1]] + ([T[:, 0, 2], T[:, 1, 2]] if d == 3 else [])
        return np.stack(cols, axis=1)

    def material_field(self, name):
        """material[name] as a number (homogeneous: a number or a scalar Constant) or an array with one value per cell of
        self.mesh: a per-region dict, a degree-0 Expression (cell mid-points), on CG1 spaces a scalar Function or Expression
        (the mean of its vertex values - what the P1 operator integrates exactly for a linear E)."""
        if name in ('elastic_modulus', 'poisson_ratio') and self.material.get(name) is None and self.is_anisotropic():
            raise self._no_lame("material '{}'".format(name))
        v = self.material[name]
        if isinstance(v, numbers.Number):
            return v
        if isinstance(v, Constant) and v.value_size() == 1:
            return float(v)
        if isinstance(v, forms.VolumeCoefficient) and v.kind in ('const', 'cell'):
            return float(v.value) if v.kind == 'const' else np.asarray(v.value, dtype=np.float64)
        if isinstance(v, dict):
            return case.cellwise_from_regions(v, self.subdomains)
        if isinstance(v, (Expression, UserExpression)) and v.value_size() == 1:
            if v.degree == 0:
                co = self.mesh.coordinates()
                return np.asarray(v.eval_points(co[self.mesh.cells().astype(np.int64)].mean(axis=1)), dtype=np.float64)
            self._require_cg1(name, 'an Expression of degree %d' % v.degree)
            from .fem import FunctionSpace
            return nodal_values(v, FunctionSpace(self.mesh, 'P', 1))[self.mesh.cells().astype(np.int64)].mean(axis=1)
        if isinstance(v, Function) and v.function_space()._ncomp == 1:
            self._require_cg1(name, 'a Function')
            return np.asarray(v.vertex_values(), dtype=np.float64)[self.mesh.cells().astype(np.int64)].mean(axis=1)
        raise SolverError("material '{}': a number, a scalar Constant, a per-region dict, a scalar Expression or (CG1) a scalar "
                          "Function is expected, got {}".format(name, type(v).__name__))

    def _require_cg1(self, name, what):
        if self.function_space.degree() != 1:
            raise SolverError("material '{}': {} is a nodal field; on a CG{} displacement space the material must be piecewise "
                              "constant (a number, a per-region dict or a degree-0 Expression)".format(
                                  name, what, self.function_space.degree()))

    def _bad_cell(self, name, ok):
        """SolverError naming the region (per-region input) or the first cell where ``ok`` fails."""
        bad = int(np.argmin(ok))
        v = self.material[name]
        if isinstance(v, dict) and getattr(self, 'subdomains', None) is not None:
            sid = self.subdomains.array()[bad]
            region = next((k for k, it in v.items() if it['subdomain_id'] == sid), sid)
            return SolverError("material '{}' of region '{}' is out of range".format(name, region))
        return SolverError("material '{}' is out of range in cell {}".format(name, bad))

    def lame_parameters(self):
        """(mu, lambda): numbers for a homogeneous material, arrays [n_cells] when E or nu vary from cell to cell.  An anisotropic
        material has none: SolverError (what makes solve_buckling and the inelastic / dynamic subclasses refuse it)."""
        if self.is_anisotropic():
            raise self._no_lame('lame_parameters')
        elasticity = self.material_field('elastic_modulus')
        nu = self.material_field('poisson_ratio')
        if np.ndim(elasticity) == 0 and np.ndim(nu) == 0:
            mu = elasticity / (2.0 * (1.0 + nu))
            lmbda = elasticity * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
            return mu, lmbda
        nc = self.mesh.num_cells()
        E = np.broadcast_to(np.asarray(elasticity, dtype=np.float64), (nc,))
        nu = np.broadcast_to(np.asarray(nu, dtype=np.float64), (nc,))
        for name, ok in (('elastic_modulus', E > 0.0), ('poisson_ratio', (nu > -1.0) & (nu < 0.5))):
            if not ok.all():
                raise self._bad_cell(name, ok)
        mu = E / (2.0 * (1.0 + nu))
        lmbda = E * nu / ((1.0 + nu) * (1.0 - 2.0 * nu))
        return mu, lmbda

    def _cell_gradients(self, u):
        """grad u per cell [nc,3,3] (component i, derivative j); P2 displacements: at the cell centroid."""
        co = self.mesh.coordinates()
        ce = self.mesh.cells().astype(np.int64)
        X = co[ce]
        d = ce.shape[1] - 1                 # 3: tetrahedra, 2: triangles ([nc,2,2] gradients)
        J = np.stack([X[:, k] - X[:, 0] for k in range(1, d + 1)], axis=2)
        Ji = np.linalg.inv(J)
        g = np.zeros((len(ce), d + 1, d))
        g[:, 1:, :] = Ji
        g[:, 0, :] = -Ji.sum(axis=1)
        V = u.function_space()
        if V.degree() == 1:
            return np.einsum("cai,caj->cij", u.vertex_values()[ce], g)
        cd = V.cell_nodes()
        if d == 2:
            # triangles at the centroid (lambda = 1/3): vertex i (4/3 - 1) g_i, edge (i,j): 4/3 (g_i + g_j)
            ei, ej = [1, 0, 0], [2, 2, 1]
            gv = g / 3.0
            ge = (4.0 / 3.0) * (g[:, ei, :] + g[:, ej, :])
            return np.einsum("cai,caj->cij", u.node_values()[cd], np.concatenate([gv, ge], axis=1))
        # tetrahedra at the centroid (lambda = 1/4): vertex functions have zero gradient there, edge (i,j): g_i + g_j
        ei, ej = [2, 1, 1, 0, 0, 0], [3, 3, 2, 3, 2, 1]
        U = u.node_values()[cd[:, 4:]]                  # [nc,6,3]
        ge = g[:, ei, :] + g[:, ej, :]
        return np.einsum("cai,caj->cij", U, ge)

    def sigma(self, u):
        """Cell-wise (DG0) stress tensor [nc,3,3] of a displacement Function (post-processing helper on the host; the
        reference returns the UFL expression, LinearElasticitySolver.py:62-69).  Anisotropic material: C : eps(u), [nc,2,2] (the
        in-plane part) in plane strain."""
        aniso = self.anisotropic_material()
        if aniso is not None:
            return self._sigma_anisotropic(u, aniso)
        mu, lmbda = self.lame_parameters()
        G = self._cell_gradients(u)
        eps = 0.5 * (G + np.transpose(G, (0, 2, 1)))
        tr = np.trace(G, axis1=1, axis2=2)
        if np.ndim(mu) > 0:                 # per-cell material
            mu, lmbda = np.asarray(mu)[:, None, None], np.asarray(lmbda)[:, None, None]
        return 2.0 * mu * eps + lmbda * tr[:, None, None] * np.eye(G.shape[1])[None]

    def _sigma_anisotropic(self, u, aniso):
        G = self._cell_gradients(u)
        d = G.shape[1]
        E = np.zeros((len(G), 3, 3))
        E[:, :d, :d] = 0.5 * (G + np.transpose(G, (0, 2, 1)))
        R = aniso.frames
        if R is not None:
            E = np.einsum('cki,ckl,clj->cij', R, E, R)                  # R^T E R: into the material axes
        ev = np.stack([E[:, 0, 0], E[:, 1, 1], E[:, 2, 2], 2.0 * E[:, 0, 1], 2.0 * E[:, 0, 2], 2.0 * E[:, 1, 2]], axis=1)
        D = aniso.table[aniso.index] if aniso.index is not None else np.broadcast_to(aniso.table[0], (len(G), 6, 6))
        sv = np.einsum('cij,cj->ci', D, ev)
        S = np.empty((len(G), 3, 3))
        S[:, 0, 0], S[:, 1, 1], S[:, 2, 2] = sv[:, 0], sv[:, 1], sv[:, 2]
        S[:, 0, 1] = S[:, 1, 0] = sv[:, 3]
        S[:, 0, 2] = S[:, 2, 0] = sv[:, 4]
        S[:, 1, 2] = S[:, 2, 1] = sv[:, 5]
        if R is not None:
            S = np.einsum('cik,ckl,cjl->cij', R, S, R)
        return S[:, :d, :d]

    def von_Mises(self, u):
        """project(sqrt(3/2 s:s), FunctionSpace(mesh, 'P', 1)) (:71-76): the consistent L2 projection, on the device -
        right-hand side int vm phi_a dx (fs_assemble_von_mises; anisotropic material: fs_anisotropic_stress with s the deviator
        of C : eps(u)), P1 mass matrix, Jacobi-CG to 1e-12."""
        from .fem import FunctionSpace
        from . import backend
        V = u.function_space()
        aniso = self.anisotropic_material()
        if aniso is not None:
            self._refuse_anisotropic_case()
        else:
            mu, lmbda = self.lame_parameters()
        P = FunctionSpace(self.mesh, 'P', 1)
        dV, dP = V.device(), P.device()
        loc, ploc = V.localizer(), P.localizer()
        uh = u.vector()._values()
        if loc is not None and not getattr(loc, 'is_identity', False):
            uh = loc.nodes(uh)                       # host field -> this rank's owned + ghost entries in device order
        ud = backend.DeviceVector(dV.n_local, uh)
        b = backend.DeviceVector(dP.n_owned)
        if aniso is not None:
            backend.anisotropic_stress(dV, ud, aniso.material(loc), p1_space=dP, vm_rhs=b)
        else:
            if np.ndim(mu) > 0:                      # per-cell material: (mu, lambda) pairs in device cell order
                pairs = np.stack([mu, lmbda], axis=1)
                mu, lmbda = ('cell', pairs if loc is None else loc.cells(pairs)), None
            backend.assemble_von_mises(dV, ud, mu, lmbda, dP, b)
        M = backend.DeviceMatrix(dP)
        M.assemble(mass=1.0)
        x = backend.DeviceVector(dP.n_local)
        st = backend.krylov_solve(M, b, x, rtol=1e-12, max_iter=2000, precond="jacobi", norm="preconditioned")
        if st['converged'] != 1:
            raise SolverError('von_Mises: the mass-matrix solve did not converge')
        f = Function(P)
        if ploc is None:
            f.vector().set_local(x.get()[:dP.n_owned])
        elif getattr(ploc, 'is_local_view', False):
            from . import parallel
            if parallel.world()[1] > 1:
                backend.halo_exchange(dP, x)
            f.vector()._adopt_device(x)
        else:
            from . import parallel
            f.vector().set_local(parallel.gather_owned(x.get()[:dP.n_owned], ploc.owned_gids(), ploc.n_global, 1))
        return f

    def thermal_stress_coefficient(self):
        """E alpha / (1 - 2 nu): a number, or an array [n_cells] for a material that varies from cell to cell."""
        elasticity = self.material_field('elastic_modulus')
        nu = self.material_field('poisson_ratio')
        tec = self.material_field('thermal_expansion_coefficient')
        return elasticity / (1.0 - 2.0 * nu) * tec

    def thermal_stress(self, T):
        """The isotropic thermal stress  E/(1-2nu) * alpha * (T - T_ref)  (the multiplier of Identity(dim),
        LinearElasticitySolver.py:78-85) for a number, an array of nodal temperatures or a Function.  A per-cell material
        gives one value per cell, a nodal temperature entering by its mean at the cell's vertices."""
        vals = T.vector()._values() if isinstance(T, Function) else np.asarray(T, dtype=np.float64)
        coef = self.thermal_stress_coefficient()
        if np.ndim(coef) > 0 and np.ndim(vals) > 0:
            vals = vals[:self.mesh.num_vertices()][self.mesh.cells().astype(np.int64)].mean(axis=1)
        return coef * (vals - float(self.reference_values['temperature']))

    def strain_energy(self, u):
        raise SolverError("strain_energy: the reference's expression (LinearElasticitySolver.py:87-93) uses an undefined "
                          "symbol and '^' on UFL objects; nothing to reproduce")

    _MODAL_DEFAULTS = {'number_of_modes': 6, 'tolerance': 1e-8, 'max_iterations': 500, 'shift': 0.0}

    def modal_settings(self):
        """settings['solver_settings']['modal_settings'] with its defaults, checked (SolverError on a bad value)."""
        given = self.solver_settings.get('modal_settings') or {}
        unknown = set(given) - set(self._MODAL_DEFAULTS)
        if unknown:
            raise SolverError('modal_settings: unknown key(s) {}'.format(sorted(unknown)))
        ms = dict(self._MODAL_DEFAULTS, **given)
        nm = ms['number_of_modes']
        if isinstance(nm, bool) or not isinstance(nm, numbers.Integral) or not 1 <= nm <= 32:
            raise SolverError('modal_settings: number_of_modes must be an integer in 1..32, got {!r}'.format(nm))
        for key, low in (('tolerance', 0.0), ('max_iterations', 0)):
            if isinstance(ms[key], bool) or not isinstance(ms[key], numbers.Real) or not ms[key] > low:
                raise SolverError('modal_settings: {} must be positive, got {!r}'.format(key, ms[key]))
        if isinstance(ms['shift'], bool) or not isinstance(ms['shift'], numbers.Real) or not ms['shift'] >= 0.0:
            raise SolverError('modal_settings: shift must be a number >= 0, got {!r}'.format(ms['shift']))
        return {'number_of_modes': int(nm), 'tolerance': float(ms['tolerance']), 'max_iterations': int(ms['max_iterations']),
                'shift': float(ms['shift'])}

    def solve_modal_form(self, F, bcs):
        """The lowest natural modes of the form's stiffness and the consistent mass, the displacement BCs' dofs constrained (their
        prescribed values and every load are ignored).  Sets self.eigenvalues (ascending, rad^2/s^2), self.natural_frequencies (Hz)
        and self.modes (M-normalised Functions); returns mode 1."""
        from . import backend, parallel
        ms = self.modal_settings()
        if parallel.world()[1] > 1 or F.space.localizer() is not None:
            raise SolverError('modal analysis runs on one rank')
        if hasattr(F.space, 'periodic_pairs') and F.space.periodic_pairs() is not None:
            raise SolverError('modal analysis on a periodic space is not supported')
        dofs, vals = self._bc_arrays(bcs)
        constrained = np.unique(dofs)
        nm, shift = ms['number_of_modes'], ms['shift']
        n_free = F.space.dim() - constrained.size
        if nm >= n_free:
            raise SolverError('modal_settings: {} modes asked of a space with {} free dofs'.format(nm, n_free))
        if constrained.size == 0 and shift <= 0.0:
            raise SolverError('modal analysis of a free-free part (no displacement BC) needs modal_settings shift > 0')
        if np.any(vals != 0.0):
            self.logger.info('solve_modal: prescribed displacements are ignored, their dofs are held at zero')
        rho = self.material_field('density')
        rho_spec = float(rho) if np.ndim(rho) == 0 else ('cell', np.asarray(rho, dtype=np.float64))
        shifted = None if shift == 0.0 else (shift * rho_spec if np.ndim(rho) == 0 else ('cell', shift * rho_spec[1]))
        V = F.space.device()
        K = backend.DeviceMatrix(V)
        if F.anisotropic is not None:
            if F.space.localizer() is not None:
                # (the guard above runs before device() exists: a file mesh uploaded in locality order gets its localizer here, and
                # the constrained dofs and the modes below are in the host's numbering)
                raise SolverError('modal analysis with an anisotropic material: the mesh was uploaded in locality order (FS_RENUMBER=1, '
                                  'or a tetrahedral file mesh of {} vertices or more), which solve_modal does not serve; set '
                                  'FS_RENUMBER=0'.format(type(F.space).RENUMBER_MIN_VERTICES))
            K.assemble_anisotropic(F.anisotropic.material(), mass=shifted)
        else:
            K.assemble(lame=F.lame_spec(), mass=shifted)          # K + shift M: one form
        M = backend.DeviceMatrix(V)
        M.assemble(lame=(0.0, 0.0), mass=rho_spec)
        if constrained.size:
            K.apply_dirichlet(None, constrained, np.zeros(constrained.size), symmetric=True)
        amg = None
        if self.dimension == 3:
            amg, _ = self._amg_hierarchy(K, None, "rigid_body")
        try:
            lam, modes, st = backend.eigen_solve(K, M, nm, amg=amg, constrained=constrained, tol=ms['tolerance'],
                                                 max_iter=ms['max_iterations'], shift=shift)
        finally:
            if amg is not None:
                amg.close()
        self.modal_stats = st
        if st['n_converged'] < nm:
            raise SolverError('solve_modal: {} of {} modes converged in {} iterations (largest relative residual {:.3e})'.format(
                st['n_converged'], nm, st['iterations'], st['max_rel_residual']))
        self.eigenvalues = np.asarray(lam, dtype=np.float64)
        self.natural_frequencies = np.sqrt(np.maximum(self.eigenvalues, 0.0)) / (2.0 * np.pi)
        self.modes = []
        for x in modes:
            f = Function(self.function_space)
            f.vector().set_local(x.get()[:V.n_owned])
            self.modes.append(f)
        self.logger.info('solve_modal: %d modes in %d iterations, %.1f ms, f = %s Hz', nm, st['iterations'], st['solve_ms'],
                         np.array2string(self.natural_frequencies, precision=5))
        return self.modes[0]

    # ------------------------------------------------------------------ linear buckling
    _BUCKLING_DEFAULTS = {'number_of_modes': 4, 'tolerance': 1e-8, 'max_iterations': 500}

    def buckling_settings(self):
        """settings['solver_settings']['buckling_settings'] with its defaults, checked (SolverError on a bad value)."""
        given = self.solver_settings.get('buckling_settings') or {}
        unknown = set(given) - set(self._BUCKLING_DEFAULTS)
        if unknown:
            raise SolverError('buckling_settings: unknown key(s) {}'.format(sorted(unknown)))
        bs = dict(self._BUCKLING_DEFAULTS, **given)
        nm = bs['number_of_modes']
        if isinstance(nm, bool) or not isinstance(nm, numbers.Integral) or not 1 <= nm <= 32:
            raise SolverError('buckling_settings: number_of_modes must be an integer in 1..32, got {!r}'.format(nm))
        for key, low in (('tolerance', 0.0), ('max_iterations', 0)):
            if isinstance(bs[key], bool) or not isinstance(bs[key], numbers.Real) or not bs[key] > low:
                raise SolverError('buckling_settings: {} must be positive, got {!r}'.format(key, bs[key]))
        return {'number_of_modes': int(nm), 'tolerance': float(bs['tolerance']), 'max_iterations': int(bs['max_iterations'])}

    def _refuse_buckling_space(self, what):
        """The spaces the geometric stiffness is written for: vector CG1, one rank, not periodic (no device call is made here)."""
        from . import parallel
        V = self.function_space
        if V.degree() != 1:
            raise SolverError('{}: P2 displacement spaces are not supported - the geometric stiffness of a stress that is linear '
                              'in the cell needs its own quadrature kernel (a follow-up); use a P1 space'.format(what))
        if parallel.world()[1] > 1 or V.localizer() is not None:
            raise SolverError('{} runs on one rank'.format(what))
        if hasattr(V, 'periodic_pairs') and V.periodic_pairs() is not None:
            raise SolverError('{} on a periodic space is not supported'.format(what))

    def _geometric_stiffness(self, u, cell_stress):
        from . import backend
        if self.is_anisotropic():
            raise self._no_lame('geometric_stiffness')
        self._refuse_buckling_space('geometric_stiffness')
        u = self.w_current if u is None else u
        F = forms.ElasticityForm(self.function_space)
        F.mu, F.lmbda = self.lame_parameters()
        V = self.function_space.device()
        ud = backend.DeviceVector(V.n_local, u.vector()._values())
        KG = backend.DeviceMatrix(V)
        return KG, KG.assemble_geometric(F.lame_spec(), ud, cell_stress=cell_stress)

    def geometric_stiffness(self, u=None):
        """The geometric stiffness K_G[(a,i),(b,j)] = delta_ij sum_cells |c| grad N_a . sigma_c grad N_b of the stress sigma(u) (u: a
        displacement Function, default the current one), as a backend.DeviceMatrix without Dirichlet rows."""
        return self._geometric_stiffness(u, False)[0]

    def solve_buckling(self):
        """Linear (eigenvalue) buckling: the static solve of the case as given - its loads are the reference load - then the smallest
        factors lambda > 0 with (K + lambda K_G) phi = 0, K_G the geometric stiffness of the static stress, every dof that carries
        a displacement BC held at zero in the modes.  Sets self.buckling_factors (ascending), self.buckling_modes (Functions scaled to
        max |component| = 1), self.prestress (per-cell stress [n_cells, 6] as xx, yy, zz, xy, xz, yz, or [n_cells, 4] as xx, yy,
        zz, xy in plane strain) and self.buckling_stats; the static displacement stays where solve() leaves it.  Returns mode 1."""
        import time
        from . import backend
        bs = self.buckling_settings()
        what = 'solve_buckling'
        if self.is_anisotropic():
            raise self._no_lame(what + ' (the geometric stiffness of its prestress)')
        self._refuse_constraint_sides(what)
        self._refuse_buckling_space('buckling analysis')
        if self.settings.get('temperature_distribution') is not None or getattr(self, 'temperature_distribution', None) is not None:
            raise SolverError(what + ': a thermal prestress (temperature_distribution) is not supported')
        if self.transient_settings['transient']:
            raise SolverError(what + ': the reference load is a static load; transient_settings must not be transient')
        if not any(bc.get('type') in ('Dirichlet', 'displacement') for bc in self.boundary_conditions.values()):
            raise SolverError(what + ': no displacement boundary condition - the static solve of the reference load is singular')
        nm = bs['number_of_modes']
        t0 = time.perf_counter()
        u0 = self.solve()
        backend.synchronize()
        t1 = time.perf_counter()
        F, bcs = self.generate_form(0, None, None, self.w_current, self.w_prev)
        constrained = np.unique(self._bc_arrays(bcs)[0])
        n_free = F.space.dim() - constrained.size
        if nm >= n_free:
            raise SolverError('buckling_settings: {} modes asked of a space with {} free dofs'.format(nm, n_free))
        V = F.space.device()
        K = backend.DeviceMatrix(V)
        K.assemble(lame=F.lame_spec())
        KG, self.prestress = self._geometric_stiffness(u0, True)
        K.apply_dirichlet(None, constrained, np.zeros(constrained.size), symmetric=True)
        backend.synchronize()
        t2 = time.perf_counter()
        amg = None
        if self.dimension == 3:
            # An operator of at most 500 rows is a single level by default, whose "cycle" is the smoother alone - no better than
            # Jacobi, and K is the B matrix here: a part that small gets a coarse level of its own.
            sp_ = self.solver_settings.get('solver_parameters', {}) or {}
            amg = backend.AMG(K, nullspace="rigid_body", strength_threshold=float(sp_.get('amg_strength_threshold', 0.0)),
                              coarse_size=max(12, V.n_owned // 8) if V.n_owned <= 500 else 0)
        backend.synchronize()
        t3 = time.perf_counter()
        try:
            lam, modes, st = backend.buckling_solve(K, KG, nm, amg=amg, constrained=constrained, tol=bs['tolerance'],
                                                    max_iter=bs['max_iterations'])
        except backend.BackendError as e:
            if 'buckling mode' in str(e):
                raise SolverError(what + ': ' + str(e).split(': ', 1)[-1])
            raise
        finally:
            if amg is not None:
                amg.close()
        st.update(static_ms=1e3 * (t1 - t0), assembly_ms=1e3 * (t2 - t1), amg_setup_ms=1e3 * (t3 - t2))
        self.buckling_stats = st
        if st['n_converged'] < nm:
            raise SolverError('solve_buckling: {} of {} modes converged in {} iterations (largest relative residual {:.3e})'.format(
                st['n_converged'], nm, st['iterations'], st['max_rel_residual']))
        self.buckling_factors = np.asarray(lam, dtype=np.float64)
        self.buckling_modes = []
        for x in modes:
            xh = x.get()[:V.n_owned]
            f = Function(self.function_space)
            f.vector().set_local(xh / xh[np.argmax(np.abs(xh))])
            self.buckling_modes.append(f)
        self.logger.info('solve_buckling: %d factors in %d iterations, %.1f ms: %s', nm, st['iterations'], st['solve_ms'],
                         np.array2string(self.buckling_factors, precision=6))
        return self.buckling_modes[0]

    def get_flux(self, u, mag_vector):
        return mag_vector

    # ------------------------------------------------------------------ boundary conditions
    def _facet_normals(self, marker_id):
        """Outward unit normals and areas (lengths in 2-D) of the facets carrying marker_id."""
        return self._normals_of_facets(self.boundary_facets.where(marker_id))

    def _normals_of_facets(self, sel):
        """(vertex lists, outward unit normals, areas) of the boundary facets mesh.facets()[sel]."""
        mesh = self.mesh
        tri = mesh.facets()[sel].astype(np.int64)
        co = mesh.coordinates()
        p = co[tri]
        if tri.shape[1] == 2:          # boundary edges of a triangular mesh: the tangent turned by -90 degrees
            t = p[:, 1] - p[:, 0]
            n = np.stack([t[:, 1], -t[:, 0]], axis=1)
        else:
            n = 0.5 * np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])
        area = np.linalg.norm(n, axis=1)
        # orient away from the interior: use the centroid of the (single) adjacent cell
        cf = mesh.cell_facets()
        cells = mesh.cells().astype(np.int64)
        owner = np.full(mesh.num_facets(), -1, dtype=np.int64)
        owner[cf.ravel()] = np.repeat(np.arange(len(cells)), cells.shape[1])
        cc = co[cells[owner[sel]]].mean(axis=1)
        flip = np.einsum("fi,fi->f", n, p.mean(axis=1) - cc) < 0
        n[flip] *= -1.0
        return tri, n / area[:, None], area

    # int phi_node lambda_b ds / |F| on a boundary facet: P2 nodes (vertices, then edge mid-points) against the P1 weights
    _W_TRI_P2 = np.array([[1 / 30 if b == v else -1 / 60 for b in range(3)] for v in range(3)] +
                         [[2 / 15 if b in e else 1 / 15 for b in range(3)] for e in ((0, 1), (0, 2), (1, 2))])
    _W_SEG_P2 = np.array([[1 / 6, 0.0], [0.0, 1 / 6], [1 / 3, 1 / 3]])

    def _varying_pressure_load(self, marker_id, pval, direction, name):
        from .fem import nodal_values, FunctionSpace
        V = self.function_space
        tri, nrm, area = self._facet_normals(marker_id)
        if direction:
            nrm = np.tile(self._vector_of(direction, name), (len(tri), 1))
        pv = nodal_values(pval, FunctionSpace(self.mesh, 'P', 1))[tri]              # [nf, d]: p at the facet's vertices
        d = tri.shape[1]
        nv = self.mesh.num_vertices()
        if V.degree() == 1:
            nodes = tri
            w = (pv.sum(axis=1, keepdims=True) + pv) / (d * (d + 1.0))              # [nf, d]
        else:
            ed = V.edge_nodes().astype(np.int64)
            ekey = ed[:, 0] * nv + ed[:, 1]
            sorter = np.argsort(ekey)
            pairs = ((0, 1), (0, 2), (1, 2)) if d == 3 else ((0, 1),)
            enodes = []
            for a, b in pairs:
                lo, hi = np.minimum(tri[:, a], tri[:, b]), np.maximum(tri[:, a], tri[:, b])
                enodes.append(nv + sorter[np.searchsorted(ekey[sorter], lo * nv + hi)])
            nodes = np.concatenate([tri, np.stack(enodes, axis=1)], axis=1)         # [nf, 6] or [nf, 3]
            w = pv @ (self._W_TRI_P2 if d == 3 else self._W_SEG_P2).T               # [nf, n_nodes]
        loads = self.load_sign_for_tractions() * area[:, None, None] * w[:, :, None] * nrm[:, None, :]     # [nf, nn, dim]
        dofs = nodes[:, :, None] * self.dimension + np.arange(self.dimension)[None, None, :]
        return forms.NodalLoad(dofs, loads, 'pressure(field) ds(%d)' % marker_id)

    def load_sign_for_tractions(self):
        return -1.0 if self.reference_load_sign else 1.0

    def _total_area(self, tri, area):
        """assemble(Constant(1)*ds(id)): on a distributed mesh every facet is counted once - by the rank owning its vertex
        of smallest global id - and the ranks' sums are added."""
        mesh = self.mesh
        if not (hasattr(mesh, 'is_distributed') and mesh.is_distributed()):
            return float(area.sum())
        from . import backend
        gid = mesh.global_vertex_ids()[tri]
        first = np.take_along_axis(tri, np.argmin(gid, axis=1)[:, None], axis=1)[:, 0]
        mine = first < mesh.num_owned_vertices()
        return float(backend.comm_allreduce_sum([float(area[mine].sum())])[0])

    def _vector_of(self, value, what):
        if isinstance(value, Constant):
            v = value.values()
        elif isinstance(value, (tuple, list, np.ndarray)):
            v = np.asarray(value, dtype=np.float64)
        else:
            raise SolverError('{}: a constant vector is required, got {}'.format(what, type(value)))
        if v.size != self.dimension:
            raise SolverError('{}: vector of size {} in a {}D problem'.format(what, v.size, self.dimension))
        return v

    def update_boundary_conditions(self, time_iter_, u, v, ds):
        V = self.function_space
        bcs = []
        integrals_N = []
        sides = []
        if 'point_source' in self.settings and self.settings['point_source']:
            # The reference reads the WRONG key here - settings['surface_source'] (LinearElasticitySolver.py:105-108) - and appends that
            # dict to the Dirichlet list, which assemble_system (:643-650 of SolverBase.py) then rejects: no elasticity case with a
            # point_source runs upstream.  Kept as an error ("refusals"); a point load is a 'force' boundary
            # condition on a small marked facet patch, or a PointSource of the scalar solver for scalar problems.
            raise SolverError("point_source is not supported by LinearElasticitySolver (the reference's own branch reads "
                              "settings['surface_source'] and fails in assemble_system); use a 'force' boundary condition")
        if 'surface_source' in self.settings and self.settings['surface_source']:
            raise SolverError('surface_source is not supported')

        for name, bc_settings in self.boundary_conditions.items():
            i = bc_settings['boundary_id']
            bc = self.get_boundary_variable(bc_settings)
            btype = bc['type']
            if btype == 'Dirichlet' or btype == 'displacement':
                bv = bc['value']
                if isinstance(bv, (tuple, list)) and len(bv) == self.dimension and \
                        any(c is None or isinstance(c, (Constant, Expression, str)) for c in bv):
                    for axis_i, disp in enumerate(bv):
                        if disp is not None:   # None = free; zero is a constraint
                            val = self.translate_value(disp)
                            bcs.append(DirichletBC(V.sub(axis_i), val, self.boundary_facets, i))
                else:
                    bcs.append(DirichletBC(V, self.translate_value(bv), self.boundary_facets, i))
            elif btype == 'force':
                val = bc['value']
                if isinstance(val, (tuple, list)) and len(val) == self.dimension:
                    # the reference applies a tuple-valued 'force' as a traction density (:166-167)
                    g = self._vector_of(val, name)
                    integrals_N.append(forms.FacetLoad(i, g, 'force(vector density)'))
                elif isinstance(val, Constant) and val.value_size() == self.dimension:
                    # Constant((Fx,Fy,Fz)) as in examples/test_linear_elasticity.py:86: the reference forms
                    # n * (F / area), a vector-vector product UFL rejects; the evident intent - the total
                    # force vector spread over the face - is what is applied here: traction = F / area
                    tri, nrm, area = self._facet_normals(i)
                    bc_area = self._total_area(tri, area)
                    self.logger.info('boundary area (m2) for force boundary is %g', bc_area)
                    integrals_N.append(forms.FacetLoad(i, val.values() / bc_area, 'force(vector / area)'))
                else:
                    bc_force = self.translate_value(val)
                    if not is_constant_value(bc_force):
                        raise SolverError("boundary '{}': force magnitude must be a constant".format(name))
                    tri, nrm, area = self._facet_normals(i)
                    bc_area = self._total_area(tri, area)     # assemble(Constant(1)*ds(id)) (:171)
                    self.logger.info('boundary area (m2) for force boundary is %g', bc_area)
                    gmag = float(bc_force) / bc_area
                    if 'direction' in bc and bc['direction']:
                        integrals_N.append(forms.FacetLoad(i, self._vector_of(bc['direction'], name) * gmag,
                                                           'force(direction)'))
                    else:
                        integrals_N.append(forms.FacetLoad(i, nrm * gmag, 'force(normal)'))
            elif btype == 'pressure':
                pval = self.translate_value(bc['value'])
                if not is_constant_value(pval):
                    # a pressure that varies over the boundary (hydrostatic load on a wall): n * p with p through its P1
                    # interpolant on every facet, integrated exactly against the P1 / P2 test functions
                    integrals_N.append(self._varying_pressure_load(i, pval, bc.get('direction'), name))
                    continue
                if 'direction' in bc and bc['direction']:
                    integrals_N.append(forms.FacetLoad(i, self._vector_of(bc['direction'], name) * float(pval),
                                                       'pressure(direction)'))
                else:
                    tri, nrm, area = self._facet_normals(i)
                    integrals_N.append(forms.FacetLoad(i, nrm * float(pval), 'pressure(normal)'))
            elif btype == 'stress':
                g = self.translate_value(bc['value'])
                if isinstance(g, Constant) and g.value_size() == self.dimension:
                    integrals_N.append(forms.FacetLoad(i, g.values(), 'stress(vector)'))
                elif isinstance(g, Constant) and g.value_size() == self.dimension ** 2:
                    tri, nrm, area = self._facet_normals(i)
                    integrals_N.append(forms.FacetLoad(i, nrm @ g.values().reshape(self.dimension, self.dimension).T, 'stress(tensor.n)'))
                else:
                    raise SolverError("boundary '{}': stress must be a constant vector or tensor".format(name))
            elif btype in ('contact', 'sliding') and self._constraint_sides:
                if not sides:
                    self._refuse_contact_case()
                sides.append((name, i, btype, bc))          # resolved below, once every displacement BC is known
            elif btype == 'Neumann':
                raise SolverError('Neumann boundary type`{}` is not supported'.format(btype))
            elif btype == 'symmetry':
                raise SolverError('symmetry boundary type`{}` is not supported'.format(btype))
            else:
                raise SolverError('boundary type`{}` is not supported'.format(btype))
        self._contact = self._contact_setup(sides, bcs) if sides else None
        return bcs, integrals_N

    # ------------------------------------------------------------------ frictionless contact and sliding supports
    # 'contact': a rigid frictionless obstacle, n.u <= g, lambda >= 0, lambda (g - n.u) = 0 at every node of the marked facets;
    # 'sliding': the bilateral case n.u = value (oblique rollers and symmetry planes).  The five subclasses set this to False and
    # keep refusing both types.
    _constraint_sides = True
    _CONTACT_DEFAULTS = {'max_iterations': 30, 'initial_active': 'all'}

    def contact_settings(self):
        """settings['solver_settings']['contact_settings'] with its defaults, checked (SolverError on a bad value)."""
        given = self.solver_settings.get('contact_settings') or {}
        unknown = set(given) - set(self._CONTACT_DEFAULTS)
        if unknown:
            raise SolverError('contact_settings: unknown key(s) {}'.format(sorted(unknown)))
        cs = dict(self._CONTACT_DEFAULTS, **given)
        mi = cs['max_iterations']
        if isinstance(mi, bool) or not isinstance(mi, numbers.Integral) or mi < 1:
            raise SolverError('contact_settings: max_iterations must be a positive integer, got {!r}'.format(mi))
        if cs['initial_active'] not in ('all', 'none'):
            raise SolverError("contact_settings: initial_active must be 'all' or 'none', got {!r}".format(cs['initial_active']))
        return {'max_iterations': int(mi), 'initial_active': cs['initial_active']}

    def _constraint_side_names(self):
        return [name for name, bc in self.boundary_conditions.items()
                if self.get_boundary_variable(bc).get('type') in ('contact', 'sliding')]

    def _refuse_constraint_sides(self, what):
        names = self._constraint_side_names() if self._constraint_sides else []
        if names:
            raise SolverError("{}: contact / sliding boundary conditions ({}) are not supported - the eigenproblem needs a linear "
                              "constraint set; replace them by displacement BCs on the nodes in contact".format(what, ', '.join(names)))

    def _refuse_contact_case(self):
        """What the contact path is written for: vector CG1, one rank, not periodic, a static case (no device call is made here)."""
        from . import parallel
        self.contact_settings()
        V = self.function_space
        what = 'contact / sliding boundary conditions'
        if V.degree() != 1:
            raise SolverError(what + ': P2 displacement spaces are not supported - the constraint is nodal, on the vertices of the '
                              'marked facets; use a P1 space')
        if parallel.world()[1] > 1 or V.localizer() is not None:
            raise SolverError(what + ' run on one rank')
        if hasattr(V, 'periodic_pairs') and V.periodic_pairs() is not None:
            raise SolverError(what + ' on a periodic space are not supported')
        if self.transient_settings['transient']:
            raise SolverError(what + ': transient_settings must not be transient (the active-set loop solves a static case)')

    def _contact_setup(self, sides, bcs):
        """The constraint nodes of the 'contact' / 'sliding' sides (host only): the vertices of the marked facets, less those that
        carry a displacement BC (Dirichlet wins) or belong to a side listed earlier.  Returns a dict of arrays over the nodes in
        ascending order: nodes, normals [n, d] (unit), values, bilateral, area (lumped area of the marked facets), side (index)."""
        d = self.dimension
        co = self.mesh.coordinates()
        nv = co.shape[0]
        taken = np.zeros(nv, dtype=bool)
        dd = self._bc_arrays(bcs)[0]
        taken[np.unique(dd // d)] = True
        parts = []
        for k, (name, marker, btype, bc) in enumerate(sides):
            sel = self.boundary_facets.where(marker)
            if len(sel) == 0:
                raise SolverError("boundary '{}': no facet carries marker {}".format(name, marker))
            tri, nrm, area = self._normals_of_facets(sel)
            nodes = np.unique(tri)
            lumped = np.zeros(nv)
            np.add.at(lumped, tri.ravel(), np.repeat(area / tri.shape[1], tri.shape[1]))
            if bc.get('normal') is not None:
                n = np.asarray(self._vector_of(bc['normal'], "boundary '{}': normal".format(name)), dtype=np.float64)
                length = np.linalg.norm(n)
                if not np.isfinite(length) or length == 0.0:
                    raise SolverError("boundary '{}': the normal is a zero vector".format(name))
                normals = np.tile(n / length, (len(nodes), 1))
            else:
                acc = np.zeros((nv, d))
                np.add.at(acc, tri.ravel(), np.repeat(nrm * area[:, None], tri.shape[1], axis=0))
                normals = acc[nodes]
                length = np.linalg.norm(normals, axis=1)
                if np.any(length <= 1e-12 * area.max()):
                    raise SolverError("boundary '{}': the facet normals cancel at node {} (a zero normal); give 'normal'".format(
                        name, int(nodes[np.argmin(length)])))
                normals = normals / length[:, None]
            keep = ~taken[nodes]
            dropped = int((~keep).sum())
            if dropped:
                self.logger.info("boundary '%s': %d of %d nodes carry a displacement BC or belong to an earlier constraint side and "
                                 "are dropped", name, dropped, len(nodes))
            if not keep.any():
                raise SolverError("boundary '{}': no candidate node is left (every node of the side carries a displacement BC or "
                                  "belongs to an earlier constraint side)".format(name))
            nodes, normals = nodes[keep], normals[keep]
            taken[nodes] = True
            value = bc.get('value')
            value = 0.0 if value is None else (Expression(value, degree=1) if isinstance(value, str) else value)
            if is_constant_value(value):
                vals = np.full(len(nodes), float(value))
            elif isinstance(value, (Expression, UserExpression)):
                vals = np.asarray(value.eval_points(co[nodes]), dtype=np.float64).reshape(len(nodes), -1)[:, 0]
            else:
                raise SolverError("boundary '{}': value must be a number, a Constant, an Expression or a str".format(name))
            if not np.all(np.isfinite(vals)):
                raise SolverError("boundary '{}': the value is not finite at node {}".format(name, int(nodes[np.argmin(np.isfinite(vals))])))
            parts.append((nodes, normals, vals, np.full(len(nodes), btype == 'sliding'), lumped[nodes], np.full(len(nodes), k)))
        cat = [np.concatenate([p[j] for p in parts]) for j in range(6)]
        order = np.argsort(cat[0], kind='stable')
        keys = ('nodes', 'normals', 'values', 'bilateral', 'area', 'side')
        out = {key: a[order] for key, a in zip(keys, cat)}
        out['names'] = [s[0] for s in sides]
        return out

    def solve_contact(self, F, u, bcs):
        """The static solve with 'contact' / 'sliding' sides, by the primal-dual active-set strategy in per-node frames: K' = H K H and
        b' = H b are built once (fs_matrix_rotate_nodes); every active set is a component Dirichlet condition on a copy of K' (the
        user's Dirichlet dofs with the active normal dofs), solved by AMG-CG (3-D; the rigid-body modes rotated by H as near-null
        space, a hierarchy per active set) or Jacobi-CG (2-D), warm-started; fs_contact_update gives lambda, the penetration and the
        next set; the loop ends when no flag changes.  Only sliding sides: one solve.  u = H u' on the way out."""
        import time
        from . import backend
        cs = self.contact_settings()
        C_ = self._contact
        d = self.dimension
        V = F.space.device()
        rtol, max_iter, pc = self._krylov_options()
        sp_ = self.solver_settings.get('solver_parameters', {}) or {}
        use_amg = d == 3 and (pc == 'amg' or 'preconditioner' not in sp_)
        norm = sp_.get('norm_type', 'preconditioned' if pc != 'none' or use_amg else 'unpreconditioned')
        phases = {'assembly_ms': 0.0, 'copy_dirichlet_ms': [], 'amg_setup_ms': [], 'cg_ms': [], 'update_ms': []}

        def lap(t0):
            backend.synchronize()
            return 1e3 * (time.perf_counter() - t0)
        t0 = time.perf_counter()
        K, b = self.assemble_system(F, [])
        first = np.ones(len(C_['nodes']), dtype=np.int32) if cs['initial_active'] == 'all' else C_['bilateral'].astype(np.int32)
        frames = backend.ContactFrames(V, C_['nodes'], C_['normals'], C_['values'], C_['bilateral'], first)
        K.rotate_nodes(frames)
        b.rotate_nodes(frames)
        ns = None
        if use_amg:
            ns = []
            for mode in self.build_nullspace(F.space):
                mv = backend.DeviceVector(V.n_owned, mode)
                mv.rotate_nodes(frames)
                ns.append(mv.get())
                mv.close()
            ns = np.stack(ns)
        x = backend.DeviceVector(V.n_local)
        u0 = u.vector()._values()
        warm = bool(np.any(u0 != 0.0))
        if warm:
            x.set(np.concatenate([u0, np.zeros(V.n_local - u0.size)]))
            x.rotate_nodes(frames)
        Kc = backend.DeviceMatrix(V)
        bc_ = backend.DeviceVector(V.n_owned)
        phases['assembly_ms'] = lap(t0)
        user_dofs, user_vals = self._bc_arrays(bcs)
        target = frames.sigma * frames.values                 # u'[d a + k] = sigma n . u on an active node
        active = first.astype(bool)
        history, cg_iterations, seen = [int(active.sum())], [], {active.tobytes()}
        amg_setups = 0
        for outer in range(1, cs['max_iterations'] + 1):
            t0 = time.perf_counter()
            Kc.copy_from(K)
            bc_.copy_from(b)
            dofs = np.concatenate([user_dofs, frames.normal_dofs[active]]).astype(np.int32)
            vals = np.concatenate([user_vals, target[active]])
            if dofs.size:
                Kc.apply_dirichlet(bc_, dofs, vals, symmetric=True)
                backend.set_dirichlet_values(x, dofs, vals)
            phases['copy_dirichlet_ms'].append(lap(t0))
            t0 = time.perf_counter()
            if use_amg:
                hierarchy = backend.AMG(Kc, nullspace=ns, strength_threshold=float(sp_.get('amg_strength_threshold', 0.0)))
                amg_setups += 1
                phases['amg_setup_ms'].append(lap(t0))
                t0 = time.perf_counter()
                try:
                    st = hierarchy.solve(bc_, x, rtol=rtol, max_iter=min(max_iter, int(sp_.get('maximum_iterations', 500))),
                                         nonzero_guess=True, norm=norm)
                finally:
                    hierarchy.close()
            else:
                phases['amg_setup_ms'].append(0.0)
                st = backend.krylov_solve(Kc, bc_, x, rtol=rtol, max_iter=max_iter, precond='none' if pc == 'none' else 'jacobi',
                                          method='cg', nonzero_guess=True, norm=norm)
            phases['cg_ms'].append(lap(t0))
            self.last_solve_stats = st
            cg_iterations.append(int(st['iterations']))
            if st['converged'] != 1:
                user_tol = 'krylov_relative_tolerance' in sp_ or float(sp_.get('relative_tolerance', 1.0)) < 1e-8
                if user_tol or st['converged'] < 0 or not (st['true_rel_residual'] <= 1e-8):
                    raise SolverError('solve_contact: Krylov solver did not converge in {} iterations (||r||/||b|| = {:.3e}) on active '
                                      'set {} (active counts {})'.format(st['iterations'], st['true_rel_residual'], outer, history))
                self.logger.warning('solve_contact: stopped at ||r||/||b|| = %.3e after %d iterations (default tolerance %.0e not attained)',
                                    st['true_rel_residual'], st['iterations'], rtol)
            t0 = time.perf_counter()
            changed, n_active = backend.contact_update(frames, K, x, b)
            phases['update_ms'].append(lap(t0))
            if changed == 0:
                break
            active = frames.get()[0]
            history.append(n_active)
            key = active.tobytes()
            if key in seen:
                raise SolverError('solve_contact: the active set of iteration {} repeats an earlier one - the active-set strategy cycles '
                                  '(active counts {})'.format(outer + 1, history))
            seen.add(key)
        else:
            raise SolverError('solve_contact: no fixed active set within max_iterations = {} (active counts {})'.format(
                cs['max_iterations'], history))
        act, lam, pen = frames.get()
        x.rotate_nodes(frames)
        u.vector()._adopt_device(x)
        for h in (Kc, K, bc_, b):
            h.close()
        frames.close()
        self._contact_result = {'nodes': C_['nodes'].copy(), 'active': act, 'lambda': lam, 'gap': -pen, 'area': C_['area'],
                                'bilateral': C_['bilateral'].copy(), 'normals': C_['normals'].copy(), 'values': C_['values'].copy()}
        self.contact_stats = dict(phases, outer_iterations=outer, active_history=history, cg_iterations=cg_iterations, amg_setups=amg_setups)
        self.logger.info('solve_contact: %d active-set iteration(s), active counts %s, CG iterations %s', outer, history, cg_iterations)
        return u

    def _contact_solved(self):
        res = getattr(self, '_contact_result', None)
        if res is None:
            raise SolverError('no contact result: solve() a case with a contact or sliding boundary condition first')
        return res

    def contact_forces(self):
        """(node ids, lambda) after a solve: the normal force in N that the obstacle (or the sliding support, where it may have either
        sign) exerts on every constraint node, against its normal; zero on nodes that are not in contact."""
        res = self._contact_solved()
        return res['nodes'].copy(), np.where(res['active'], res['lambda'], 0.0)

    def contact_pressure(self):
        """The contact pressure as a P1 scalar Function: lambda over the lumped area of the marked facets at the node, zero elsewhere."""
        from .fem import FunctionSpace
        res = self._contact_solved()
        f = Function(FunctionSpace(self.mesh, 'P', 1))
        p = np.zeros(self.mesh.num_vertices())
        p[res['nodes']] = np.where(res['active'], res['lambda'], 0.0) / res['area']
        f.vector().set_local(p)
        return f

    def contact_status(self):
        """(node ids, active flags, gaps g - n.u) after a solve."""
        res = self._contact_solved()
        return res['nodes'].copy(), res['active'].copy(), res['gap'].copy()

    @staticmethod
    def _try_values(val):
        if isinstance(val, Constant):
            return val.values()
        try:
            return np.asarray(val, dtype=np.float64)
        except (TypeError, ValueError):
            return np.zeros(0)

    # ------------------------------------------------------------------ the form
    def generate_form(self, time_iter_, u, v, u_current, u_prev):
        F = forms.ElasticityForm(self.function_space)
        aniso = self.anisotropic_material()
        if aniso is not None:
            self._refuse_anisotropic_case()
        if self.transient_settings['transient'] and self.solving_dynamics and time_iter_ >= 1:
            # F -= density * inner(accel, v) * dx (:216-220) with the explicit acceleration of SolverBase.get_acceleration
            rho = self.material_field('density')
            F.inertia = (float(rho) if np.ndim(rho) == 0 else ('cell', rho), self.get_acceleration(time_iter_))
        if aniso is None:
            F.mu, F.lmbda = self.lame_parameters()
        F.load_sign = -1.0 if self.reference_load_sign else 1.0

        bcs, integrals_F = self.update_boundary_conditions(time_iter_, u, v, Measure("ds", subdomain_data=self.boundary_facets))
        F.tractions.extend(integrals_F)

        if self.body_source:
            self._set_body_force(F)

        if not hasattr(self, 'temperature_distribution'):
            if 'temperature_distribution' in self.settings and self.settings['temperature_distribution']:
                self.temperature_distribution = self.translate_value(self.settings['temperature_distribution'])
        if hasattr(self, 'temperature_distribution') and self.temperature_distribution:
            T = self.temperature_distribution
            T_ref = float(self.reference_values['temperature'])
            if is_constant_value(T):
                Tval = float(T)
            else:
                from .fem import FunctionSpace
                nod = nodal_values(T, FunctionSpace(self.mesh, 'P', 1))
                Tval = float(nod[0]) if np.ptp(nod) == 0.0 else nod
            if aniso is None:
                F.thermal = (self.thermal_stress_coefficient(), Tval, T_ref)
            else:
                # eps* per unit temperature in global axes: R alpha R^T, alpha given in material axes
                alpha = self._expansion_tensors()
                if aniso.frames is not None:
                    alpha = np.einsum('cik,ckl,cjl->cij', aniso.frames, alpha, aniso.frames)
                if self.dimension == 2 and max(np.abs(alpha[:, 0, 2]).max(), np.abs(alpha[:, 1, 2]).max()) > 1e-12 * np.abs(alpha).max():
                    raise SolverError("material 'thermal_expansion_coefficient': plane strain needs an expansion tensor without "
                                      "xz / yz components")
                aniso = forms.AnisotropicElasticity(aniso.table, aniso.index, aniso.frames,
                                                    thermal=(self._tensor_storage(alpha, self.dimension), Tval, T_ref))
        F.anisotropic = aniso
        return F, bcs

    def _set_body_force(self, F):
        """F.body_force (a constant vector) or F.body_force_nodal (a field) from self.body_source."""
        bs = self.body_source
        if isinstance(bs, Expression):
            vals = bs.eval_points(self.mesh.coordinates()[:1])   # constant body force expected
            allv = bs.eval_points(self.mesh.coordinates())
            if np.abs(allv - vals).max() > 1e-12 * max(1.0, np.abs(allv).max()):
                # a field (e.g. a centrifugal load): its interpolant in the displacement space, integrated with the
                # consistent mass matrix - what FFC's quadrature gives for an Expression of the element's degree
                F.body_force_nodal = bs.eval_points(self.function_space.node_coordinates())[:, :self.dimension]
                F.body_force = None
            else:
                F.body_force = tuple(float(x) for x in vals[0])
        else:
            F.body_force = tuple(float(x) for x in self._vector_of(bs, 'body_source'))

    def solve_form(self, F, u_, bcs):
        if getattr(self, '_contact', None) is not None:
            return self.solve_contact(F, u_, bcs)
        if self.dimension == 3:
            u_ = self.solve_amg(F, u_, bcs)
        else:
            u_ = self.solve_linear_problem(F, u_, bcs)
        return u_

    def displacement(self):
        if self.is_mixed_function_space:
            raise SolverError('subclass with mixed_function_space must override this function')
        return self.w_current

    def velocity(self):
        dt = self.get_time_step(self.current_step)
        out = Function(self.function_space)
        out.vector().set_local((self.w_current.vector()._values() - self.w_prev.vector()._values()) / dt)
        return out

    def solve_modal(self):
        """Modal analysis of the case (LinearElasticitySolver.py:270-281): the form of step 0, then solve_modal_form."""
        self.modal_settings()
        self._refuse_constraint_sides('solve_modal')
        self.init_solver()
        F, bcs = self.generate_form(0, None, None, self.w_current, self.w_prev)
        return self.solve_modal_form(F, bcs)
