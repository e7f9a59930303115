"""The row-length-dependent paths of the symbolic phase and of the assembly, on meshes with ONE long row (tests/hub_meshes.py), against
oracle/fem_oracle.py.  What depends on the longest row of a space (fs_space_s::max_row) or on the cells around a node:

    k_row_columns<32, 256> / <160, 64>   more than 32 (CG1) / 160 (CG2) columns in a row: the pattern comes from the sorted keys
    k_inc_fill                           stored width <= 16, <= 32, beyond: positions from 16 / 32 registers or by search in memory
    make_row_gather_shape                max_row <= 32: workgroups of 256 threads, <= 128: of 64, beyond: the row-gather kernels refuse
    fs_space_create step 5a / 5b         incidence tables up to 255 entries (CG1 on tetrahedra: up to 128, beyond that the slot table
                                         and the atomic k_assemble_p1_scalar)
    gather lists, *_load kernels         loops over the cells of an entry or a node

Every hub size is the one just below or just above one of these limits; the hub sits on row 63 (last lane of a slice), and for one
size per family on rows 0, 64 and the last one too.

Bounds.  Matrix and load-vector entries: |got - ref| <= RTOL_ASSEMBLY max|ref| as elsewhere in the suite, and ENTRY BY ENTRY
|got - ref| <= RTOL_ASSEMBLY sum_cells |local entry| + own (the oracle assembles the absolute local matrices): 1e-12 is 4 500 eps,
which covers the 516-term sum of the largest hub and the rounding of the geometry, and a dropped or doubled contribution at the hub
is at least 1 / 516 of that sum.  `own` is the oracle's own rounding.  Thousands of entries vanish by cancellation INSIDE a local
matrix (orthogonal gradients, mixed components of an axis-aligned cell, the vertex functions of a CG2 source): there the absolute
local entries are themselves rounding noise (or exactly 0 where the kernel leaves 1e-19) and their sum says nothing about the
error of either side: without `own` the kernels sit at up to 2e14 times (and at "inf" times) that bound at such entries, with the
largest error of every form below 2e-15 max|ref|.  The yardstick is measured on the oracle alone: the same form over the same
cells with their vertices in the opposite order (the same numbers up to rounding; the local matrices behind it come from
numpy's LAPACK inverses, which have no extended-precision form), the largest distance between the two assembled results, times 8
for the kernel's different order of operations.  It is asserted to stay below OWN_MAX = 256 eps max|ref| (1 / 17 of the first
bound, far below any single contribution at the hub), so that a twin that is not the same form cannot make the entry check
vacuous.  Measured on the MI355X: own 1 to 122 eps max|ref|; largest error 0.25 of the entry bound, 0.018 of the matrix bound,
at the cancelling entries 0.25 of `own`.
Products: row_length eps (|A| |x|)_row against the extended-precision host product of the assembled matrix - the bound of any
order of summation.  Solves: RTOL_SOLUTION max|u| against a direct solve.

Every entry point either returns values within these bounds or raises BackendError naming the row length and the limit, and
which of the two it does at which length is pinned (_limit: the table of DESIGN.md section 2); what works at one row length works
at every shorter one (test_supported_row_lengths_are_monotone)."""
import re

import numpy as np
import pytest
import scipy.sparse as sp

import hub_meshes as hm
from oracle import fem_oracle as fo
from spmv_reference import EPS, _host_product

pytestmark = pytest.mark.gpu

RTOL_ASSEMBLY = 1e-12   # relative to max |A_ij| and to the sum of the absolute contributions of an entry
RTOL_SOLUTION = 1e-9    # relative to max |u|
VEL = np.array([0.6, -0.3, 0.2])
PE, K0, M0 = 2.0, 1.7, 0.9
MAT1, MAT2 = (3.0e3, 0.3), (1.1e3, 0.22)          # (E, nu) of the two materials of the per-cell Lame form
BODY = np.array([0.3, -9.81, 0.5])

OWN_MAX = 256.0         # ceiling of the oracle's own rounding (8 x the distance between its two evaluations), in eps max|ref|
GATHER_MAX_ROW, TABLE_MAX_ROW = 128, 255          # FS_GATHER_MAX_ROW, FS_TABLE_MAX_ROW of fs_common.h
_cases, _runs = {}, {}


# ---------------------------------------------------------------------------------------------------------------- references
class _Case:
    """mesh and dof tables of one (family, size, hub row)"""

    def __init__(self, family, size, hub_row, reverse=False):
        gen, self.degree, _, _ = hm.FAMILIES[family]
        self.family, self.size = family, size
        self.co, self.ce, self.row = hm.build(family, size, hub_row)
        if reverse:         # the same cells with their vertices in descending order: the same forms, rounded differently
            self.ce = np.ascontiguousarray(self.ce[:, ::-1])
        else:
            self.twin = _Case(family, size, hub_row, True)
        self.tdim = self.co.shape[1]
        nv = len(self.co)
        if self.degree == 1:
            self.cd, self.edges, self.x = self.ce.astype(np.int64), None, self.co
        else:
            cd, self.edges = (fo.p2_cell_dofs if self.tdim == 3 else fo.tri_p2_cell_dofs)(nv, self.ce)
            self.cd, self.x = cd.astype(np.int64), fo.p2_dof_coordinates(self.co, self.edges)
        self.n = len(self.x)
        self.hub_len = hm.hub_row_length(gen, self.degree, size)
        assert hm.row_lengths(self.n, self.cd)[self.row] == self.hub_len
        self.vel = VEL if self.tdim == 3 else VEL * np.array([1.0, 1.0, 0.0])
        self.region = np.random.default_rng(3).random(len(self.ce)) < 0.5

    def size_and_grads(self):
        if self.tdim == 3:
            detJ, g = fo.p1_geometry(self.co, self.ce)
            return np.abs(detJ) / 6.0, g
        return fo.tri_geometry(self.co, self.ce)

    def boundary_nodes(self):
        nv = len(self.co)
        if self.tdim == 3:
            facets, _, cnt = fo.facet_numbering(self.ce)
            if self.degree == 1:
                return np.unique(facets[cnt == 1].ravel()).astype(np.int64)
            return fo.p2_facet_dofs(nv, self.edges, facets, (cnt == 1).astype(int), 1).astype(np.int64)
        edges, _, cnt = fo.tri_edge_numbering(self.ce)
        if self.degree == 1:
            return np.unique(edges[cnt == 1].ravel()).astype(np.int64)
        return np.unique(fo.tri_p2_edge_nodes(nv, self.edges, edges[cnt == 1]).ravel()).astype(np.int64)


def _case(family, size, hub_row):
    key = (family, size, hub_row)
    if key not in _cases:
        _cases[key] = _Case(*key)
    return _cases[key]


def _scalar_matrix_forms(c):
    """name -> (keywords of DeviceMatrix.assemble, local matrices [n_cells, nd, nd])"""
    co, ce, d = c.co, c.ce, c.tdim
    if c.degree == 2:
        loc = lambda pe, scale, mass: fo.p2_supg_system_local(co, ce, c.vel[:d], pe, K0, scale, mass)
        km, ka, kas = loc(None, 0.0, M0), loc(None, 1.0, 0.0), loc(PE, 1.0, 0.0)
    elif d == 3:
        K = fo.p1_stiffness_local(co, ce, K0)
        km = K + fo.p1_mass_local(co, ce, M0)
        ka = K + fo.p1_advection_local(co, ce, c.vel, 1.0)
        kas = ka + fo.p1_supg_local(co, ce, c.vel, PE, 1.0, 0.0)
    else:
        K = fo.tri_stiffness_local(co, ce, K0)
        km = K + fo.tri_mass_local(co, ce, M0)
        ka = K + fo.tri_advection_local(co, ce, c.vel[:2], 1.0)
        kas = ka + fo.tri_supg_local(co, ce, c.vel, PE, 1.0, 0.0)
    return {"stiffness+mass": (dict(stiffness=K0, mass=M0), km),
            "stiffness+advection": (dict(stiffness=K0, advection=tuple(c.vel)), ka),
            "stiffness+advection+supg": (dict(stiffness=K0, advection=tuple(c.vel), supg_pe=PE), kas)}


def _mass_locals(c, coef):
    co, ce = c.co, c.ce
    if c.degree == 2:
        return (fo.p2_mass_local if c.tdim == 3 else fo.tri_p2_mass_local)(co, ce, coef)
    return (fo.p1_mass_local if c.tdim == 3 else fo.tri_mass_local)(co, ce, coef)


def _source_locals(c):
    """int phi_a dx of every cell [n_cells, nd]"""
    size, _ = c.size_and_grads()
    if c.degree == 2:
        return (fo.p2_source_local if c.tdim == 3 else fo.tri_p2_source_local)(c.co, c.ce, 1.0)
    return np.repeat((size / (c.tdim + 1.0))[:, None], c.tdim + 1, axis=1)


def _vector_matrix_forms(c):
    co, ce, d = c.co, c.ce, c.tdim
    el = {(3, 1): fo.p1_elasticity_local, (2, 1): fo.tri_elasticity_local, (3, 2): fo.p2_elasticity_local,
          (2, 2): fo.tri_p2_elasticity_local}[(d, c.degree)]
    nd = c.cd.shape[1]
    Mv = np.einsum("cab,ij->caibj", _mass_locals(c, M0), np.eye(d)).reshape(len(ce), nd * d, nd * d)
    K1, K2 = el(co, ce, *MAT1), el(co, ce, *MAT2)
    pairs = np.where(c.region[:, None], np.array(fo.lame(*MAT1))[None, :], np.array(fo.lame(*MAT2))[None, :])
    return {"lame+mass": (dict(lame=fo.lame(*MAT1), mass=M0), K1 + Mv),
            "cell lame+mass": (dict(lame=("cell", pairs), mass=M0), np.where(c.region[:, None, None], K1, K2) + Mv)}


def _scalar_load_forms(c):
    """name -> (keywords of assemble_vector, local vectors [n_cells, nd])"""
    co, ce, d = c.co, c.ce, c.tdim
    src = _source_locals(c)
    fn = 2.0 + np.sin(3.0 * c.x[:, 0]) + c.x[:, 1]
    fc = np.random.default_rng(5).uniform(1.0, 2.0, len(ce))
    if c.degree == 2:
        supg = fo.p2_supg_source_local(co, ce, c.vel[:d], PE, fc)
    else:
        size, _ = c.size_and_grads()
        w = (fo.supg_weights(co, ce, c.vel, PE) if d == 3 else fo.tri_supg_weights(co, ce, c.vel, PE))[0]
        supg = fc[:, None] * src + w * (fc * size)[:, None]
        whole = (fo.assemble_p1_source(co, ce, fc) + fo.assemble_p1_supg_source(co, ce, c.vel, PE, fc)) if d == 3 else \
            (fo.assemble_tri_source(co, ce, fc) + fo.assemble_tri_supg_source(co, ce, c.vel, PE, fc))
        assert np.abs(fo.assemble_generic_vector(c.n, c.cd, supg) - whole).max() <= 1e-14 * np.abs(whole).max()
    return {"constant source": (dict(source=2.5), 2.5 * src),
            "nodal source": (dict(source=("nodal", fn)), np.einsum("cab,cb->ca", _mass_locals(c, 1.0), fn[c.cd])),
            "supg source": (dict(source=("cell", fc), supg=(tuple(c.vel), PE)), supg)}


def _vector_load_forms(c):
    d = c.tdim
    return {"body force": (dict(vector_value=tuple(BODY[:d])), (_source_locals(c)[:, :, None] * BODY[None, None, :d]).reshape(len(c.ce), -1))}


def _vector_dofs(cd, d):
    return (cd[:, :, None] * d + np.arange(d)[None, None, :]).reshape(len(cd), -1)


def _sum_and_abs(n, cd, loc, cd2, loc2):
    """The assembled local contributions (ref), the assembled absolute contributions, and the oracle's own rounding: 8 x the largest
    distance of ref from the same sum over the twin case (cells with their vertices in the opposite order - the same numbers up to
    rounding).  Matrices: CSR with the full pattern."""
    if loc.ndim == 3:
        ref, other = fo.assemble_generic(n, cd, loc), fo.assemble_generic(n, cd2, loc2)
        assert np.array_equal(ref.indptr, other.indptr) and np.array_equal(ref.indices, other.indices)
        return ref, fo.assemble_generic(n, cd, np.abs(loc)), 8.0 * np.abs(ref.data - other.data).max()
    ref = fo.assemble_generic_vector(n, cd, loc)
    return ref, fo.assemble_generic_vector(n, cd, np.abs(loc)), 8.0 * np.abs(ref - fo.assemble_generic_vector(n, cd2, loc2)).max()


# ---------------------------------------------------------------------------------------------------------------- one case
def _within(got, ref, ref_abs, own):
    """(largest error / (RTOL_ASSEMBLY max|ref|), largest entry error / (RTOL_ASSEMBLY sum of absolute contributions + own),
    largest entry error / (own / 8) where the absolute contributions alone do not cover it, own / (eps max|ref|))"""
    err = np.abs(got - ref)
    with np.errstate(divide="ignore", invalid="ignore"):
        entry = np.where(err > 0.0, err / (RTOL_ASSEMBLY * ref_abs + own), 0.0)
        cancelling = np.where(err > RTOL_ASSEMBLY * ref_abs, err / own, 0.0)
    return float(err.max() / (RTOL_ASSEMBLY * np.abs(ref).max())), float(entry.max()), float(8.0 * cancelling.max()), float(own / (EPS * np.abs(ref).max()))


def _csr(A):
    rp, ci, va, shape = A.to_csr()
    return sp.csr_matrix((va, ci, rp), shape=shape)


def _table_max(c):
    """longest row up to which the scalar space of the case keeps its incidence tables"""
    return GATHER_MAX_ROW if c.family == "cg1_tet" else TABLE_MAX_ROW


def _limit(c, what):
    """Longest row at which the entry point gives values (None: any length): the table of DESIGN.md, section 2."""
    if what.startswith("vector "):
        return None                                      # slot table and gather lists: no LDS or table limit
    if "matrix:" in what:                                # the row-gather kernels; CG1 on tetrahedra has the atomic kernel beyond
        return None if (c.family == "cg1_tet" and what.endswith(":stiffness+mass")) else GATHER_MAX_ROW
    if c.family == "cg2_tri" or (c.degree == 2 and what.endswith(":supg source")):
        return TABLE_MAX_ROW                             # these load kernels walk the tables; the others have an atomic form
    return None


def _refusal(c, e, what):
    """a refusal names the row length and the limit that was passed: the tables' where the space has none, else the gather kernels'"""
    named = _table_max(c) if (c.hub_len > _table_max(c) or " load:" in what) else GATHER_MAX_ROW
    ok = re.search(r"\b%d entries" % c.hub_len, str(e)) and re.search(r"\b%d\b" % named, str(e))
    return [] if ok else ["%s refused without naming the %d entries of the longest row and the limit %d: %s" % (what, c.hub_len, named, e)]


def _run_space(gpu, c, vector, out, bad, figures):
    d = c.tdim
    ncomp = d if vector else 1
    tag = "vector" if vector else "scalar"
    mesh = gpu.DeviceMesh(c.co, c.ce)
    V = gpu.DeviceSpace(mesh, ncomp=ncomp, degree=c.degree)
    cd = _vector_dofs(c.cd, d) if vector else c.cd
    cd2 = _vector_dofs(c.twin.cd, d) if vector else c.twin.cd
    n = c.n * ncomp
    if V.n_owned != n:
        bad.append("%s space: %d dofs, expected %d" % (tag, V.n_owned, n))
        return
    if c.degree == 2 and not np.array_equal(V.edges(), c.edges):
        bad.append("%s space: the edge nodes are not the oracle's" % tag)
        return
    rp_ref, ci_ref = fo.csr_pattern(c.n, c.cd, ncomp)
    assembled = {}
    forms = _vector_matrix_forms if vector else _scalar_matrix_forms
    twin_forms = forms(c.twin)
    for name, (kw, loc) in forms(c).items():
        what = "%s matrix:%s" % (tag, name)
        A = gpu.DeviceMatrix(V)
        try:
            A.assemble(**kw)
        except gpu.BackendError as e:
            out[what] = "refused"
            bad += _refusal(c, e, what)
            continue
        out[what] = "values"
        rp, ci, va, _ = A.to_csr()
        if not (np.array_equal(rp, rp_ref) and np.array_equal(ci, ci_ref)):
            bad.append("%s: the pattern is not the oracle's" % what)
            continue
        ref, ref_abs, own = _sum_and_abs(n, cd, loc, cd2, twin_forms[name][1])
        assert np.array_equal(ref.indptr, rp_ref) and np.array_equal(ref.indices, ci_ref)
        f = _within(va, ref.data, ref_abs.data, own)
        figures.append((what, f))
        if not 0.0 < f[3] <= OWN_MAX:
            bad.append("%s: the oracle's two evaluations differ by %.3g eps max|ref| (x 8)" % (what, f[3]))
        if max(f[:2]) > 1.0:
            bad.append("%s: error %.3g of the matrix bound, %.3g of the entry bound" % ((what,) + f[:2]))
        assembled[name] = (A, ref)
    loads = _vector_load_forms if vector else _scalar_load_forms
    twin_loads = loads(c.twin)
    load_ref = None
    for name, (kw, loc) in loads(c).items():
        what = "%s load:%s" % (tag, name)
        b = gpu.DeviceVector(n)
        try:
            gpu.assemble_vector(V, b, **kw)
        except gpu.BackendError as e:
            out[what] = "refused"
            bad += _refusal(c, e, what)
            continue
        out[what] = "values"
        ref, ref_abs, own = _sum_and_abs(n, cd, loc, cd2, twin_loads[name][1])
        f = _within(b.get(), ref, ref_abs, own)
        figures.append((what, f))
        if not 0.0 < f[3] <= OWN_MAX:
            bad.append("%s: the oracle's two evaluations differ by %.3g eps max|ref| (x 8)" % (what, f[3]))
        if max(f[:2]) > 1.0:
            bad.append("%s: error %.3g of the vector bound, %.3g of the entry bound" % ((what,) + f[:2]))
        if load_ref is None:
            load_ref = (kw, ref)
    first = "lame+mass" if vector else "stiffness+mass"
    if first not in assembled:
        return
    A, ref = assembled[first]
    # products of the assembled operator: any order of summation stays within row_length eps |A| |x|
    rng = np.random.default_rng(17)
    rows = np.diff(A.to_csr()[0])
    X = [rng.standard_normal(V.n_local) for _ in range(3)]
    dX = [gpu.DeviceVector(V.n_local, x) for x in X]
    dY = [gpu.DeviceVector(n) for _ in X]
    A.spmv(dX[0], dY[0])
    got = [dY[0].get()]
    kinds = ["spmv"]
    if vector:
        gpu.spmv_multi(A, dX, dY)
        got += [y.get() for y in dY]
        kinds += ["spmv_multi %d" % j for j in range(3)]
    for kind, y, x in zip(kinds, got, [X[0]] + X):
        y_ref, ax = _host_product(A, x)
        worst = float((np.abs(y - y_ref) / np.maximum(rows * EPS * ax, 1e-300)).max())
        figures.append(("%s %s" % (tag, kind), (worst,)))
        if not (np.all(np.isfinite(y)) and worst <= 1.0):
            bad.append("%s %s: error %.3g of row_length eps |A| |x|" % (tag, kind, worst))
    # one Jacobi-CG solve, Dirichlet values on the whole boundary (the ball's surface, the ballast's faces)
    if load_ref is None:
        return
    nodes = c.boundary_nodes()
    g = 1.0 + c.x[nodes, 0] + 2.0 * c.x[nodes, 1]
    if vector:
        dofs = (nodes[:, None] * d + np.arange(d)[None, :]).ravel()
        vals = (1e-3 * g[:, None] * np.array([1.0, -0.5, 0.25])[None, :d]).ravel()
    else:
        dofs, vals = nodes, g
    Ab, bb = fo.apply_dirichlet(ref, load_ref[1], dofs, vals, True)
    u_ref = fo.solve_direct(Ab, bb)
    b = gpu.DeviceVector(n)
    gpu.assemble_vector(V, b, **load_ref[0])
    A.apply_dirichlet(b, dofs, vals, symmetric=True)
    x = gpu.DeviceVector(V.n_local)
    st = gpu.krylov_solve(A, b, x, rtol=1e-13, max_iter=5000, method="cg")
    err = float(np.abs(x.get()[:n] - u_ref).max() / (RTOL_SOLUTION * np.abs(u_ref).max()))
    figures.append(("%s solve (%d iterations)" % (tag, st["iterations"]), (err,)))
    if not (st["converged"] == 1 and err <= 1.0):
        bad.append("%s solve: converged %d after %d iterations, error %.3g of RTOL_SOLUTION max|u|" % (tag, st["converged"], st["iterations"], err))


def _run(gpu, family, size, hub_row):
    """(entry point -> "values" | "refused", failures, figures) of one case, computed once"""
    key = (family, size, hub_row)
    if key not in _runs:
        c = _case(*key)
        out, bad, figures = {}, [], []
        for vector in (False, True):
            _run_space(gpu, c, vector, out, bad, figures)
        _runs[key] = (out, bad, figures)
    return _runs[key]


# ---------------------------------------------------------------------------------------------------------------- tests
@pytest.mark.parametrize("family,size,hub_row", hm.cases())
def test_hub_spaces_match_the_oracle_or_refuse_by_row_length(gpu, family, size, hub_row):
    c = _case(family, size, hub_row)
    out, bad, figures = _run(gpu, family, size, hub_row)
    print("%s %d, hub of %d entries on row %d:" % (family, size, c.hub_len, c.row))
    for what, f in figures:
        print("    %-44s %s" % (what, " ".join("%.3g" % x for x in f)))
    print("    refused: %s" % sorted(k for k, v in out.items() if v == "refused"))
    assert not bad, bad
    # values up to the limit of each entry point, a refusal beyond it
    assert len(out) == 9
    want = {k: "values" if _limit(c, k) is None or c.hub_len <= _limit(c, k) else "refused" for k in out}
    assert out == want, {k: (out[k], want[k]) for k in out if out[k] != want[k]}


def test_supported_row_lengths_are_monotone(gpu):
    """what an entry point takes at one row length it takes at every shorter one"""
    for family, (_, _, sizes, _) in hm.FAMILIES.items():
        runs = sorted((_case(family, s, 63).hub_len, _run(gpu, family, s, 63)[0]) for s in sizes)
        for what in runs[0][1]:
            seq = [(length, out.get(what)) for length, out in runs]
            assert all(o in ("values", "refused") for _, o in seq), (family, what, seq)
            refused = [length for length, o in seq if o == "refused"]
            if refused:
                assert all(o == "refused" for length, o in seq if length >= refused[0]), (family, what, seq)
            print("%-16s %-40s values up to %s, refused from %s" % (family, what, max([l for l, o in seq if o == "values"], default=None),
                                                                       refused[0] if refused else None))


# ------------------------------------------------------------------------------------------ solid-mechanics gather kernels
# The per-entry gather lists (gmap_ptr / gmap_src) of the CG1 vector space and the per-node loops of the load kernels, on the longest
# hubs: 261 entries in the hub row and 516 cells on its diagonal block in 3-D, 129 entries and 128 cells in 2-D.  Tolerances: those of
# each family's own "kernels match the host reference" test.
def _solid_mesh(d):
    co, ce, hub = hm.ball(260) if d == 3 else hm.fan(128)
    return hm.with_ballast(co, ce, 63, hub)


def _smooth_u(co, amp):
    d = co.shape[1]
    x = co
    u = np.stack([amp * np.sin(1.3 * x[:, 0] + 0.7 * x[:, 1]) + 0.3 * amp * x[:, 1] ** 2,
                  amp * np.cos(0.9 * x[:, 0] - 1.1 * x[:, 1])] + ([amp * x[:, 0] * x[:, 2] + 0.5 * amp * np.sin(2 * x[:, 2])] if d == 3 else []),
                 axis=1)
    return u.ravel()


def _min_J(co, ce, u):
    d = co.shape[1]
    ce = ce.astype(np.int64)
    E0 = np.swapaxes(co[ce][:, 1:] - co[ce][:, :1], 1, 2)
    U = u.reshape(-1, d)[ce]
    return (np.linalg.det(E0 + np.swapaxes(U[:, 1:] - U[:, :1], 1, 2)) / np.linalg.det(E0)).min()


@pytest.mark.parametrize("d", [3, 2])
@pytest.mark.parametrize("model", ["neo_hookean", "mooney_rivlin"])
def test_hyperelastic_kernels_on_a_hub(gpu, d, model):
    import hyperelastic_models_reference as mr
    import hyperelastic_reference as hr
    co, ce, row = _solid_mesh(d)
    nc = len(ce)
    uh = _smooth_u(co, 0.05)
    assert _min_J(co, ce, uh) > 0.5
    r4 = np.random.default_rng(5).random((nc, 4))
    if model == "neo_hookean":
        mu, lm = 1.0 + r4[:, 0], 2.0 + r4[:, 1]
        kw = dict(lame=("cell", np.stack([mu, lm], axis=1)))
        e_h, f_h, K_h, J_h = hr.assemble(co, ce, uh, mu, lm)
    else:
        rows = np.stack([0.5 + 0.5 * r4[:, 0], 0.2 + 0.2 * r4[:, 1], 4.0 + r4[:, 2], 0 * r4[:, 3]], axis=1)
        kw = dict(lame=None, model=model, params=("cell", np.ascontiguousarray(rows[:, :3])))
        e_h, f_h, K_h, J_h, _ = mr.assemble(co, ce, uh, model, rows)
    assert J_h.min() > 0.5
    V = gpu.DeviceSpace(gpu.DeviceMesh(co, ce), d, 1)
    u = gpu.DeviceVector(V.n_local, uh)
    outs = []
    for _ in range(2):
        K, r = gpu.DeviceMatrix(V), gpu.DeviceVector(V.n_owned)
        info = gpu.assemble_hyperelastic(V, u, K=K, r=r, energy=True, **kw)
        assert info["n_inverted"] == 0
        outs.append((K.to_csr()[2], r.get(), info["energy"]))
    errs = (abs(_csr(K) - K_h).max() / abs(K_h).max(), np.abs(outs[0][1] - f_h).max() / np.abs(f_h).max(), abs(outs[0][2] - e_h) / abs(e_h))
    print("%s d=%d: relative errors tangent %.2e force %.2e energy %.2e" % ((model, d) + errs))
    assert max(errs) <= 1e-12
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


@pytest.mark.parametrize("d", [3, 2])
def test_geometric_stiffness_on_a_hub(gpu, d):
    import buckling_reference as br
    co, ce, row = _solid_mesh(d)
    nc = len(ce)
    mu0, lm0 = fo.lame(*MAT1)
    mu = mu0 * (1.0 + 0.5 * np.sin(np.arange(nc)))
    lm = lm0 * (1.0 + 0.3 * np.cos(0.7 * np.arange(nc)))
    uh = _smooth_u(co, 1e-3)
    V = gpu.DeviceSpace(gpu.DeviceMesh(co, ce), d, 1)
    u = gpu.DeviceVector(V.n_local, uh)
    ref = br.geometric_stiffness_csr(co, ce, uh, mu, lm)
    _, rec = br.cell_stress(co, ce, uh, mu, lm)
    out = []
    for _ in range(2):
        KG = gpu.DeviceMatrix(V)
        sig = KG.assemble_geometric(("cell", np.stack([mu, lm], axis=1)), u, cell_stress=True)
        out.append((KG.to_csr(), sig))
    rp, ci, va, shape = out[0][0]
    assert shape == ref.shape and np.array_equal(rp, ref.indptr) and np.array_equal(ci, ref.indices)
    errs = (np.abs(va - ref.data).max() / np.abs(ref.data).max(), np.abs(out[0][1] - rec).max() / np.abs(rec).max())
    print("geometric stiffness d=%d: relative errors K_G %.2e stress %.2e" % ((d,) + errs))
    assert max(errs) <= 1e-12
    assert np.array_equal(va, out[1][0][2]) and np.array_equal(out[0][1], out[1][1])


def test_von_mises_load_onto_a_hub_with_tables(gpu):
    """ball(127): the scalar CG1 target has a row of 128 entries, the longest that keeps its incidence tables; every contribution
    is non-negative, so the sum of the absolute contributions is the reference itself"""
    co, ce, hub = hm.ball(127)
    co, ce, row = hm.with_ballast(co, ce, 63, hub)
    mesh = gpu.DeviceMesh(co, ce)
    V, P = gpu.DeviceSpace(mesh, 3, 1), gpu.DeviceSpace(mesh, 1, 1)
    uh = _smooth_u(co, 1e-3)
    _, ref = fo.von_mises_projection(co, ce, uh.reshape(-1, 3), *MAT1)
    out = []
    for _ in range(2):
        b = gpu.DeviceVector(P.n_owned)
        gpu.assemble_von_mises(V, gpu.DeviceVector(V.n_local, uh), *fo.lame(*MAT1), P, b)
        out.append(b.get())
    err = np.abs(out[0] - ref)
    print("von Mises load: largest error %.3g of the entry bound" % (err / (RTOL_ASSEMBLY * ref)).max())
    assert ref.min() > 0.0 and np.all(err <= RTOL_ASSEMBLY * ref)
    assert np.array_equal(out[0], out[1])
    # the target without tables names its longest row
    co2, ce2, hub2 = hm.ball(128)
    co2, ce2, _ = hm.with_ballast(co2, ce2, 63, hub2)
    mesh2 = gpu.DeviceMesh(co2, ce2)
    V2, P2 = gpu.DeviceSpace(mesh2, 3, 1), gpu.DeviceSpace(mesh2, 1, 1)
    with pytest.raises(gpu.BackendError, match="129 entries"):
        gpu.assemble_von_mises(V2, gpu.DeviceVector(V2.n_local), *fo.lame(*MAT1), P2, gpu.DeviceVector(P2.n_owned))


@pytest.mark.parametrize("d", [3, 2])
def test_plasticity_kernels_on_a_hub(gpu, d):
    """the mixed state of test_gpu_plasticity.py (strains around the yield strain, a random admissible history, a material that
    varies from cell to cell) on the hub mesh: both branches among the cells of the hub"""
    import plasticity_reference as pr
    co, ce, row = _solid_mesh(d)
    nc = len(ce)
    rng = np.random.default_rng(40 + d)
    uh = _smooth_u(co, 1.7e-3 if d == 3 else 2.5e-3)
    b = 4e-4 * rng.standard_normal((nc, 3, 3))
    ep = 0.5 * (b + np.transpose(b, (0, 2, 1)))
    if d == 2:
        ep[:, :2, 2] = ep[:, 2, :2] = 0.0
    ep -= np.trace(ep, axis1=1, axis2=2)[:, None, None] * np.eye(3) / 3.0
    p = 1e-3 * rng.random(nc)
    mu0, lm0 = fo.lame(200.0, 0.3)
    mat = np.stack([mu0 * (1 + 0.2 * rng.random(nc)), lm0 * (1 + 0.2 * rng.random(nc)), 0.4 * (1 + 0.2 * rng.random(nc)),
                    20.0 * rng.random(nc)], axis=1)
    ref = pr.assemble(co, ce, uh, ep, p, *mat.T)
    fy = ref["fy"]
    at_hub = np.any(ce == row, axis=1)
    # the branch of a cell within rounding of f = 0 is undetermined: every cell stays away from it, both branches at the hub
    assert np.abs(fy / mat[:, 2]).min() > 1e-6 and 0.15 < (fy[at_hub] > 0).mean() < 0.85
    V = gpu.DeviceSpace(gpu.DeviceMesh(co, ce), d, 1)
    hist = gpu.PlasticHistory(V)
    hist.set(pr.pack(ep, d), p)
    u = gpu.DeviceVector(V.n_local, uh)
    outs = []
    for _ in range(2):
        K, r = gpu.DeviceMatrix(V), gpu.DeviceVector(V.n_owned)
        info = gpu.assemble_plasticity(V, u, hist, ("cell", mat), K=K, r=r)
        outs.append((K.to_csr()[2], r.get()))
    assert info["n_yielded"] == int((fy > 0).sum()) and info["n_nonfinite"] == 0
    errs = (abs(_csr(K) - ref["K"]).max() / abs(ref["K"]).max(), np.abs(outs[0][1] - ref["f"]).max() / np.abs(ref["f"]).max())
    print("plasticity d=%d: relative errors tangent %.2e force %.2e" % ((d,) + errs))
    assert max(errs) <= 1e-12
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


@pytest.mark.parametrize("d", [3, 2])
def test_viscoelastic_kernels_on_a_hub(gpu, d):
    """the per-cell three-term material of test_gpu_viscoelasticity.py, a random committed history: update and history load"""
    import viscoelastic_reference as vr
    co, ce, row = _solid_mesh(d)
    nc, nt, dt = len(ce), 3, 0.4
    rng = np.random.default_rng(7)
    mu0, lm0 = fo.lame(200.0, 0.3)
    mu, lm = mu0 * (1 + 0.2 * rng.random(nc)), lm0 * (1 + 0.2 * rng.random(nc))
    g = np.stack([0.3 * rng.random(nc) + 0.01, 0.3 * rng.random(nc) + 0.01, 0.3 * rng.random(nc) + 0.01], axis=1)
    tau = np.stack([10.0 ** rng.uniform(-3, 0, nc), 10.0 ** rng.uniform(0, 3, nc), 10.0 ** rng.uniform(4, 8, nc)], axis=1)
    material = ("cell", np.concatenate([mu[:, None], lm[:, None], np.stack([g, tau], axis=2).reshape(nc, 6)], axis=1))

    def random_dev(shape):
        b = 1e-3 * rng.standard_normal(shape + (3, 3))
        t = 0.5 * (b + np.swapaxes(b, -1, -2))
        if d == 2:
            t[..., :2, 2] = 0.0
            t[..., 2, :2] = 0.0
        return t - np.trace(t, axis1=-2, axis2=-1)[..., None, None] * np.eye(3) / 3.0

    def pack_h(h):
        return vr.pack(h.reshape(nc * nt, 3, 3), d).reshape(nc, nt, -1)
    e0, h0 = random_dev((nc,)), random_dev((nc, nt))
    uh = _smooth_u(co, 2e-3)
    V = gpu.DeviceSpace(gpu.DeviceMesh(co, ce), d, 1)
    hist = gpu.ViscoHistory(V, nt)
    hist.set(vr.pack(e0, d), pack_h(h0))
    u = gpu.DeviceVector(V.n_local, uh)
    outs = []
    for _ in range(2):
        r = gpu.DeviceVector(V.n_owned, np.full(V.n_owned, 123.0))           # overwritten
        info = gpu.assemble_viscoelastic(V, hist, material, dt, load=r, u=u)
        assert info["n_nonfinite"] == 0
        outs.append((r.get(),) + hist.get(trial=True))
    load, e1, h1, sg = outs[0]
    ref_e, ref_h, ref_s = vr.update(vr.strains(co, ce, uh)[0], e0, h0, mu, lm, g, tau, dt)
    ref_load = vr.history_load(co, ce, e0, h0, mu, g, tau, dt)
    errs = (np.abs(load - ref_load).max() / np.abs(ref_load).max(), np.abs(e1 - vr.pack(ref_e, d)).max() / np.abs(ref_e).max(),
            np.abs(h1 - pack_h(ref_h)).max() / np.abs(ref_h).max(), np.abs(sg - vr.pack(ref_s, d)).max() / np.abs(ref_s).max())
    print("viscoelasticity d=%d: relative errors load %.2e e %.2e h %.2e sigma %.2e" % ((d,) + errs))
    assert max(errs) <= 1e-12
    for a, b in zip(outs[0], outs[1]):
        assert np.array_equal(a, b)



def _aniso_state(ar, co, ce, row, d):
    """three materials spread over the cells, a random frame per cell (about z in plane strain), as test_gpu_anisotropic.py has them:
    (device material, the reference's global D per cell, eigenstrains in the tensor storage)"""
    nc = len(ce)
    table = np.stack([ar.to_library(ar.orthotropic_voigt(ar.CFRP['elastic_moduli'], ar.CFRP['poisson_ratios'], ar.CFRP['shear_moduli'])),
                      ar.to_library(ar.orthotropic_voigt([40e9, 12e9, 9e9], [0.28, 0.3, 0.42], [4e9, 3.5e9, 3.2e9])),
                      ar.to_library(ar.isotropic_voigt(3.5e9, 0.35))])
    table = 0.5 * (table + np.transpose(table, (0, 2, 1)))
    idx = np.random.default_rng(9).integers(0, 3, nc).astype(np.int32)
    assert len(np.unique(idx[np.any(ce == row, axis=1)])) == 3           # every material among the cells of the hub
    R = ar.random_rotations(nc, 21, about_z=(d == 2))
    eig = 1e-4 * np.random.default_rng(10).standard_normal((nc, 6 if d == 3 else 4))
    return (table, idx, R), ar.global_D(table, idx, R, nc), eig


@pytest.mark.parametrize("d", [3, 2])
def test_anisotropic_kernels_on_a_hub(gpu, d):
    """operator with its consistent mass, eigenstrain load, cell stresses and the von Mises load against
    tests/anisotropic_reference.py: identical pattern, 1e-12 max|ref| (the bound of test_gpu_anisotropic.py), two runs bit for bit"""
    import anisotropic_reference as ar
    co, ce, row = _solid_mesh(d)
    n = len(co)
    material, Dg, eig = _aniso_state(ar, co, ce, row, d)
    rho = 1600.0
    ref = ar.assemble(n, ce, ar.local_stiffness(co, ce, Dg) + ar.local_mass(co, ce, rho), d)
    ref_load = ar.eigenstress_load(n, co, ce, Dg, eig)
    uh = _smooth_u(co, 1e-3)
    ref_sig = ar.cell_stress(co, ce, uh, Dg, eig)
    mesh = gpu.DeviceMesh(co, ce)
    V = gpu.DeviceSpace(mesh, d, 1)
    u = gpu.DeviceVector(V.n_local, uh)
    outs = []
    for _ in range(2):
        A = gpu.DeviceMatrix(V)
        A.assemble_anisotropic(material, mass=rho)
        b = gpu.DeviceVector(V.n_owned)
        gpu.assemble_anisotropic_load(V, material, eig, b, add=False)
        sig = gpu.anisotropic_stress(V, u, material, eigenstrain=eig, cell_stress=True)
        outs.append((A.to_csr(), b.get(), sig))
    rp, ci, va, shape = outs[0][0]
    assert shape == ref.shape and np.array_equal(rp, ref.indptr) and np.array_equal(ci, ref.indices)
    errs = (np.abs(va - ref.data).max() / np.abs(ref.data).max(), np.abs(outs[0][1] - ref_load).max() / np.abs(ref_load).max(),
            np.abs(outs[0][2] - ref_sig).max() / np.abs(ref_sig).max())
    print("anisotropic d=%d: relative errors operator %.2e eigenstrain load %.2e stress %.2e" % ((d,) + errs))
    assert max(errs) <= 1e-12
    assert np.array_equal(va, outs[1][0][2]) and np.array_equal(outs[0][1], outs[1][1]) and np.array_equal(outs[0][2], outs[1][2])
    # the von Mises load walks the tables of the scalar CG1 space: 129 entries on the fan; in 3-D the ball of 127 points (128 entries)
    # keeps them and the one of 128 does not
    if d == 3:
        for size in (128, 127):
            co, ce, hub = hm.ball(size)
            co, ce, row = hm.with_ballast(co, ce, 63, hub)
            material, Dg, eig = _aniso_state(ar, co, ce, row, d)
            mesh = gpu.DeviceMesh(co, ce)
            V = gpu.DeviceSpace(mesh, 3, 1)
            P = gpu.DeviceSpace(mesh, 1, 1)
            if size == 128:
                with pytest.raises(gpu.BackendError, match="129 entries.*up to 128"):
                    gpu.anisotropic_stress(V, gpu.DeviceVector(V.n_local), material, p1_space=P, vm_rhs=gpu.DeviceVector(P.n_owned))
    else:
        P = gpu.DeviceSpace(mesh, 1, 1)
    n, uh = len(co), _smooth_u(co, 1e-3)
    ref_vm = ar.von_mises_rhs(n, co, ce, ar.cell_stress(co, ce, uh, Dg, eig))
    got = []
    for _ in range(2):
        b = gpu.DeviceVector(P.n_owned)
        gpu.anisotropic_stress(V, gpu.DeviceVector(V.n_local, uh), material, eigenstrain=eig, p1_space=P, vm_rhs=b)
        got.append(b.get())
    err = np.abs(got[0] - ref_vm).max() / np.abs(ref_vm).max()
    print("anisotropic d=%d: relative error von Mises load %.2e" % (d, err))
    assert err <= 1e-12 and np.array_equal(got[0], got[1])


def test_matrix_free_apply_on_a_hub_with_tables(gpu):
    """fs_operator_apply walks the incidence tables: the product of the assembled operator at 128 entries, refused at 129"""
    for size in (127, 128):
        co, ce, hub = hm.ball(size)
        co, ce, row = hm.with_ballast(co, ce, 63, hub)
        V = gpu.DeviceSpace(gpu.DeviceMesh(co, ce), 1, 1)
        xh = np.random.default_rng(2).standard_normal(V.n_local)
        x, y = gpu.DeviceVector(V.n_local, xh), gpu.DeviceVector(V.n_owned)
        if size == 128:
            with pytest.raises(gpu.BackendError, match="129 entries.*up to 128"):
                gpu.apply_operator(V, x, y, stiffness=K0, mass=M0)
            return
        gpu.apply_operator(V, x, y, stiffness=K0, mass=M0)
        A = gpu.DeviceMatrix(V)
        A.assemble(stiffness=K0, mass=M0)
        y_ref, ax = _host_product(A, xh)
        # the row of the local matrix is multiplied into x cell by cell: 4 products per cell, at most 4 x 250 terms in the hub row
        terms = 4 * np.bincount(ce.ravel(), minlength=len(co))
        worst = float((np.abs(y.get() - y_ref) / (terms * EPS * _abs_apply(co, ce, xh))).max())
        print("matrix-free apply at 128 entries: error %.3g of terms eps sum|Ke||x|" % worst)
        assert worst <= 1.0


def _abs_apply(co, ce, x):
    """sum over the cells of |local row| |x|: what the cell-by-cell product of fs_operator_apply is bounded by, row by row"""
    loc = np.abs(fo.p1_stiffness_local(co, ce, K0) + fo.p1_mass_local(co, ce, M0))
    return fo.assemble_generic_vector(len(co), ce, np.einsum("cab,cb->ca", loc, np.abs(x)[ce.astype(np.int64)]))


# ------------------------------------------------------------------------------------------ AMG on a wide row
def test_amg_solve_with_a_hub_row(gpu):
    """the strength, aggregation and Galerkin-product kernels with a block row of 261 entries: CG1 elasticity on the ball of 260
    surface points and its ballast, rigid-body near-null space, against a direct solve"""
    co, ce, row = _solid_mesh(3)
    n = len(co)
    V = gpu.DeviceSpace(gpu.DeviceMesh(co, ce), 3, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(lame=fo.lame(*MAT1))
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_vector(V, b, vector_value=tuple(BODY))
    # both parts held where they cannot move rigidly: the cap z < -0.6 of the ball, the face of the ballast nearest to it
    in_ball = np.linalg.norm(co - co[row], axis=1) < 1.25
    box_x0 = co[~in_ball, 0].min()
    held = np.flatnonzero((in_ball & (co[:, 2] < -0.6)) | (~in_ball & (co[:, 0] < box_x0 + 1e-9)))
    assert 10 < len(held) < n // 3 and row not in held
    dofs = (held[:, None] * 3 + np.arange(3)[None, :]).ravel()
    A.apply_dirichlet(b, dofs, 0.0, symmetric=True)
    K = fo.assemble_p1_elasticity(co, ce, *MAT1)
    Ab, bb = fo.apply_dirichlet(K, fo.assemble_p1_vector_source(co, ce, BODY), dofs, 0.0, True)
    ref = fo.solve_direct(Ab, bb)
    amg = gpu.AMG(A, nullspace="rigid_body")
    x = gpu.DeviceVector(V.n_local)
    st = amg.solve(b, x, rtol=1e-13)
    err = np.abs(x.get()[:3 * n] - ref).max() / np.abs(ref).max()
    print("AMG-CG with a 261-entry row: %d levels, %d iterations, error %.3g of max|u|" % (amg.info()["levels"], st["iterations"], err))
    assert st["converged"] == 1 and err <= RTOL_SOLUTION
