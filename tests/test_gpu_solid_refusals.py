"""The refusals of the solid-mechanics assembly entry points on the MI355X: fs_assemble_hyperelastic (neo-Hookean and St
Venant-Kirchhoff), fs_hyper_stress, fs_plastic_state_create, fs_assemble_plasticity, fs_visco_state_create, fs_assemble_viscoelastic,
fs_assemble_geometric_stiffness, fs_assemble_anisotropic, fs_anisotropic_stress and fs_assemble_anisotropic_load, each on
DeviceMesh.box(2, 2, 2) and on the 2 x 2 rectangle of triangles.  Every case calls the library with valid handles and holds the
return code and the text: wrong kinds of space, short vectors, a missing or foreign matrix, a missing or short force vector, a
history of another space, one constant material and one per-cell material (the message names the cell), and which message wins
where two conditions fail at once.  Each test ends with a call that the library accepts, on the handles it has just refused.

Codes: FS_ERR_INVALID (-1) everywhere but for DG handles, which every entry point turns away with FS_ERR_UNSUPPORTED (-4) and
"not built for DG spaces" before it looks at anything else.

Not covered, because no call with valid handles reaches them: "vector space without slot table" (fs_space_create gives every vector
space its slot table), "the space has ghost nodes" (one rank), the null-pointer refusals, and "the matrix is not on a vector
space" of fs_assemble_anisotropic (a matrix has the block size of its space)."""
import ctypes as C

import numpy as np
import pytest

from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu

INVALID, UNSUPPORTED = -1, -4
CG1 = "vector CG1 spaces on tetrahedra or triangles only"
DG = "not built for DG spaces"
SHORT_U = "displacement vector shorter than the space's dofs"
TANGENT = "the tangent needs a matrix on this space"
FORCE = "the internal force needs a vector of the space's owned dofs"
HISTORY = "the history belongs to another space"


class _Ctx:
    """the handles of one mesh: the vector CG1 space V with vectors and a matrix, a second space W of the same kind (another
    space to the library), and the three kinds the entry points refuse"""

    def __init__(self, d):
        from fenicssolver_amd import backend
        backend.init()
        self.d = d
        if d == 3:
            self.mesh = backend.DeviceMesh.box(2, 2, 2)
        else:
            co, ce = fo.rectangle_mesh((0.0, 0.0), (1.0, 1.0), 2, 2)
            self.mesh = backend.DeviceMesh(co, ce)
        self.nc = self.mesh.info()[1]
        self.ne = 6 if d == 3 else 4
        self.V, self.W = backend.DeviceSpace(self.mesh, d, 1), backend.DeviceSpace(self.mesh, d, 1)
        self.scalar, self.cg2, self.dg = backend.DeviceSpace(self.mesh, 1, 1), backend.DeviceSpace(self.mesh, d, 2), backend.DeviceDGSpace(self.mesh)
        self.kinds = ((self.scalar, INVALID, CG1), (self.cg2, INVALID, CG1), (self.dg, UNSUPPORTED, DG))
        n = self.V.n_local
        self.u = backend.DeviceVector(n, 1e-3 * np.arange(n))
        self.u_short = backend.DeviceVector(n - 1)
        self.r, self.r_short = backend.DeviceVector(self.V.n_owned), backend.DeviceVector(self.V.n_owned - 1)
        self.K, self.K_other = backend.DeviceMatrix(self.V), backend.DeviceMatrix(self.W)

    def cells(self, row, bad_cell, bad_row):
        """('cell', rows): `row` in every cell but `bad_cell`, which gets `bad_row`"""
        a = np.tile(np.asarray(row, dtype=np.float64), (self.nc, 1))
        a[bad_cell] = bad_row
        return ("cell", a)


@pytest.fixture(scope="module", params=[3, 2], ids=["box", "triangles"])
def ctx(request):
    return _Ctx(request.param)


def refused(call, code, *texts):
    """call() is a backend call (raises BackendError) or a raw library call (returns the code)"""
    from fenicssolver_amd import backend, _lib as L
    try:
        rc = call()
        msg = L.load().fs_last_error().decode()
    except backend.BackendError as e:
        rc, msg = e.rc, str(e)
    assert rc == code, (rc, msg)
    for t in texts:
        assert t in msg, (t, msg)


def _h(x):
    return x.h if x is not None else None


# ------------------------------------------------------------------------------------------------ hyperelasticity
@pytest.mark.parametrize("model", ["neo_hookean", "st_venant_kirchhoff"])
def test_assemble_hyperelastic(ctx, model):
    from fenicssolver_amd import backend as B, _lib as L
    who = "fs_assemble_hyperelastic: "
    lame = (1.0, 2.0)

    def raw(space, K, r, u, what, info=True, lame=lame):
        keep = []
        f = B._hyper_form("test", space, lame, model, None, False, keep)
        i = L.fs_hyper_info()
        return L.load().fs_assemble_hyperelastic(space.h, _h(K), _h(r), u.h, C.byref(f), what, C.byref(i) if info else None)

    for space, code, text in ctx.kinds:
        refused(lambda: B.assemble_hyperelastic(space, ctx.u, lame, r=ctx.r, model=model), code, text)
    refused(lambda: raw(ctx.V, None, None, ctx.u, 8), INVALID, who + "unknown bits in what (8)")
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u_short, lame, K=ctx.K, model=model), INVALID, who + SHORT_U)
    refused(lambda: raw(ctx.V, None, None, ctx.u, L.FS_HYPER_TANGENT), INVALID, who + TANGENT)
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u, lame, K=ctx.K_other, model=model), INVALID, who + TANGENT)
    refused(lambda: raw(ctx.V, None, None, ctx.u, L.FS_HYPER_FORCE), INVALID, who + FORCE)
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u, lame, r=ctx.r_short, model=model), INVALID, who + FORCE)
    refused(lambda: raw(ctx.V, None, None, ctx.u, L.FS_HYPER_ENERGY, info=False), INVALID, who + "the energy needs an info struct")
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u, (-1.0, 2.0), r=ctx.r, model=model), INVALID, "mu > 0 and lambda >= 0 are required")
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u, ctx.cells(lame, 3, (1.0, float('nan'))), r=ctx.r, model=model), INVALID,
            "cell 3 (device order) has mu = 1, lambda = nan")
    # two conditions at once: the checks run space, displacement, tangent, force, material
    refused(lambda: B.assemble_hyperelastic(ctx.scalar, ctx.u_short, lame, K=ctx.K_other, model=model), INVALID, CG1)
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u_short, lame, K=ctx.K_other, model=model), INVALID, SHORT_U)
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u, lame, K=ctx.K_other, r=ctx.r_short, model=model), INVALID, TANGENT)
    refused(lambda: B.assemble_hyperelastic(ctx.V, ctx.u, (-1.0, 2.0), r=ctx.r_short, model=model), INVALID, FORCE)
    # and none of them left anything behind: the same handles assemble
    out = B.assemble_hyperelastic(ctx.V, ctx.u, lame, K=ctx.K, r=ctx.r, energy=True, model=model)
    assert out["n_inverted"] == 0 and np.isfinite(out["energy"])


def test_hyper_stress(ctx):
    from fenicssolver_amd import backend as B
    who = "fs_hyper_stress: "
    for space, code, text in ctx.kinds:
        refused(lambda: B.hyperelastic_stress(space, ctx.u, (1.0, 2.0)), code, text)
    refused(lambda: B.hyperelastic_stress(ctx.V, ctx.u_short, (1.0, 2.0)), INVALID, who + SHORT_U)
    refused(lambda: B.hyperelastic_stress(ctx.V, ctx.u, (0.0, 2.0)), INVALID, who + "the material has mu = 0, lambda = 2")
    refused(lambda: B.hyperelastic_stress(ctx.V, ctx.u, None, model="mooney_rivlin", params=(0.0, 0.0, 1.0)), INVALID,
            "c10 + c01 > 0 and kappa > 0 are required")
    refused(lambda: B.hyperelastic_stress(ctx.V, ctx.u, None, model="yeoh", params=ctx.cells((1.0, 0.0, 0.0, 1.0), 5, (1.0, 0.0, 0.0, 0.0))),
            INVALID, who + "cell 5 (device order) has c10 = 1")
    refused(lambda: B.hyperelastic_stress(ctx.scalar, ctx.u_short, (1.0, 2.0)), INVALID, CG1)
    refused(lambda: B.hyperelastic_stress(ctx.V, ctx.u_short, (0.0, 2.0)), INVALID, SHORT_U)
    assert np.isfinite(B.hyperelastic_stress(ctx.V, ctx.u, (1.0, 2.0))).all()


# ------------------------------------------------------------------------------------------------ plasticity
def test_plasticity(ctx):
    from fenicssolver_amd import backend as B, _lib as L
    who = "fs_assemble_plasticity: "
    mat = (1.0, 2.0, 0.5, 0.1)
    for space, code, text in ctx.kinds:
        refused(lambda: B.PlasticHistory(space), code, "fs_plastic_state_create: ", text)
    hist, foreign = B.PlasticHistory(ctx.V), B.PlasticHistory(ctx.W)

    def raw(what, K=None, r=None):
        f = L.fs_plastic_form()
        f.mu, f.lambda_, f.yield_stress, f.hardening = mat
        i = L.fs_plastic_info()
        return L.load().fs_assemble_plasticity(ctx.V.h, _h(K), _h(r), ctx.u.h, hist.h, C.byref(f), what, C.byref(i))

    for space, code, text in ctx.kinds:
        refused(lambda: B.assemble_plasticity(space, ctx.u, hist, mat, r=ctx.r), code, text)
    refused(lambda: raw(4), INVALID, who + "unknown bits in what (4)")
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, foreign, mat, r=ctx.r), INVALID, who + HISTORY)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u_short, hist, mat, r=ctx.r), INVALID, who + SHORT_U)
    refused(lambda: raw(L.FS_PLASTIC_TANGENT), INVALID, who + TANGENT)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, hist, mat, K=ctx.K_other), INVALID, who + TANGENT)
    refused(lambda: raw(L.FS_PLASTIC_FORCE), INVALID, who + FORCE)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, hist, mat, r=ctx.r_short), INVALID, who + FORCE)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, hist, (1.0, 2.0, 0.0, 0.1), r=ctx.r), INVALID,
            who + "mu > 0, lambda >= 0, yield stress > 0 and hardening >= 0 are required (mu = 1, lambda = 2, yield stress = 0")
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, hist, ctx.cells(mat, 5, (1.0, 2.0, 0.5, -1.0)), r=ctx.r), INVALID,
            who + "cell 5 (device order) has mu = 1, lambda = 2, yield stress = 0.5, hardening = -1")
    # two conditions at once: space, history, displacement, tangent, force, material
    refused(lambda: B.assemble_plasticity(ctx.scalar, ctx.u_short, foreign, mat, r=ctx.r), INVALID, CG1)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u_short, foreign, mat, r=ctx.r), INVALID, HISTORY)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u_short, hist, mat, K=ctx.K_other), INVALID, SHORT_U)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, hist, mat, K=ctx.K_other, r=ctx.r_short), INVALID, TANGENT)
    refused(lambda: B.assemble_plasticity(ctx.V, ctx.u, hist, (1.0, 2.0, 0.0, 0.1), r=ctx.r_short), INVALID, FORCE)
    out = B.assemble_plasticity(ctx.V, ctx.u, hist, mat, K=ctx.K, r=ctx.r)
    assert out["n_nonfinite"] == 0
    hist.close()
    foreign.close()


# ------------------------------------------------------------------------------------------------ viscoelasticity
def test_viscoelasticity(ctx):
    from fenicssolver_amd import backend as B, _lib as L
    who = "fs_assemble_viscoelastic: "
    mat = (1.0, 2.0, [(0.3, 0.5), (0.2, 5.0)])
    for space, code, text in ctx.kinds:
        refused(lambda: B.ViscoHistory(space, 2), code, "fs_visco_state_create: ", text)
    refused(lambda: B.ViscoHistory(ctx.V, 9), INVALID, "fs_visco_state_create: 9 Prony terms: 0 to FS_VISCO_MAX_TERMS = 8 are supported")
    refused(lambda: B.ViscoHistory(ctx.scalar, 9), INVALID, CG1)
    hist, foreign = B.ViscoHistory(ctx.V, 2), B.ViscoHistory(ctx.W, 2)

    def raw(what, r=None, u=None):
        f = L.fs_visco_form()
        f.mu, f.lambda_, f.n_terms, f.dt = 1.0, 2.0, 2, 0.1
        for k, (g, tau) in enumerate(mat[2]):
            f.g[k], f.tau[k] = g, tau
        i = L.fs_visco_info()
        return L.load().fs_assemble_viscoelastic(ctx.V.h, _h(r), _h(u), hist.h, C.byref(f), what, C.byref(i))

    for space, code, text in ctx.kinds:
        refused(lambda: B.assemble_viscoelastic(space, hist, mat, 0.1, u=ctx.u), code, text)
    refused(lambda: raw(8), INVALID, who + "unknown bits in what (8)")
    refused(lambda: raw(L.FS_VISCO_LOAD | L.FS_VISCO_FORCE, r=ctx.r), INVALID, who + "FS_VISCO_LOAD and FS_VISCO_FORCE write the same vector")
    refused(lambda: B.assemble_viscoelastic(ctx.V, foreign, mat, 0.1, u=ctx.u), INVALID, who + HISTORY)
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, (1.0, 2.0, [(0.3, 0.5)]), 0.1, u=ctx.u), INVALID,
            who + "the form has 1 Prony terms, the history was created for 2")
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, mat, 0.0, u=ctx.u), INVALID, who + "the step length is 0: dt > 0 and finite is required")
    refused(lambda: raw(L.FS_VISCO_UPDATE), INVALID, who + "the update needs a displacement vector of the space's dofs")
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, mat, 0.1, u=ctx.u_short), INVALID, who + "the update needs a displacement vector")
    need_r = who + "the history load and the internal force need a vector of the space's owned dofs"
    refused(lambda: raw(L.FS_VISCO_LOAD), INVALID, need_r)
    refused(lambda: raw(L.FS_VISCO_FORCE), INVALID, need_r)
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, mat, 0.1, load=ctx.r_short), INVALID, need_r)
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, mat, 0.1, force=ctx.r_short), INVALID, need_r)
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, (-1.0, 2.0, mat[2]), 0.1, u=ctx.u), INVALID,
            who + "mu = -1, lambda = 2: mu > 0 and a bulk modulus lambda + 2/3 mu > 0 are required")
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, (1.0, 2.0, [(0.6, 0.5), (0.5, 5.0)]), 0.1, u=ctx.u), INVALID, "sum g_k < 1 is required")
    row = (1.0, 2.0, 0.3, 0.5, 0.2, 5.0)
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, ctx.cells(row, 2, (1.0, 2.0, 0.3, 0.5, 0.2, 0.0)), 0.1, u=ctx.u), INVALID,
            who + "cell 2 (device order): Prony term 1 has relative modulus 0.2 and relaxation time 0")
    # two conditions at once: space, history, terms, step length, displacement, vector, material
    refused(lambda: B.assemble_viscoelastic(ctx.scalar, foreign, mat, 0.0, u=ctx.u_short), INVALID, CG1)
    refused(lambda: B.assemble_viscoelastic(ctx.V, foreign, mat, 0.0, u=ctx.u_short), INVALID, HISTORY)
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, mat, 0.0, u=ctx.u_short), INVALID, "the step length is 0")
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, mat, 0.1, u=ctx.u_short, load=ctx.r_short), INVALID, "the update needs a displacement")
    refused(lambda: B.assemble_viscoelastic(ctx.V, hist, (-1.0, 2.0, mat[2]), 0.1, load=ctx.r_short), INVALID, need_r)
    out = B.assemble_viscoelastic(ctx.V, hist, mat, 0.1, u=ctx.u, load=ctx.r)
    assert out["n_nonfinite"] == 0
    hist.close()
    foreign.close()


# ------------------------------------------------------------------------------------------------ geometric stiffness
def test_geometric_stiffness(ctx):
    from fenicssolver_amd import backend as B, _lib as L
    who = "fs_assemble_geometric_stiffness: "
    lame = (1.0, 2.0)
    for space, code, text in ctx.kinds[:2]:
        refused(lambda: B.DeviceMatrix(space).assemble_geometric(lame, ctx.u), code, who + text)
    refused(lambda: B.DeviceDGMatrix(ctx.dg).assemble_geometric(lame, ctx.u), UNSUPPORTED, who + DG)
    refused(lambda: L.load().fs_assemble_geometric_stiffness(ctx.V.h, 1.0, 2.0, None, ctx.u.h, ctx.K_other.h, None), INVALID,
            who + "the matrix is not on this space")
    refused(lambda: ctx.K.assemble_geometric(lame, ctx.u_short), INVALID, who + SHORT_U)
    refused(lambda: ctx.K.assemble_geometric((1.0, float('inf')), ctx.u), INVALID, who + "mu = 1, lambda = inf are not finite")
    refused(lambda: ctx.K.assemble_geometric(ctx.cells(lame, 4, (float('nan'), 2.0)), ctx.u), INVALID, who + "cell 4 (device order) has mu = nan")
    # two conditions at once: space, matrix, displacement, material
    refused(lambda: B.DeviceMatrix(ctx.scalar).assemble_geometric(lame, ctx.u_short), INVALID, CG1)
    refused(lambda: L.load().fs_assemble_geometric_stiffness(ctx.V.h, 1.0, 2.0, None, ctx.u_short.h, ctx.K_other.h, None), INVALID,
            "the matrix is not on this space")
    refused(lambda: ctx.K.assemble_geometric((1.0, float('inf')), ctx.u_short), INVALID, SHORT_U)
    assert np.isfinite(ctx.K.assemble_geometric(lame, ctx.u, cell_stress=True)).all()


# ------------------------------------------------------------------------------------------------ anisotropic elasticity
def _aniso(ctx, bad=None):
    """(table, material_of_cell, frames): the identity as the one material; bad = 'table': an entry that is not finite,
    'index': cell 3 points past the table, 'frame': the frame of cell 1 is not finite"""
    table = np.eye(6)[None].copy()
    index = np.zeros(ctx.nc, dtype=np.int32)
    frames = None
    if bad == "table":
        table[0, 1, 1] = float('nan')
    elif bad == "index":
        index[3] = 1
    elif bad == "frame":
        frames = np.tile(np.eye(3), (ctx.nc, 1, 1))
        frames[1, 0, 0] = float('inf')
    return (table, index, frames)


def test_assemble_anisotropic(ctx):
    from fenicssolver_amd import backend as B
    who = "fs_assemble_anisotropic: "
    for space, code, text in ctx.kinds[:2]:
        refused(lambda: B.DeviceMatrix(space).assemble_anisotropic(_aniso(ctx)), code, who + text)
    refused(lambda: B.DeviceDGMatrix(ctx.dg).assemble_anisotropic(_aniso(ctx)), UNSUPPORTED, who + DG)
    refused(lambda: ctx.K.assemble_anisotropic(_aniso(ctx), mass=float('nan')), INVALID, who + "the mass coefficient nan is not finite")
    refused(lambda: ctx.K.assemble_anisotropic(_aniso(ctx, "table")), INVALID, who + "material 0 has a stiffness entry that is not finite")
    refused(lambda: ctx.K.assemble_anisotropic(_aniso(ctx, "index")), INVALID, who + "cell 3 (device order) has material index 1 outside 0 .. 0")
    refused(lambda: ctx.K.assemble_anisotropic(_aniso(ctx, "frame")), INVALID, who + "the frame of cell 1 (device order) is not finite")
    if ctx.d == 2:
        table = np.eye(6)[None].copy()
        table[0, 0, 4] = table[0, 4, 0] = 0.5
        refused(lambda: ctx.K.assemble_anisotropic((table, None, None)), INVALID, who + "plane strain needs a material that is monoclinic about z")
    # two conditions at once: space, mass coefficient, material
    refused(lambda: B.DeviceMatrix(ctx.scalar).assemble_anisotropic(_aniso(ctx, "table"), mass=float('nan')), INVALID, CG1)
    refused(lambda: ctx.K.assemble_anisotropic(_aniso(ctx, "table"), mass=float('nan')), INVALID, "the mass coefficient nan is not finite")
    ctx.K.assemble_anisotropic(_aniso(ctx), mass=1.0)
    B.synchronize()


def test_anisotropic_stress(ctx):
    from fenicssolver_amd import backend as B, _lib as L
    who = "fs_anisotropic_stress: "
    vm, vm_short = B.DeviceVector(ctx.scalar.n_owned), B.DeviceVector(ctx.scalar.n_owned - 1)

    def raw(p1_space, vm_rhs):
        keep = []
        m = B._aniso_material(_aniso(ctx), ctx.nc, keep)
        return L.load().fs_anisotropic_stress(ctx.V.h, ctx.u.h, C.byref(m), None, None, _h(p1_space), _h(vm_rhs))

    for space, code, text in ctx.kinds:
        refused(lambda: B.anisotropic_stress(space, ctx.u, _aniso(ctx), cell_stress=True), code, who, text)
    refused(lambda: B.anisotropic_stress(ctx.V, ctx.u_short, _aniso(ctx)), INVALID, who + SHORT_U)
    refused(lambda: raw(ctx.scalar, None), INVALID, who + "the von Mises load needs both the scalar CG1 space and its vector")
    refused(lambda: raw(None, vm), INVALID, who + "the von Mises load needs both the scalar CG1 space and its vector")
    refused(lambda: raw(ctx.dg, vm), UNSUPPORTED, who + DG)
    refused(lambda: raw(ctx.W, vm), INVALID, who + "the target is the scalar CG1 space of the mesh")
    refused(lambda: raw(ctx.scalar, vm_short), INVALID, who + "vector too short")
    refused(lambda: B.anisotropic_stress(ctx.V, ctx.u, _aniso(ctx, "table")), INVALID, who + "material 0 has a stiffness entry that is not finite")
    refused(lambda: B.anisotropic_stress(ctx.V, ctx.u, _aniso(ctx, "index")), INVALID, who + "cell 3 (device order) has material index 1")
    eig = np.zeros((ctx.nc, ctx.ne))
    eig[1, 2] = float('nan')
    refused(lambda: B.anisotropic_stress(ctx.V, ctx.u, _aniso(ctx), eigenstrain=eig), INVALID, who + "the eigenstrain of cell 1 (device order) is not finite")
    # two conditions at once: space, displacement, von Mises target, material, eigenstrain
    refused(lambda: B.anisotropic_stress(ctx.scalar, ctx.u_short, _aniso(ctx, "table")), INVALID, CG1)
    refused(lambda: B.anisotropic_stress(ctx.V, ctx.u_short, _aniso(ctx, "table")), INVALID, SHORT_U)
    refused(lambda: B.anisotropic_stress(ctx.V, ctx.u, _aniso(ctx, "table"), eigenstrain=eig), INVALID, "stiffness entry that is not finite")
    sig = B.anisotropic_stress(ctx.V, ctx.u, _aniso(ctx), cell_stress=True, p1_space=ctx.scalar, vm_rhs=vm)
    assert np.isfinite(sig).all()


def test_assemble_anisotropic_load(ctx):
    from fenicssolver_amd import backend as B, _lib as L
    who = "fs_assemble_anisotropic_load: "
    eig = np.full((ctx.nc, ctx.ne), 1e-3)
    bad_eig = eig.copy()
    bad_eig[1, 0] = float('nan')

    def raw(space, material, e, b):            # (the wrapper sizes the eigenstrain by the space's components)
        keep = []
        m = B._aniso_material(material, ctx.nc, keep)
        return L.load().fs_assemble_anisotropic_load(space.h, C.byref(m), L.p_f64(e), b.h, 1)

    for space, code, text in ctx.kinds:
        refused(lambda: raw(space, _aniso(ctx), eig, ctx.r), code, who, text)
    refused(lambda: B.assemble_anisotropic_load(ctx.V, _aniso(ctx), eig, ctx.r_short), INVALID, who + "vector too short")
    refused(lambda: B.assemble_anisotropic_load(ctx.V, _aniso(ctx, "table"), eig, ctx.r), INVALID, who + "material 0 has a stiffness entry that is not finite")
    refused(lambda: B.assemble_anisotropic_load(ctx.V, _aniso(ctx, "index"), eig, ctx.r), INVALID, who + "cell 3 (device order) has material index 1")
    refused(lambda: B.assemble_anisotropic_load(ctx.V, _aniso(ctx), bad_eig, ctx.r), INVALID, who + "the eigenstrain of cell 1 (device order) is not finite")
    # two conditions at once: space, vector, material, eigenstrain
    refused(lambda: raw(ctx.scalar, _aniso(ctx, "table"), bad_eig, ctx.r_short), INVALID, CG1)
    refused(lambda: B.assemble_anisotropic_load(ctx.V, _aniso(ctx, "table"), bad_eig, ctx.r_short), INVALID, "vector too short")
    refused(lambda: B.assemble_anisotropic_load(ctx.V, _aniso(ctx, "table"), bad_eig, ctx.r), INVALID, "stiffness entry that is not finite")
    B.assemble_anisotropic_load(ctx.V, _aniso(ctx), eig, ctx.r, add=False)
    assert np.isfinite(ctx.r.get()).all()
