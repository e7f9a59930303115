"""The host dispatch of fs_assemble_matrix / fs_assemble_vector: every (dimension, degree, block size) family with and without
`add`, with per-cell Lame parameters, with the advection / SUPG variants and with the box fast path on and off.

Every stored matrix value is written once per assembly and `add` is one fp64 addition per entry, so the matrix assertions
are exact: a launch with a swapped template flag (ADD, CELL, ADV) cannot pass them.  The meshes are the smallest with one
full 64-row slice and a partial one."""
import numpy as np
import pytest

from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps
MAX_CELLS_PER_NODE = 64        # bound of the load-vector tolerance; asserted from the cell arrays below

# (mesh kind, components, degree)
SPACES = [(kind, nc, deg) for kind in ("box", "jittered", "triangles") for nc in (1, "vector") for deg in (1, 2)]
# Every load-vector kernel these spaces reach sums a row's cells in ascending order, except the one of scalar CG1 on triangles
# (k_assemble_tri_source: thread per cell, fp64 atomics), where two runs need not agree in the last bits.
ATOMIC_LOADS = {("triangles", 1, 1)}


@pytest.fixture(scope="module")
def meshes(gpu):
    """kind -> (mesh, cells [n_cells, vertices per cell], topological dimension)"""
    box = gpu.DeviceMesh.box(4, 4, 3)
    assert box.info()[:2] == (100, 288)
    co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), 4, 4, 3)
    h = np.array([1.0 / 4, 1.0 / 4, 1.0 / 3])
    inner = np.all((co > 1e-12) & (co < 1.0 - 1e-12), axis=1)
    assert inner.any()
    co = co + 0.1 * h * np.random.default_rng(11).uniform(-1.0, 1.0, co.shape) * inner[:, None]
    co2, ce2 = fo.rectangle_mesh((0, 0), (2, 0.5), 9, 8)
    assert len(co) == 100 and len(co2) == 90
    out = {"box": (box, box.get()[1], 3), "jittered": (gpu.DeviceMesh(co, ce), ce, 3), "triangles": (gpu.DeviceMesh(co2, ce2), ce2, 2)}
    for _, cells, _ in out.values():
        assert np.bincount(np.asarray(cells).ravel()).max() <= MAX_CELLS_PER_NODE
    return out


def _space(gpu, meshes, kind, ncomp, degree):
    mesh, cells, tdim = meshes[kind]
    return gpu.DeviceSpace(mesh, ncomp=(tdim if ncomp == "vector" else 1), degree=degree), len(cells), tdim


def _values(A):
    return A.to_csr()[2].copy()


def _check_matrix_forms(gpu, V, forms):
    for kw in forms:
        A1, A2, A3 = gpu.DeviceMatrix(V), gpu.DeviceMatrix(V), gpu.DeviceMatrix(V)
        A1.assemble(**kw)
        A2.assemble(**kw)
        v = _values(A1)
        assert v.any(), kw
        assert np.array_equal(v, _values(A2)), kw                     # 1. two fresh matrices agree
        A3.assemble(mass=99.0)
        A3.assemble(**kw)
        assert np.array_equal(v, _values(A3)), kw                     # 2. without add, what the matrix held is gone
        A3.assemble(add=True, **kw)
        assert np.array_equal(2.0 * v, _values(A3)), kw               # 3. add: one fp64 addition per entry


@pytest.mark.parametrize("kind,ncomp,degree", SPACES)
def test_assemble_matrix_add_and_overwrite_are_exact(gpu, meshes, kind, ncomp, degree):
    V, n_cells, tdim = _space(gpu, meshes, kind, ncomp, degree)
    if ncomp == "vector":
        pairs = np.random.default_rng(5).uniform((1.0, 0.5), (2.0, 1.5), (n_cells, 2))
        forms = [dict(lame=lame, **m) for lame in ((1.3, 0.8), ("cell", pairs)) for m in ({}, dict(mass=0.7))]
        _check_matrix_forms(gpu, V, forms)
        return
    vel = (0.6, -0.3, 0.2 if tdim == 3 else 0.0)
    forms = [dict(stiffness=1.7), dict(stiffness=1.7, mass=0.9), dict(stiffness=1.7, advection=vel),
             dict(stiffness=1.7, advection=vel, supg_pe=2.0)]
    if kind != "box":
        _check_matrix_forms(gpu, V, forms)
        return
    try:
        for fast in (1, 0):
            gpu.set_option("box_assembly", fast)
            _check_matrix_forms(gpu, V, forms)
    finally:
        gpu.set_option("box_assembly", 1)


@pytest.mark.parametrize("kind,ncomp,degree", SPACES)
def test_assemble_vector_add_and_overwrite(gpu, meshes, kind, ncomp, degree):
    """Without add a pre-filled vector comes out as a fresh one, bit for bit; with add the result is b0 + x to
    64 eps (|b0| + |x|): the atomic kernels add one cell's contribution at a time in no fixed order, and no node has more than
    64 cells around it.  The atomic kernel of ATOMIC_LOADS is held to that bound without add too, with the zero it starts from in
    the place of b0: 64 eps |x|."""
    V, _, tdim = _space(gpu, meshes, kind, ncomp, degree)
    kw = dict(vector_value=(0.3, -9.81, 0.5)[:tdim]) if ncomp == "vector" else dict(source=2.5)
    n = V.n_owned
    b0 = np.random.default_rng(7).uniform(-1.0, 1.0, n)
    fresh = gpu.DeviceVector(n)
    gpu.assemble_vector(V, fresh, **kw)
    x = fresh.get()
    assert x.any()
    b = gpu.DeviceVector(n, b0)
    gpu.assemble_vector(V, b, **kw)
    if (kind, ncomp, degree) in ATOMIC_LOADS:
        assert np.all(np.abs(b.get() - x) <= MAX_CELLS_PER_NODE * EPS * np.abs(x))
    else:
        assert np.array_equal(b.get(), x)
    b.set(b0)
    gpu.assemble_vector(V, b, add=True, **kw)
    err = np.abs(b.get() - (b0 + x))
    tol = MAX_CELLS_PER_NODE * EPS * (np.abs(b0) + np.abs(x))
    assert np.all(err <= tol), (err.max(), int((err > tol).sum()))
