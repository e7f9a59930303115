"""What the products do with the memory at and behind the end of a vector.

The marching-window loaders (k_box_spmv, k_lat_march, k_box_cg_iter) copy x into LDS in 16-byte pairs clamped to the last pair
that starts inside the vector.  For an odd n that pair is (x[n - 1], x[n]): x[n] is not part of the vector, and the top-plane terms
meet it with zero coefficients - harmless only while it is finite, since fma(0, NaN, acc) is NaN.  The block cache hands out re-used
blocks with whatever their last owner left in them, so these tests fill the cache with NaN, Inf and all-ones bits (an int32 -1 array,
a NaN as a double) before the library allocates, and check every product kind against a host fp64 reference and against the same
work on a zero-filled cache, bit for bit (fma(+-0, finite, acc) == acc).

Kinds 0, 1, 3 and 4 are reached through fs_spmv_dictionary; kinds 2 and 5 need the lattice order a solve sets up, so they are
tested through solves only.  The lattice of a CG2 box has (2 nx + 1)(2 ny + 1)(2 nz + 1) rows, always odd: there is no even CG2
control."""
import numpy as np
import pytest

from spmv_reference import _check_against_host, _host_product, _poison, _vector_from_cache

pytestmark = pytest.mark.gpu

PATTERNS = ("zero", "finite", "nan", "inf", "ones")


# ---- products --------------------------------------------------------------------------------------------------------------------

P1_BOXES = [(20, 20, 20), (70, 8, 10), (12, 12, 500), (21, 20, 20)]     # odd n: 9261, 7029, 84669 (many z-chunks); even: 9702
P1_KINDS = {0: {"row_dictionary": (0, 1)}, 1: {"box_spmv": (0, 1)}, 3: {"box_min_rows": (0, 1500000)}}


def _product_runs(gpu, A, n_local, n_owned, kind, opts, seed):
    rng = np.random.default_rng(seed)
    xv = rng.standard_normal(n_local)
    y_ref, ax = _host_product(A, xv)
    out = {}
    try:
        for name, (on, _) in opts.items():
            gpu.set_option(name, on)
        for pattern in ("zero", "finite", "nan", "inf", "ones"):
            y = gpu.DeviceVector(n_owned)
            _poison(gpu, (n_local + 1, n_local + 2), pattern, seed)
            x = _vector_from_cache(gpu, n_local)
            x.set(xv)
            nc = A.spmv_dictionary(x, y)
            assert gpu.last_product_kind() == kind, (pattern, gpu.last_product_kind(), kind)
            assert (nc > 0) == (kind != 0), nc
            out[pattern] = y.get()
            x.close()
            y.close()
    finally:
        for name, (_, off) in opts.items():
            gpu.set_option(name, off)
    for pattern, y in out.items():
        _check_against_host(y, y_ref, ax, (kind, pattern))
        assert np.array_equal(y, out["zero"]), (kind, pattern, int((y != out["zero"]).sum()))


@pytest.mark.parametrize("kind", sorted(P1_KINDS))
@pytest.mark.parametrize("dims", P1_BOXES)
def test_p1_box_product_with_poisoned_tails(gpu, dims, kind):
    """Kinds 0 (streaming), 1 (k_dict_spmv) and 3 (k_box_spmv) of a P1 box operator with a mass term, x in a block of the cache that
    held NaN / Inf / all-ones bits / random numbers / zeros: every row within 4 eps |A| |x| of the host product, finite, and equal to
    the product on the zero-filled cache.  Shapes: odd n with odd and even plane strides (the windows of every other plane start one
    entry early), lines longer than a patch, a deep box of many z-chunks, an even-n control."""
    nx, ny, nz = dims
    mesh = gpu.DeviceMesh.box(nx, ny, nz)
    V = gpu.DeviceSpace(mesh, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=20.0, mass=0.7)
    _product_runs(gpu, A, V.n_local, V.n_owned, kind, P1_KINDS[kind], seed=sum(dims))


def test_block_row_product_with_poisoned_tails(gpu):
    """Kind 4 (k_dict_spmv3): the 3 x 3 block rows of the elasticity operator of a uniform box (above the 150 000 nodes from which
    the block form is used; 3 x 156 839 rows, odd), as the P1 products."""
    mesh = gpu.DeviceMesh.box(70, 46, 46, (0.0, 0.0, 0.0), (2.0, 1.0, 1.0))
    V = gpu.DeviceSpace(mesh, 3)
    A = gpu.DeviceMatrix(V)
    A.assemble(lame=(1.0, 1.5))
    assert V.n_owned % 2 == 1
    _product_runs(gpu, A, V.n_local, V.n_owned, 4, {}, seed=4)


# ---- solves ----------------------------------------------------------------------------------------------------------------------

def _p1_box(gpu, n, mass=None):
    mesh = gpu.DeviceMesh.box(n, n, n)
    V = gpu.DeviceSpace(mesh, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=20.0, mass=mass)
    nn = (n + 1) ** 2
    dofs = np.concatenate([np.arange(nn), np.arange(n * nn, (n + 1) * nn)]).astype(np.int32)
    vals = np.concatenate([np.full(nn, 350.0), np.full(nn, 300.0)])
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_vector(V, b, source=1.0)
    A.apply_dirichlet(b, dofs, vals, True)
    return V, A, b


def _cg2_box(gpu, nx, ny, nz):
    mesh = gpu.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    V = gpu.DeviceSpace(mesh, 1, degree=2)
    xyz, _, _ = mesh.get()
    edges = V.edges().astype(np.int64)
    co = np.concatenate([xyz[:, 0], 0.5 * (xyz[edges[:, 0], 0] + xyz[edges[:, 1], 0])])
    lo, hi = np.flatnonzero(co == 0.0), np.flatnonzero(co == 1.0)
    A = gpu.DeviceMatrix(V)
    b = gpu.DeviceVector(V.n_owned)
    A.assemble(stiffness=20.0)
    b.fill(0.0)
    A.apply_dirichlet(b, np.concatenate([lo, hi]).astype(np.int32), np.concatenate([np.full(len(lo), 350.0), np.full(len(hi), 300.0)]), True)
    return V, A, b


def _tiny_solve(gpu):
    """A solve of another size: the next solve's Krylov workspace is allocated again (ws_prepare keeps it while n is unchanged)."""
    V, A, b = _p1_box(gpu, 3)
    x = gpu.DeviceVector(V.n_owned)
    st = gpu.krylov_solve(A, b, x, rtol=1e-8, max_iter=500)
    assert st["converged"] == 1


# name: (problem, solve keywords, options (on, restored), product kind, fused iteration).  CG without the diagonal scaling and
# BiCGStab do not take the row-dictionary form on this box (row_classes 0: the streaming product, kind 0); they stay for their
# workspaces (r, p, z, w, s, rhat, t of n + 2 entries), which the other cases share only in part.
SOLVES = {
    "cg_scaled": ("p1", dict(method="cg", diagonal_scale=True), {"box_min_rows": (0, 1500000), "cg_fused": (0, -1)}, 3, 0),
    "cg_unscaled": ("p1", dict(method="cg", diagonal_scale=False), {"box_min_rows": (0, 1500000), "cg_fused": (0, -1)}, 0, 0),
    "bicgstab": ("p1_mass", dict(method="bicgstab", diagonal_scale=True), {"box_min_rows": (0, 1500000), "cg_fused": (0, -1)}, 0, 0),
    "pipelined": ("p1", dict(method="cg", pipelined=True), {"box_min_rows": (0, 1500000), "cg_fused": (0, -1)}, 3, 0),
    "box_iter": ("p1", dict(method="cg"), {"box_iter_min_rows": (0, 400000), "cg_fused": (1, -1), "box_iter": (1, 0)}, 3, 1),
    "lattice_march": ("cg2", dict(method="cg"), {"lattice_order": (1, -1), "cg_fused": (0, -1), "lattice_march": (1, 1)}, 5, 0),
    "lattice_march_lines": ("cg2_lines", dict(method="cg"), {"lattice_order": (1, -1), "cg_fused": (0, -1), "lattice_march": (1, 1)}, 5, 0),
    "lattice_tiles": ("cg2", dict(method="cg"), {"lattice_order": (1, -1), "cg_fused": (0, -1), "lattice_march": (0, 1)}, 2, 0),
}


@pytest.mark.parametrize("case", sorted(SOLVES))
def test_solve_with_poisoned_cache(gpu, case):
    """Krylov solves whose workspace (r, p, z, w, s of n + 2 entries, re-allocated after a solve of another size) and x come out of a
    cache poisoned with random numbers, NaN, Inf or all-ones bits: the same iteration count as on a zero-filled cache, the same
    solution bit for bit, the true residual at the tolerance, no NaN in the history.  P1 box of 41^3 rows (odd) through k_box_spmv
    (CG, pipelined CG, the one-launch k_box_cg_iter) or the streaming product (CG without the diagonal scaling, BiCGStab with a mass
    term); CG2 boxes in lattice order through
    k_lat_march (83 x 57 x 45 rows: lines of one piece; 141 x 53 x 37: lines of two) and the tile product k_lattice_spmv.  (A CG2
    cube of 20 cells a side is not solved in lattice order: product kind 0.)"""
    problem, kw, opts, kind, fused = SOLVES[case]
    rtol = 1e-10
    if problem.startswith("p1"):
        V, A, b = _p1_box(gpu, 40, mass=0.3 if problem == "p1_mass" else None)
    else:
        V, A, b = _cg2_box(gpu, *((41, 28, 22) if problem == "cg2" else (70, 26, 18)))
    n = V.n_owned
    assert n % 2 == 1
    runs = {}
    try:
        for name, (on, _) in opts.items():
            gpu.set_option(name, on)
        for pattern in PATTERNS:
            _tiny_solve(gpu)
            _poison(gpu, (n + 1, n + 2), pattern, seed=7)
            x = _vector_from_cache(gpu, n)
            st = gpu.krylov_solve(A, b, x, rtol=rtol, max_iter=5000, **kw)
            runs[pattern] = (st, x.get(), gpu.krylov_history().copy())
            x.close()
    finally:
        for name, (_, off) in opts.items():
            gpu.set_option(name, off)
    s0, x0, _ = runs["zero"]
    for pattern, (st, xs, hist) in runs.items():
        assert st["converged"] == 1, (pattern, st)
        assert st["product_kind"] == kind and (st["row_classes"] > 0) == (kind != 0), (pattern, st["product_kind"], kind)
        if fused:
            assert st["fused_iteration"] == 1, (pattern, st)
        assert st["iterations"] == s0["iterations"], (pattern, st["iterations"], s0["iterations"])
        assert np.all(np.isfinite(hist)), (pattern, int((~np.isfinite(hist)).sum()))
        assert np.array_equal(xs, x0), (pattern, int((xs != x0).sum()))
        assert st["true_rel_residual"] <= 5 * rtol, (pattern, st["true_rel_residual"])


def test_elasticity_amg_solve_with_poisoned_cache(gpu):
    """The AMG-preconditioned CG of the elasticity box, whose fine-level products run through k_dict_spmv3 (kind 4: row_classes > 0,
    as in test_gpu_kernels.py - the last product of a V-cycle is a coarse level's), with the hierarchy, the workspace and x allocated
    from a cache poisoned as above: same iterations, same solution bit for bit, the true residual at the tolerance."""
    nx, ny, nz = 70, 46, 46
    mesh = gpu.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), (2.0, 1.0, 1.0))
    V = gpu.DeviceSpace(mesh, 3)
    A = gpu.DeviceMatrix(V)
    A.assemble(lame=(1.0, 1.5))
    nodes = np.arange((nx + 1) * (ny + 1) * (nz + 1))
    left = nodes[nodes % (nx + 1) == 0]
    dofs = (left[:, None] * 3 + np.arange(3)).ravel().astype(np.int32)
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_vector(V, b, vector_value=(0.0, 0.0, -1.0))
    A.apply_dirichlet(b, dofs, 0.0, True)
    n = V.n_owned
    rtol = 1e-9
    runs = {}
    for pattern in PATTERNS:
        _tiny_solve(gpu)
        _poison(gpu, (n + 1, n + 2), pattern, seed=8)
        x = _vector_from_cache(gpu, n)
        amg = gpu.AMG(A, nullspace="rigid_body")
        st = amg.solve(b, x, rtol=rtol)
        runs[pattern] = (st, x.get(), gpu.krylov_history().copy())
        amg.close()
        x.close()
    s0, x0, _ = runs["zero"]
    for pattern, (st, xs, hist) in runs.items():
        assert st["converged"] == 1 and st["row_classes"] > 0, (pattern, st)
        assert st["iterations"] == s0["iterations"], (pattern, st["iterations"], s0["iterations"])
        assert np.all(np.isfinite(hist)), pattern
        assert np.array_equal(xs, x0), (pattern, int((xs != x0).sum()))
        assert st["true_rel_residual"] <= 5 * rtol, (pattern, st["true_rel_residual"])
