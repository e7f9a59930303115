"""The one-launch CG iteration on work vectors with guard bands of zeros (option "cg_guard"): no item takes the clamped edge path, and
on a Kuhn box the own rows come out of the centre run instead of a run of their own.  A column outside the vector has a zero
coefficient, so fma(+0, 0, acc) replaces fma(+0, finite, acc); the own rows are the same memory words through the same two fmas:
everything a solve returns is equal BIT FOR BIT between cg_guard = 1 and cg_guard = 0 (the unguarded vectors and the kernels with
the edge path), whatever the block cache held where the bands are."""
import numpy as np
import pytest

from spmv_reference import _poison

pytestmark = pytest.mark.gpu

PAIR, DTAB, GUARD, CENTRE = 1, 2, 4, 8       # bits 0, 1 of fs_last_iteration_form, and bits 0, 1 of fs_last_iteration_guard behind them

# (nx, ny, nz), rtol of the converged solve.  12^3: 18 items, 5 of them edge items; 40^3: more than 64 iterations, so captured batches
# run; 30 x 7 x 5: 31 rows per line, 248 per plane - 12 items, 6 of them edge, items straddle several lines; 40 x 3 x 3: 6 items, all
# but one of them edge
BOXES = [((12, 12, 12), 1e-8), ((24, 24, 24), 1e-10), ((40, 40, 40), 1e-12), ((30, 7, 5), 1e-10), ((40, 3, 3), 1e-10)]


def _box_system(gpu, dims, p1=None):
    """Heat conduction on a box, the two z faces held at 350 and 300 (vertex v sits at (v % (nx + 1), ...), x fastest)."""
    nx, ny, nz = dims
    mesh = gpu.DeviceMesh.box(nx, ny, nz) if p1 is None else gpu.DeviceMesh.box(nx, ny, nz, p1=p1)
    V = gpu.DeviceSpace(mesh, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=20.0)
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_vector(V, b, source=3.0)
    plane = (nx + 1) * (ny + 1)
    lo, hi = np.arange(plane), nz * plane + np.arange(plane)
    dofs = np.concatenate([lo, hi]).astype(np.int32)
    vals = np.concatenate([np.full(plane, 350.0), np.full(plane, 300.0)])
    A.apply_dirichlet(b, dofs, vals, symmetric=True)
    return mesh, V, A, b


def _solve(gpu, V, A, b, x0=None, **kw):
    x = gpu.DeviceVector(V.n_local)
    if x0 is not None:
        x.set(x0)
    st = gpu.krylov_solve(A, b, x, nonzero_guess=x0 is not None, **kw)
    keep = {k: st[k] for k in ("iterations", "converged", "bnorm", "rel_residual", "true_rel_residual", "row_classes", "fused_iteration")}
    return keep, np.array(gpu.krylov_history()), x.get()[:V.n_owned].copy(), gpu.last_iteration_form() | gpu.last_iteration_guard() << 2


def _both_forms(gpu, run):
    got = {}
    try:
        for guard in (1, 0):
            gpu.set_option("cg_guard", guard)
            got[guard] = run()
    finally:
        gpu.set_option("cg_guard", 1)
    return got[1], got[0]


def _assert_same(new, old, what, bits=GUARD | CENTRE):
    (s1, h1, x1, f1), (s0, h0, x0, f0) = new, old
    assert s1["fused_iteration"] == 1 and s0["fused_iteration"] == 1, what
    assert f1 & PAIR and f0 & PAIR, (what, f1, f0)
    assert f1 & (GUARD | CENTRE) == bits and f0 & (GUARD | CENTRE) == 0, (what, f1, f0)
    assert s1 == s0, (what, s1, s0)
    assert h1.tobytes() == h0.tobytes(), what
    assert x1.tobytes() == x0.tobytes(), (what, int((x1 != x0).sum()))


def _solves(gpu, V, A, b, rtol):
    """The converged solve, the iteration limit at 1, 2, 36 and 37 (odd: the solve stops in a PAIR launch and owes x the step of
    k_cg_pair_flush), a restart from a nonzero guess, the same solve again."""
    out = [_solve(gpu, V, A, b, rtol=rtol, max_iter=5000)]
    for lim in (1, 2, 36, 37):
        out.append(_solve(gpu, V, A, b, rtol=1e-14, max_iter=lim))
    xg = out[0][2].copy()
    xg *= 1.0 + 1e-3 * np.cos(np.arange(V.n_owned))
    guess = np.zeros(V.n_local)
    guess[:V.n_owned] = xg
    out.append(_solve(gpu, V, A, b, x0=guess, rtol=rtol, max_iter=5000))
    out.append(_solve(gpu, V, A, b, rtol=rtol, max_iter=5000))
    return out


NAMES = ["converged", "limit 1", "limit 2", "limit 36", "limit 37", "nonzero guess", "second solve"]


@pytest.mark.parametrize("dims,rtol", BOXES, ids=["x".join(map(str, d)) for d, _ in BOXES])
def test_guarded_vectors_give_the_bits_of_the_edge_item_path(gpu, dims, rtol):
    mesh, V, A, b = _box_system(gpu, dims)
    new, old = _both_forms(gpu, lambda: _solves(gpu, V, A, b, rtol))
    for a, c, what in zip(new, old, NAMES):
        _assert_same(a, c, (dims, what))
    assert new[0][0]["converged"] == 1 and (dims != (40, 40, 40) or new[0][0]["iterations"] > 64)
    for k, lim in zip((1, 2, 3, 4), (1, 2, 36, 37)):
        assert new[k][0]["iterations"] <= lim
        assert dims[1] < 12 or (new[k][0]["iterations"] == lim and new[k][0]["converged"] == 0)
    assert new[6][2].tobytes() == new[0][2].tobytes()


def test_the_every_launch_form_keeps_its_kernel_and_its_bits(gpu):
    """cg_pair = 0: the launches that update p and x every time are not touched by cg_guard - form word 0 on both sides, same bits."""
    mesh, V, A, b = _box_system(gpu, (12, 12, 12))
    gpu.set_option("cg_pair", 0)
    try:
        new, old = _both_forms(gpu, lambda: _solves(gpu, V, A, b, 1e-8))
    finally:
        gpu.set_option("cg_pair", 1)
    for (s1, h1, x1, f1), (s0, h0, x0, f0), what in zip(new, old, NAMES):
        assert s1["fused_iteration"] == 1 and f1 == 0 and f0 == 0, (what, f1, f0)
        assert s1 == s0 and h1.tobytes() == h0.tobytes() and x1.tobytes() == x0.tobytes(), what


def _guard(dims):
    a = dims[0] + 1
    b = a * (dims[1] + 1)
    max_start, min_start = a + b, -(a + b + 1)
    return 32 * -(-(max(-min_start, max_start) + 130) // 32)


def _displace_workspace(gpu):
    """A solve of another size: the next solve allocates its work vectors anew (out of the block cache)."""
    mesh, V, A, b = _box_system(gpu, (6, 6, 6))
    _solve(gpu, V, A, b, rtol=1e-8, max_iter=200)


_zero_filled = {}


def _first_solve_over(gpu, dims, pattern):
    """The first solve on a fresh space whose guarded vectors come out of blocks filled with the pattern."""
    _displace_workspace(gpu)
    mesh, V, A, b = _box_system(gpu, dims)
    n = V.n_owned
    G = _guard(dims)
    _poison(gpu, [n + 2 * G + 1, n + 2 * G + 2], pattern)
    return _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)


@pytest.mark.parametrize("pattern", ["nan", "inf", "ones", "finite"])
@pytest.mark.parametrize("dims", [(12, 12, 12), (30, 7, 5)], ids=["12x12x12", "30x7x5"])
def test_what_the_block_cache_held_does_not_reach_the_solve(gpu, dims, pattern):
    """The whole block of a guarded vector is zeroed when it is made: with NaN, infinities, all-ones bits or random numbers left in
    the cache where the bands (and the two rows behind the last) come to lie, iteration count, history and x are those of a
    zero-filled cache."""
    if dims not in _zero_filled:
        _zero_filled[dims] = _first_solve_over(gpu, dims, "zero")
    s0, h0, x0, f0 = _zero_filled[dims]
    s1, h1, x1, f1 = _first_solve_over(gpu, dims, pattern)
    assert f0 & GUARD and f1 & GUARD and s1["fused_iteration"] == 1, (f0, f1)
    assert s1["converged"] == 1 and np.isfinite(x1).all()
    assert s1["iterations"] == s0["iterations"] and h1.tobytes() == h0.tobytes() and x1.tobytes() == x0.tobytes(), (dims, pattern)


def test_a_space_without_the_centre_run_keeps_the_z_run(gpu):
    """Two Kuhn boxes with integer vertex coordinates glued at a z plane, the upper one mirrored in z: the rows of the two halves and of
    the plane between them have three different offset lists - more than one plan, so the own rows stay with the z run (guard bit
    set, centre-run bit clear) - and the answer equals cg_guard = 0 bit for bit."""
    from oracle import fem_oracle as fo
    nx, ny, nz = 16, 15, 14      # (4080 rows: the dictionary wants at most one class per 16 rows, and this operator has 157)
    coords, cells = fo.box_mesh((0.0, 0.0, 0.0), (float(nx), float(ny), float(nz)), nx, ny, nz)
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cells = np.array(cells, dtype=np.int64)
    plane, a = (nx + 1) * (ny + 1), nx + 1
    upper = coords[cells].mean(axis=1)[:, 2] > nz / 2
    # the cell pattern of the upper half reflected in z about the half's mid-plane: vertex (i, j, k) -> (i, j, nz / 2 + nz - k)
    k = cells // plane
    mirrored = cells - k * plane + (nz // 2 + nz - k) * plane
    cells = np.where(upper[:, None], mirrored, cells).astype(np.int32)
    mesh = gpu.DeviceMesh(coords, cells)
    V = gpu.DeviceSpace(mesh, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=20.0)
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_vector(V, b, source=3.0)
    lo, hi = np.arange(plane), nz * plane + np.arange(plane)
    A.apply_dirichlet(b, np.concatenate([lo, hi]).astype(np.int32), np.concatenate([np.full(plane, 350.0), np.full(plane, 300.0)]), symmetric=True)
    new, old = _both_forms(gpu, lambda: _solves(gpu, V, A, b, 1e-10))
    for c, d, what in zip(new, old, NAMES):
        _assert_same(c, d, ("mirrored half", what), bits=GUARD)
    assert new[0][0]["converged"] == 1
