"""The prologue of the one-launch CG iteration (k_dict_cg_iter): the dictionary goes into LDS with direct-to-LDS loads issued first,
with GUARD the first item's loads are branch-free (a wave without a first item loads item 0's operands and discards them), the sums
are reduced under the run loads' flight behind ONE barrier.  Nothing changes in operands or summation order: everything a solve returns
equals the two-launch iteration (cg_fused = 0: k_dict_spmv + k_cg_update_scaled, which share no prologue with it) BYTE FOR BYTE.

The dictionary copy moves C S / 2 chunks of 16 bytes, 64 per instruction (C = row_classes of the solve, S = 24 doubles per class row on
every space here: P1, plans of one round of eight runs of up to three offsets - a larger S would not fit the mirrored mesh's 157
classes into the 32 KiB the whole-dictionary form takes).  C as the solves report it (asserted below), chunks = 12 C, what the last
instructions of the copy look like (four waves, 64 chunks each per trip of 256):
    12^3, 24^3, 40^3, 30 x 7 x 5      C =  76    912 chunks = 3 trips + 2 full instructions + one of 16 lanes; the fourth wave issues 3, the others 4
    40 x 3 x 3                        C =  41    492 chunks = 1 trip + 3 full instructions + one of 44 lanes
    mirrored two-half mesh            C = 157   1884 chunks = 7 trips + 1 full instruction + one of 28 lanes; two waves issue 7, two 8
The table of C dot weights behind the dictionary goes the same way in 4-byte chunks (2 C: 152, 82, 314 - none a multiple of 64).
C S / 2 is a multiple of 64 only where 16 divides C.  No such case: twenty small boxes, cubes and slabs from 8^3 to 40^3 with p1 from
(1, 1, 1) to (3, 2, 1) and (1, 3, 3), report 76, 41 or 26 classes or do not take the dictionary form at all (more than one class per
16 rows) - stretching a Kuhn box changes the coefficients, not which rows are alike.  The full-instruction path is exercised by the
first trips of every case above.
"""
import numpy as np
import pytest

from test_gpu_cg_guard import BOXES, NAMES, _box_system, _solve, _solves

pytestmark = pytest.mark.gpu

PAIR, DTAB, GUARD, CENTRE = 1, 2, 4, 8
S = 24


def _with(gpu, options, run):
    """run() under the given options, every one put back to its default afterwards."""
    defaults = {"cg_fused": -1, "cg_guard": 1, "cg_pair": 1}
    try:
        for k, v in options.items():
            gpu.set_option(k, v)
        return run()
    finally:
        for k in options:
            gpu.set_option(k, defaults[k])


def _assert_same(one, two, what, bits):
    """one: the one-launch iteration, with the form word `bits`; two: the two-launch iteration."""
    (s1, h1, x1, f1), (s0, h0, x0, f0) = one, two
    assert s1["fused_iteration"] == 1 and s0["fused_iteration"] == 0, (what, s1, s0)
    assert f1 == bits, (what, f1, bits)
    for k in ("iterations", "converged", "bnorm", "rel_residual", "true_rel_residual", "row_classes"):
        assert np.float64(s1[k]).tobytes() == np.float64(s0[k]).tobytes(), (what, k, s1[k], s0[k])
    assert h1.tobytes() == h0.tobytes(), what
    assert x1.tobytes() == x0.tobytes(), (what, int((x1 != x0).sum()))


def _chunks(c):
    return c * S // 2


def _compare(gpu, V, A, b, rtol, what, bits, options=None, classes=None):
    one = _with(gpu, dict(options or {}), lambda: _solves(gpu, V, A, b, rtol))
    two = _with(gpu, {"cg_fused": 0}, lambda: _solves(gpu, V, A, b, rtol))
    for a, c, name in zip(one, two, NAMES):
        _assert_same(a, c, (what, name), bits)
    assert one[0][0]["converged"] == 1
    assert one[6][2].tobytes() == one[0][2].tobytes(), what
    if classes is not None:
        assert one[0][0]["row_classes"] == classes, (what, one[0][0]["row_classes"])
    return one


# C per box (the header's table)
BOX_CLASSES = {(12, 12, 12): 76, (24, 24, 24): 76, (40, 40, 40): 76, (30, 7, 5): 76, (40, 3, 3): 41}
MIRRORED_CLASSES = 157


@pytest.mark.parametrize("dims,rtol", BOXES, ids=["x".join(map(str, d)) for d, _ in BOXES])
def test_the_one_launch_iteration_gives_the_bits_of_the_two_launch_iteration(gpu, dims, rtol):
    """Converged solve, iteration limits 1, 2, 36, 37, a nonzero guess, the same solve again.  40^3 runs more than 64 iterations:
    captured batches, and the no-op launches behind the stop leave through the early return with their loads into LDS waited for;
    40 x 3 x 3 (6 items) and 12^3 (18 items) have chunks whose last waves have no first item."""
    mesh, V, A, b = _box_system(gpu, dims)
    assert _chunks(BOX_CLASSES[dims]) % 64 != 0
    one = _compare(gpu, V, A, b, rtol, dims, PAIR | DTAB | GUARD | CENTRE, classes=BOX_CLASSES[dims])
    assert dims != (40, 40, 40) or one[0][0]["iterations"] > 64
    for k, lim in zip((1, 2, 3, 4), (1, 2, 36, 37)):
        assert one[k][0]["iterations"] <= lim
        assert dims[1] < 12 or (one[k][0]["iterations"] == lim and one[k][0]["converged"] == 0)


def _mirrored_system(gpu):
    """The two-half mesh of tests/test_gpu_cg_guard.py: two Kuhn boxes glued at a z plane, the upper one mirrored in z - eight plans, so
    the guard bit is set and the centre-run bit clear."""
    from oracle import fem_oracle as fo
    nx, ny, nz = 16, 15, 14
    coords, cells = fo.box_mesh((0.0, 0.0, 0.0), (float(nx), float(ny), float(nz)), nx, ny, nz)
    coords = np.ascontiguousarray(coords, dtype=np.float64)
    cells = np.array(cells, dtype=np.int64)
    plane = (nx + 1) * (ny + 1)
    upper = coords[cells].mean(axis=1)[:, 2] > nz / 2
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
    return mesh, V, A, b


def test_more_than_one_plan_and_no_centre_run(gpu):
    mesh, V, A, b = _mirrored_system(gpu)
    one = _with(gpu, {}, lambda: _solves(gpu, V, A, b, 1e-10))
    two = _with(gpu, {"cg_fused": 0}, lambda: _solves(gpu, V, A, b, 1e-10))
    form = one[0][3]
    assert form & (PAIR | GUARD | CENTRE) == PAIR | GUARD, form
    for a, c, name in zip(one, two, NAMES):
        _assert_same(a, c, ("mirrored half", name), form)
    assert one[0][0]["converged"] == 1
    assert one[0][0]["row_classes"] == MIRRORED_CLASSES


def test_the_unguarded_form_shares_the_prologue(gpu):
    """cg_guard = 0: the first item's loads stay in their branch (edge items take the clamped path), the dictionary and the barrier are
    the new ones.  30 x 7 x 5: half of its items are edge items."""
    mesh, V, A, b = _box_system(gpu, (30, 7, 5))
    _compare(gpu, V, A, b, 1e-10, "cg_guard 0", PAIR | DTAB, options={"cg_guard": 0})


def test_the_every_launch_form_shares_the_prologue(gpu):
    """cg_pair = 0: p and x in every launch, unguarded vectors, the weight stream - form word 0."""
    mesh, V, A, b = _box_system(gpu, (12, 12, 12))
    _compare(gpu, V, A, b, 1e-8, "cg_pair 0", 0, options={"cg_pair": 0})


def test_a_second_operator_in_the_process_finds_nothing_of_the_first(gpu):
    """A solve on the mirrored mesh (157 classes: more chunks than the box's dictionary has) between two solves of the 12^3 box: the
    second equals the first bit for bit."""
    mesh, V, A, b = _box_system(gpu, (12, 12, 12))
    first = _solve(gpu, V, A, b, rtol=1e-8, max_iter=5000)
    m2, V2, A2, b2 = _mirrored_system(gpu)
    other = _solve(gpu, V2, A2, b2, rtol=1e-10, max_iter=5000)
    assert other[0]["fused_iteration"] == 1 and other[0]["converged"] == 1
    second = _solve(gpu, V, A, b, rtol=1e-8, max_iter=5000)
    assert first[0]["fused_iteration"] == 1 and first[3] == PAIR | DTAB | GUARD | CENTRE and second[3] == first[3]
    assert second[0] == first[0] and second[1].tobytes() == first[1].tobytes() and second[2].tobytes() == first[2].tobytes()
