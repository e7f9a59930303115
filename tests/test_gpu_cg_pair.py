"""The one-launch CG iteration with p and x updated every second launch (k_dict_cg_iter LIGHT / PAIR launches, option "cg_pair") and
its dot weights taken from the table by row class: the same fmas on the same operands as the every-launch form, so everything a
solve returns is equal BIT FOR BIT between cg_pair = 1 and cg_pair = 0."""
import numpy as np
import pytest

from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu

PAIR, DTAB = 1, 2       # bits of fs_last_iteration_form


def _box_system(gpu, n, stiffness=20.0):
    mesh = gpu.DeviceMesh.box(n, n, n)
    P = fo.heat_box_problem(n)
    V = gpu.DeviceSpace(mesh, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=stiffness(mesh) if callable(stiffness) else stiffness)
    b = gpu.DeviceVector(V.n_owned)
    gpu.assemble_vector(V, b, source=3.0)
    A.apply_dirichlet(b, P["dofs"], P["vals"], symmetric=True)
    return mesh, V, A, b


def _solve(gpu, V, A, b, x0=None, **kw):
    x = gpu.DeviceVector(V.n_local)
    if x0 is not None:
        x.set(x0)
    st = gpu.krylov_solve(A, b, x, nonzero_guess=x0 is not None, **kw)
    keep = {k: st[k] for k in ("iterations", "converged", "bnorm", "rel_residual", "true_rel_residual", "row_classes", "fused_iteration")}
    return keep, np.array(gpu.krylov_history()), x.get()[:V.n_owned].copy(), gpu.last_iteration_form()


def _both_forms(gpu, run):
    got = {}
    try:
        for pair in (1, 0):
            gpu.set_option("cg_pair", pair)
            got[pair] = run()
    finally:
        gpu.set_option("cg_pair", 1)
    return got[1], got[0]


def _assert_same(new, old, what):
    (s1, h1, x1, f1), (s0, h0, x0, f0) = new, old
    assert s1["fused_iteration"] == 1 and s0["fused_iteration"] == 1, what
    assert f1 & PAIR and f0 == 0, (what, f1, f0)
    assert s1 == s0, (what, s1, s0)
    assert h1.tobytes() == h0.tobytes(), what
    assert x1.tobytes() == x0.tobytes(), (what, int((x1 != x0).sum()))


@pytest.mark.parametrize("n,rtol", [(12, 1e-8), (24, 1e-10), (40, 1e-12)])
def test_pair_launches_are_the_every_launch_iteration_bit_for_bit(gpu, n, rtol):
    """Three boxes, n = 40 beyond 64 iterations so that captured batches run.  Per box: the converged solve, the iteration limit at an
    even and at an odd iteration (the odd one stops in a PAIR launch and owes x the step k_cg_pair_flush applies), a restart from a
    nonzero guess, and the same solve again (class table and dot-weight table kept from the first)."""
    mesh, V, A, b = _box_system(gpu, n)

    def run():
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

    new, old = _both_forms(gpu, run)
    names = ["converged", "limit 1", "limit 2", "limit 36", "limit 37", "nonzero guess", "second solve"]
    for a, c, what in zip(new, old, names):
        _assert_same(a, c, (n, what))
    assert new[0][0]["converged"] == 1 and (n < 40 or new[0][0]["iterations"] > 64)
    for k, lim in zip((1, 2, 3, 4), (1, 2, 36, 37)):
        assert new[k][0]["iterations"] == lim and new[k][0]["converged"] == 0
    assert new[6][2].tobytes() == new[0][2].tobytes()


def test_dot_weights_come_from_the_class_table_on_the_constant_coefficient_box(gpu):
    """Constant coefficient: every row's weight 1 / a_ii equals its class's, the weight stream is not read (bit 1 of
    fs_last_iteration_form) - on the first solve and with the kept tables of the second."""
    mesh, V, A, b = _box_system(gpu, 24)
    for rep in range(2):
        st, h, x, form = _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)
        assert st["fused_iteration"] == 1 and form == PAIR | DTAB, (rep, form)


def test_rows_of_one_class_with_different_weights_keep_the_weight_stream(gpu):
    """Conductivity 20 in the lower half of the box and 80 in the upper: an interior row of the upper half is 4 x the lower one's, the
    factor is a power of two, so the rows of D^-1/2 A D^-1/2 are equal bit for bit - one class - while 1 / a_ii differs by the factor.
    The table is then not used (never an error), and the answer equals the every-launch form's."""
    n = 24

    def stiffness(mesh):
        xyz, cells, _ = mesh.get(want_gids=False)
        zc = xyz[cells].mean(axis=1)[:, 2]
        return ("cell", np.where(zc < 0.5, 20.0, 80.0))

    mesh, V, A, b = _box_system(gpu, n, stiffness)
    new, old = _both_forms(gpu, lambda: _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
    _assert_same(new, old, "two conductivities")
    assert new[0]["converged"] == 1 and new[0]["row_classes"] > 0
    assert new[3] == PAIR, new[3]


def test_a_solve_does_not_depend_on_what_the_search_direction_held_before(gpu):
    """p is filled with NaN before the solve (option cg_poison_p): the pass sets p_{-1} = 0 itself, the LIGHT launch 0 neither reads nor
    writes p, the PAIR launch 1 makes p_0 = r_0 + 0 p_{-1} - x is what it is without the NaN, bit for bit."""
    mesh, V, A, b = _box_system(gpu, 20)
    clean = _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)
    gpu.set_option("cg_poison_p", 1)
    try:
        dirty = _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)
    finally:
        gpu.set_option("cg_poison_p", 0)
    assert clean[3] & PAIR and dirty[3] & PAIR
    assert np.isfinite(dirty[2]).all()
    assert dirty[0] == clean[0] and dirty[1].tobytes() == clean[1].tobytes() and dirty[2].tobytes() == clean[2].tobytes()
