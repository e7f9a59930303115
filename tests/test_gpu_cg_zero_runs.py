"""The one-launch CG iteration without the two runs that carry only assembly noise (option "cg_zero_runs", k_dict_cg_iter ZRUNS).
On a Kuhn box with orthogonal edges the P1 stiffness entries on the (0, 1, 1) and (1, 1, 1) diagonals vanish - the pure diffusion operator
is the 7-point stencil - and what the assembly leaves in the runs of slots 1 and 7 of a row is the rounding of sums that cancel: below
2^-53 of the unit diagonal of the scaled operator.  The host decides from the class table of the solve itself; an operator with a mass
term fills those diagonals and keeps all seven runs.  Not bit for bit: a row's product loses terms below half an ulp of its diagonal term,
so the automatic mode takes the form from 100 000 rows on only and the tests here force it.

Bounds (none of them measured on the code under test): the perturbation of the operator is dA with |dA| <= 4 * 2^-53 per row against a
unit diagonal, so k iterations move an iterate by about k * cond * 4.4e-16 relative - cond < 3 000 for these boxes, k <= 37: below 5e-11,
asserted as 1e-9.  A converged solve is held to the reference side (oracle/c_oracle.heat_box_solve on the same box): no farther from it
than twice the seven-run form's own distance in the same test."""
import numpy as np
import pytest

from test_gpu_cg_guard import _solve

pytestmark = pytest.mark.gpu

PAIR, DTAB, GUARD, CENTRE = 1, 2, 4, 8       # bits 0, 1 of fs_last_iteration_form, and bits 0, 1 of fs_last_iteration_guard behind them

# 12^3: 18 items; 30 x 7 x 5 and 70 x 5 x 4: items straddle lines and planes, cells that are no cubes; 40^3: more than 64 iterations,
# so captured batches run
BOXES = [(12, 12, 12), (30, 7, 5), (70, 5, 4), (40, 40, 40)]


def _system(gpu, dims, mass=None):
    """The problem of oracle/c_oracle.heat_box_solve: conductivity 20 on the unit box, the two z faces held at 350 and 300, no source."""
    nx, ny, nz = dims
    mesh = gpu.DeviceMesh.box(nx, ny, nz)
    V = gpu.DeviceSpace(mesh, 1)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=20.0, mass=mass)
    b = gpu.DeviceVector(V.n_owned)
    plane = (nx + 1) * (ny + 1)
    dofs = np.concatenate([np.arange(plane), nz * plane + np.arange(plane)]).astype(np.int32)
    A.apply_dirichlet(b, dofs, np.concatenate([np.full(plane, 350.0), np.full(plane, 300.0)]), symmetric=True)
    return mesh, V, A, b


def _with(gpu, value, run):
    gpu.set_option("cg_zero_runs", value)
    try:
        return run(), gpu.last_iteration_runs()
    finally:
        gpu.set_option("cg_zero_runs", -1)


def _rel(a, b):
    return float(np.abs(a - b).max() / np.abs(b).max())


@pytest.mark.parametrize("dims", BOXES, ids=["x".join(map(str, d)) for d in BOXES])
def test_dropping_the_noise_runs_moves_a_solve_by_rounding_only(gpu, dims):
    from oracle import c_oracle
    mesh, V, A, b = _system(gpu, dims)

    def solves():
        out = [_solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)]
        for lim in (1, 2, 36, 37):
            out.append(_solve(gpu, V, A, b, rtol=1e-14, max_iter=lim))
        guess = np.zeros(V.n_local)
        guess[:V.n_owned] = out[0][2] * (1.0 + 1e-3 * np.cos(np.arange(V.n_owned)))
        out.append(_solve(gpu, V, A, b, x0=guess, rtol=1e-10, max_iter=5000))
        out.append(_solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
        return out

    new, runs1 = _with(gpu, 1, solves)
    old, runs0 = _with(gpu, 0, solves)
    assert runs1 == 2 and runs0 == 0, (runs1, runs0)
    ref = c_oracle.heat_box_solve(*dims, rtol=1e-12)["x"]
    names = ["converged", "limit 1", "limit 2", "limit 36", "limit 37", "nonzero guess", "second solve"]
    for (s1, h1, x1, f1), (s0, h0, x0, f0), what in zip(new, old, names):
        print(dims, what, "iterations", s1["iterations"], s0["iterations"], "rel diff x %.3e" % _rel(x1, x0), "to the reference %.3e / %.3e" % (_rel(x1, ref), _rel(x0, ref)))
        assert s1["fused_iteration"] == 1 and s0["fused_iteration"] == 1, what
        assert f1 == f0 == PAIR | DTAB | GUARD | CENTRE, (what, f1, f0)
        assert s1["iterations"] == s0["iterations"] and s1["converged"] == s0["converged"], (what, s1, s0)
        if what.startswith("limit"):
            assert _rel(x1, x0) <= 1e-9 and len(h1) == len(h0) and np.allclose(h1, h0, rtol=1e-9, atol=0.0), what
        else:
            assert s1["converged"] == 1 and _rel(x1, ref) <= 2.0 * _rel(x0, ref), (what, _rel(x1, ref), _rel(x0, ref))
    assert dims != (40, 40, 40) or new[0][0]["iterations"] > 64
    assert new[6][2].tobytes() == new[0][2].tobytes() and new[6][1].tobytes() == new[0][1].tobytes()      # (a second solve repeats the first bit for bit)


def test_an_operator_with_entries_on_those_diagonals_keeps_its_seven_runs(gpu):
    """Stiffness + mass: the P1 mass matrix couples all 14 neighbours of a Kuhn vertex, the runs of slots 1 and 7 carry coefficients.  Forcing
    the option changes nothing then (runs word 0, same bits), and the answer is the two-launch iteration's bit for bit - which it would not
    be with two runs of the product missing."""
    mesh, V, A, b = _system(gpu, (12, 12, 12), mass=7.0)
    new, runs1 = _with(gpu, 1, lambda: _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
    old, runs0 = _with(gpu, 0, lambda: _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
    assert runs1 == 0 and runs0 == 0, (runs1, runs0)
    assert new[0]["fused_iteration"] == 1 and new[3] == PAIR | DTAB | GUARD | CENTRE and new[0]["converged"] == 1
    assert new[0] == old[0] and new[1].tobytes() == old[1].tobytes() and new[2].tobytes() == old[2].tobytes()
    gpu.set_option("cg_fused", 0)
    try:
        two, _ = _with(gpu, 1, lambda: _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
    finally:
        gpu.set_option("cg_fused", -1)
    assert two[0]["fused_iteration"] == 0
    assert new[0]["iterations"] == two[0]["iterations"] and new[1].tobytes() == two[1].tobytes() and new[2].tobytes() == two[2].tobytes()


def test_the_automatic_mode_keeps_the_seven_runs_below_100000_rows(gpu):
    """41^3 = 68 921 rows, diffusion only: the default keeps every run, and with them the bits of the two-launch iteration; the floor of
    the row threshold cannot be lowered."""
    mesh, V, A, b = _system(gpu, (40, 40, 40))
    auto = _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)
    assert auto[0]["fused_iteration"] == 1 and gpu.last_iteration_runs() == 0 and auto[0]["converged"] == 1
    gpu.set_option("cg_fused", 0)
    try:
        two = _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000)
    finally:
        gpu.set_option("cg_fused", -1)
    assert two[0]["fused_iteration"] == 0 and auto[1].tobytes() == two[1].tobytes() and auto[2].tobytes() == two[2].tobytes()
    with pytest.raises(gpu.BackendError):
        gpu.set_option("cg_zero_runs_min_rows", 50000)


def test_the_decision_follows_the_operator_of_each_solve(gpu):
    """Diffusion, the same again (kept class tables), then stiffness + mass on the SAME space (the tables are built anew), forced each time:
    two runs dropped, two, none."""
    mesh, V, A, b = _system(gpu, (12, 12, 12))
    first, r1 = _with(gpu, 1, lambda: _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
    again, r2 = _with(gpu, 1, lambda: _solve(gpu, V, A, b, rtol=1e-10, max_iter=5000))
    assert r1 == 2 and r2 == 2 and again[2].tobytes() == first[2].tobytes()
    A.assemble(stiffness=20.0, mass=7.0)
    b2 = gpu.DeviceVector(V.n_owned)
    plane = 13 * 13
    dofs = np.concatenate([np.arange(plane), 12 * plane + np.arange(plane)]).astype(np.int32)
    A.apply_dirichlet(b2, dofs, np.concatenate([np.full(plane, 350.0), np.full(plane, 300.0)]), symmetric=True)
    with_mass, r3 = _with(gpu, 1, lambda: _solve(gpu, V, A, b2, rtol=1e-10, max_iter=5000))
    assert with_mass[0]["fused_iteration"] == 1 and with_mass[0]["converged"] == 1 and r3 == 0
