"""krylov_reference.py itself, without a GPU: the replays solve the systems, agree with the oracle's recurrences where both exist
and with each other where they state the same recurrence twice, and every case test_gpu_krylov_replay.py runs qualifies - its
history is insensitive enough to the last bit of a dot (envelope <= 1e-8) over enough entries for a device comparison to mean
something, and every threshold the device tests are going to place lies well away from the history entries around it.

Measured here (extended / float64 / permuted float64 iterations at rtol 1e-10, qualifying entries of the free replay, the placed
stopping point and its factor):
  box343  cg_scaled 35/35/35, 36, k 32 x2.65     pipelined 23 qualifying, k 21 x2.28      box729  cg_scaled 29/29/29, k 27 x2.45; pipelined 26, k 23 x2.45
  box1859 cg_scaled 41/41/41, k 47 x1.93     pipelined 33, k 28 x1.90                 box1984 cg_scaled 68/68/68, k 37 x1.49; pipelined 46, k 37 x1.49
  adv390 (mass 500) BiCGStab 16/16/16 iterations, every entry within 1e-11; adv1176 (27 x 6 x 5) 34/34/34, 24 entries within 1e-8
  BiCGStab, Jacobi / none: adv343 17 / 30 qualifying, adv729 21 / 24, adv1859 22 / 23, adv1984 23 / 30, tri375 22 / 35, lame390 23 / 23"""
import numpy as np
import pytest
import scipy.sparse as sp
import scipy.sparse.linalg as spla

import krylov_reference as kr
from oracle import fem_oracle as fo

LD = np.longdouble
CG_KINDS = ("cg_scaled", "cg_unscaled", "pipelined")
# (case, kind) of every device comparison: the CG recurrences and BiCGStab on the four sizes, BiCGStab with and without Jacobi on
# the operators of test_bicgstab_against_the_replay
DEVICE_CASES = ([("box%d" % n, kind) for n in kr.SIZES for kind in CG_KINDS] + [("adv%d" % n, "bicgstab") for n in kr.SIZES] +
                [(name, kind) for name in ("adv390", "adv1859", "tri375", "lame390") for kind in ("bicgstab", "bicgstab_none")])
# the stopping rule is asserted on these, with the norm of the threshold
STOP_CASES = [("box729", "cg_scaled", "unpreconditioned"), ("box729", "cg_unscaled", "unpreconditioned"), ("adv729", "bicgstab", "unpreconditioned"),
              ("box729", "pipelined", "unpreconditioned"), ("box729", "cg_scaled", "preconditioned"), ("box729", "pipelined", "preconditioned")]
_OPS = {}


def _op(name):
    if name not in _OPS:
        A = kr.host_operator(name)
        assert A.shape[0] == kr.ROWS[name]
        _OPS[name] = (A, kr.rhs_of(name))
    return _OPS[name]


def test_operators_are_what_the_cases_say():
    for name in kr.CASES:
        A, _ = _op(name)
        asym = abs(A - A.T).max() / abs(A).max()
        if name.startswith(("adv", "tri")):
            assert asym > 1e-3, (name, asym)
        else:
            assert asym < 1e-14, (name, asym)
            assert spla.eigsh(A, k=1, which="SA", return_eigenvectors=False)[0] > 0.0, name
    assert sorted(kr.ROWS[n] for n in ("box343", "box729", "box1859", "box1984")) == list(kr.SIZES)


@pytest.mark.parametrize("name", list(kr.CASES))
def test_extended_replays_reach_the_direct_solution(name):
    A, b = _op(name)
    xs = spla.spsolve(A.tocsc(), b)
    kinds = ("bicgstab", "bicgstab_none") if name.startswith(("adv", "tri")) else CG_KINDS + ("cg_none", "bicgstab", "bicgstab_none")
    for kind in kinds:
        fn, fixed = kr.KINDS[kind]
        h, it, status, x = fn(A, b, rtol=1e-13, max_iter=400, dtype=LD, **fixed)
        err = float(np.abs(x - xs).max() / np.abs(xs).max())
        print(name, kind, "iterations", it, "max |x - x_direct| / max |x| %.2e" % err)
        assert status == 1 and len(h) == it + 1 and h[it] <= LD(1e-26) * (LD(b) * LD(b)).sum() < h[:it].min()
        # ||x - x*|| <= ||A^-1|| ||r||: the mass term bounds the smallest singular value from below; 1e-9 leaves four digits
        assert err <= 1e-9, (name, kind, err)


@pytest.mark.parametrize("name", ["box%d" % n for n in kr.SIZES])
def test_cg_replay_is_the_oracles_recurrence(name):
    """float64, zero guess, rtol only: the common ground of cg_replay and the oracle's two recurrences.  The row sums and dots are
    added in another order (BLAS, scipy), so not bit for bit: 1e-12 relative on every history entry and on x."""
    A, b = _op(name)
    for kind, oracle in (("cg_unscaled", fo.pcg_jacobi_single_reduction), ("pipelined", fo.pcg_jacobi_pipelined)):
        fn, fixed = kr.KINDS[kind]
        xo, ito, ho = oracle(A, b, rtol=1e-6)
        R = kr.replays(kind, A, b, rtol=1e-6)
        h, it, status, x = R["f64"]
        assert it == ito and status == 1 and len(h) == len(ho)
        dev = np.abs(h / np.asarray(ho) - 1.0)
        # the pipelined recurrence amplifies a last-bit change of a dot by itself (box343: its two float64 replays are 1e-10
        # apart at entry 18, and so are replay and oracle): 1e-12 holds where the envelope leaves room for it, 100 x the
        # envelope everywhere
        ground = R["env"] <= 1e-13
        print(name, kind, "iterations", it, "history %.2e over %d entries, %.2e over all" % (dev[ground].max(), ground.sum(), dev.max()),
              "x %.2e" % float(np.abs(x - xo).max() / np.abs(xo).max()))
        assert ground.sum() >= (len(h) if kind == "cg_unscaled" else 8)
        assert np.all(dev[ground] <= 1e-12) and np.all(dev <= 100 * R["env"]) and np.abs(x - xo).max() <= 1e-12 * np.abs(xo).max()
        # the iteration limit only checks
        h2, it2, status2, _ = fn(A, b, rtol=1e-6, max_iter=5, dtype=np.float64, **fixed)
        _, ito2, ho2 = oracle(A, b, rtol=1e-6, maxit=5)
        assert it2 == ito2 == 5 and status2 == 3 and len(h2) == 6 and np.array_equal(h2, h[:6])


@pytest.mark.parametrize("name", ["box%d" % n for n in kr.SIZES])
def test_scaled_and_unscaled_forms_give_one_history(name):
    """Jacobi-PCG on A and CG on D^-1/2 A D^-1/2 are one recurrence: in extended precision their histories agree to the envelope
    of either, entry by qualifying entry; the preconditioned norm is the same iteration with another weight."""
    A, b = _op(name)
    Rs, Ru = kr.replays("cg_scaled", A, b, rtol=1e-10), kr.replays("cg_unscaled", A, b, rtol=1e-10)
    hs, hu = Rs["ld"][0], Ru["ld"][0]
    assert Rs["ld"][1] == Ru["ld"][1] and len(hs) == len(hu)
    env = np.maximum(Rs["env"], Ru["env"])
    q = env <= kr.QUALIFY
    dev = np.abs(hs / hu - 1).astype(np.float64)
    print(name, "iterations", Rs["ld"][1], "qualifying", int(q.sum()), "largest deviation / envelope %.2e" % float((dev[q] / env[q]).max()))
    assert q.sum() >= 20 and np.all(dev[q] <= env[q])
    assert np.abs(Rs["ld"][3] - Ru["ld"][3]).max() <= 64 * kr.EPS * np.abs(Ru["ld"][3]).max()
    # preconditioned norm: sum r^2 / d^2 of the unscaled residual, which the unscaled form does not compute: from the iterates
    hp, itp, _, _ = kr.cg_replay(A, b, norm="preconditioned", rtol=0.0, max_iter=10, dtype=LD)
    d = LD(1) / A.diagonal().astype(LD)
    x = np.zeros(len(b), LD)
    op = kr._Op(A, LD)
    for k in range(4):
        _, _, _, x = kr.cg_replay(A, b, jacobi=True, diagonal_scale=False, rtol=0.0, max_iter=k, dtype=LD)
        r = b.astype(LD) - op @ x
        assert abs(((d * r) ** 2).sum() / hp[k] - 1) <= 1e-15, (name, k)
    assert itp == 10 and len(hp) == 11


@pytest.mark.parametrize("name,kind", DEVICE_CASES)
def test_every_device_case_qualifies(name, kind):
    """What a device comparison rests on: the three replays agree in the iteration count at rtol 1e-10 wherever the whole history
    qualifies, at least MIN_ENTRIES entries of the free history qualify, and the solve the device test places (the largest
    single-iteration drop at entry MIN_ENTRIES or later, still qualifying) has its threshold a factor PLACE_FACTOR away from the
    entries around it: a device history within 100 x 1e-8 of the replay's cannot stop anywhere else."""
    A, b = _op(name)
    P = kr.placed(kind, A, b)
    env = P["free"]["env"]
    n_q = int(np.argmax(env > kr.QUALIFY)) if (env > kr.QUALIFY).any() else len(env)
    assert n_q >= kr.MIN_ENTRIES[kind] + 1, (name, kind, n_q)
    assert P["points"], (name, kind)
    k, thr, factor = P["points"][0]
    print(name, kind, "qualifying entries", n_q, "placed stop at", k, "factor %.2f" % float(factor), "rtol %.3e" % kr.rtol_for(thr, P["bb"]))
    assert k >= kr.MIN_ENTRIES[kind] and factor >= kr.PLACE_FACTOR
    R = kr.replays(kind, A, b, rtol=kr.rtol_for(thr, P["bb"]), max_iter=kr.PLACE_ITERATIONS)
    for which in ("ld", "f64", "perm"):
        h, it, status, _ = R[which]
        assert (it, status, len(h)) == (k, 1, k + 1), (name, kind, which, it, status)
    assert np.all(R["env"] <= kr.QUALIFY)
    assert np.array_equal(R["ld"][0], P["free"]["ld"][0][:k + 1])             # (the same recurrence, stopped)


def test_issue_figures_of_bicgstab():
    """The two boxes the BiCGStab cases were sized on (stiffness 1.7, mass 500, velocity (3, -2, 1), rtol 1e-10)."""
    A, b = _op("adv390")
    R = kr.replays("bicgstab", A, b, rtol=1e-10)
    assert [R[w][1] for w in ("ld", "f64", "perm")] == [16, 16, 16] and np.all(R["env"] <= 1e-11)
    A, b = _op("adv1176")
    R = kr.replays("bicgstab", A, b, rtol=1e-10)
    assert [R[w][1] for w in ("ld", "f64", "perm")] == [34, 34, 34] and int((R["env"] <= kr.QUALIFY).sum()) >= 22


@pytest.mark.parametrize("name,kind,norm", STOP_CASES)
def test_stopping_thresholds_are_a_factor_two_from_their_neighbours(name, kind, norm):
    """Two thresholds per case (relative and absolute tolerance, and both set: the larger one wins), each in the middle of a
    single-iteration drop of at least a factor 4: the device's stopping assertions take no tolerance."""
    A, b = _op(name)
    kw = {} if norm == "unpreconditioned" else {"norm": norm}
    P = kr.placed(kind, A, b, k_min=3, **kw)
    assert len(P["points"]) >= 2
    h = P["free"]["ld"][0]
    for k, thr, factor in P["points"][:2]:
        print(name, kind, norm, "stop at", k, "factor %.2f" % float(factor))
        assert factor >= 2.0 and h[k] * 2 <= thr and np.all(h[:k] >= 2 * thr)
    assert P["points"][0][0] != P["points"][1][0]


def test_envelope_and_breakdown():
    h = np.array([4.0, 2.0, 1.0], LD)
    env = kr.envelope(h, np.array([4.0, 2.0 * (1 + 1e-9), 1.0]), np.array([4.0 * (1 - 1e-12), 2.0, 1.0, 0.5]))
    assert env.dtype == np.float64 and len(env) == 3 and np.allclose(env, [1e-12, 1e-9, 1e-9], rtol=1e-3)
    assert np.array_equal(kr.envelope(h, h, h), np.full(3, kr.EPS))
    # an indefinite operator: the device's code 2, at the iteration whose alpha is not positive
    A = sp.diags([1.0, -1.0, 2.0]).tocsr()
    h, it, status, _ = kr.cg_replay(A, np.ones(3), jacobi=False, diagonal_scale=False, dtype=np.float64)
    assert status == 2 and len(h) == it + 1
    # omega = 0 where t . t = 0 (s = 0: x + alpha y is exact): the identity converges in one iteration without a NaN
    h, it, status, x = kr.bicgstab_replay(sp.identity(4, format="csr"), np.arange(1.0, 5.0), dtype=np.float64)
    assert (it, status) == (1, 1) and np.array_equal(x, np.arange(1.0, 5.0)) and h[1] == 0.0
