"""fs_krylov_solve's iteration kernels and stopping rules held to a host replay (krylov_reference.py) of the recurrences they state:
BiCGStab (k_bicg_p / k_bicg_s / k_bicg_x, k_dot2_partial, step_bicgstab), the update kernels of the three CG recurrences
(k_cg_update, k_cg_update_scaled, k_pcg_update, k_pcg_dots) on one workgroup and on many, with the sums in the kernel and from
k_sum_partials (cg_fuse_sums = 0), with and without nontemporal accesses (FS_UPDATE_NT), and what k_set_threshold, the status word
and fill_stats report.  The solver recomputes the true residual after every pass and restarts on it, so a wrong beta, an omega from
the wrong parity or a wrong threshold costs iterations and every test that looks at `converged` and the solution stays green.

The operators are jittered boxes, a jittered triangle mesh and one SPD 3 x 3-block operator (krylov_reference.CASES), none of which
takes the row dictionary; the replay gets the device's own matrix (to_csr) and right-hand side.  Every solve is placed: the replay
runs with rtol = atol = 0 in extended precision, in float64 and in float64 with the terms of every dot permuted; envelope() of the
three is how far the history moves when the last bit of a dot does, an entry qualifies while that is at most 1e-8, and rtol is put
in the middle of the largest single-iteration drop among the qualifying entries from entry 20 (CG) or 12 (BiCGStab) on.  So every
entry of a device history qualifies, and test_krylov_reference_host.py holds every case to that on the host.

Held to the replay means: every history entry within 100 x envelope of the extended replay's (the factor of vel_lmax in
test_gpu_saddle_replay.py, over a spread measured on the reference alone), the iteration count the replay's, converged == 1, and
the solution within 100 x the difference of the float64 replay's solution from the extended one's, floored at 64 eps max |x|.

Sizes, by what ONE workgroup of k_cg_update_scaled (update_blocks = 1: stride 256 double2) does with n2 = n >> 1 - the prefetched
trip needs i + 256 < n2, every further two-element trip i + 512 j + 256 < n2, the remainder loop takes what is left one element a
trip, and lane 0 the last row of an odd n:
   n 343   6 x 6 x 6     n2 171  no thread has i + 256 < 171: remainder loop only (threads 0 .. 170), odd tail
   n 729   8 x 8 x 8     n2 364  threads 0 .. 107 (i + 256 < 364) one prefetched trip, threads 108 .. 255 the remainder loop, odd tail
   n 1859  12 x 12 x 10  n2 929  every thread the prefetched trip (elements 0 .. 511); threads 0 .. 160 (i + 768 < 929) a trip that
                                 loads for itself (512 .. 672 and 768 .. 928); threads 161 .. 255 the remainder (673 .. 767); odd tail
   n 1984  30 x 7 x 7    n2 992  the same with threads 0 .. 223 (i + 768 < 992) and 224 .. 255, n even: no tail
k_cg_update, k_pcg_update and the BiCGStab kernels make 1, 2, 4 and 4 (8 for the kernels that go row by row) grid-stride trips there.
With update_blocks = 1024 these sizes get 1, 2, 4 and 4 workgroups (n / 2 + 1 over 256) and every thread at most one trip.

Scaled and unscaled CG take their sums from the product's partials, whose grid update_blocks does not touch, and update element by
element: history, iteration count and x are asserted to be the same arrays at every update_blocks.  Pipelined CG and BiCGStab sum
their own partials per workgroup: held to the replay at every update_blocks.  With cg_fuse_sums = 0 the sums come from
k_sum_partials (1024 threads) instead of wg_sum_partials (256): equal iteration counts and the replay, no bits.  FS_UPDATE_NT changes
loads and stores only: every array of krylov_replay_worker.py equal between the two processes, and equal to this process's.

Stopping rules (729 rows): the threshold is computed here in extended precision and lies a factor 2 or more from the history
entries around it, so `hist[iterations] <= thr < hist[k] for k < iterations` is asserted on the device's own history without a
tolerance.  Passes after a true-residual restart are not covered: no placed tolerance is below 1e-10, nothing restarts."""
# Measured on the MI355X (the whole file: 3.5 s, of which the two worker processes 1.6 s; every test prints its figures with -s).
# Per case: iterations = the replay's in every case; every history entry qualifies (iterations + 1 of them); the largest deviation of
# a history entry over 100 x envelope; the error of x over its tolerance.
#   (a) BiCGStab, Jacobi / none  adv390 15, 0.025, 0.0058 / 33, 0.030, 0.013     adv1859 14, 0.013, 0.010 / 19, 0.037, 0.020
#                                tri375 13, 0.051, 0.015 / 12, 0.016, 0.0027     lame390 22, 0.019, 0.0096 / 18, 0.0087, 0.0032
#   (b) n 343   cg_scaled 24, 0.018, 0.0080   cg_unscaled 24, 0.013, 0.013   pipelined 23, 0.021, 0.016   bicgstab 13, 0.018, 0.010
#       n 729   cg_scaled 27, 0.025, 0.010    cg_unscaled 27, 0.014, 0.0076  pipelined 21, 0.037, 0.0079  bicgstab 16, 0.036, 0.010
#       n 1859  cg_scaled 28, 0.011, 0.013    cg_unscaled 28, 0.012, 0.0091  pipelined 28, 0.074, 0.012   bicgstab 14, 0.038, 0.010
#       n 1984  cg_scaled 37, 0.018, 0.0083   cg_unscaled 37, 0.018, 0.0066  pipelined 37, 0.020, 0.013   bicgstab 12, 0.024, 0.0076
#       (the larger of update_blocks 1, 2, 1024 for pipelined CG and BiCGStab, whose figures move with the grid: 0.0102 to 0.0204 for
#       pipelined CG at n 1984; scaled and unscaled CG: the same arrays at every update_blocks, as asserted - no loop rounds differently)
#   (c) cg_fuse_sums = 0, n 1859: the figures of (b) to the digits printed, the same iteration counts
#   (d) FS_UPDATE_NT 0 / 1: 56 arrays equal, and equal to this process's at update_blocks 1
#   (e) stops (iterations, hist[it] / thr, smallest earlier entry / thr): scaled and unscaled CG 27, 0.408, 2.450 (both set: 23, 0.409,
#       2.447); BiCGStab 16, 0.291, 3.431 (both set: 7, 0.292, 3.425); pipelined 8, 0.412, 2.427; preconditioned norm: scaled 23,
#       0.412, 2.424, pipelined 8, 0.418, 2.392.  bnorm equal to the host's sqrt(bb) bit for bit in all six cases, rel_residual within
#       2.2e-16 relative, |true_rel_residual - host| at most 0.0014 of the bound.  max_iter = 7: history / (100 envelope) 0.010 to
#       0.030, x 0.0061 to 0.010 of its tolerance; the twelve (cg_mirror, cg_graph, batch) runs: one history, one x.
#       Random guess: 28 / 28 / 17 iterations, 0.0099 / 0.0099 / 0.029, x 0.016 / 0.012 / 0.012.
# Four deliberate mistakes in scratch builds of fs_krylov.hip (none changes an address or a loop bound), each against this file and
# against tests/test_gpu_kernels.py (76 tests):
#   `prefetched = false` removed in k_cg_update_scaled   here: 4 tests fail - scaled CG at n 1859 and 1984 with update_blocks 1 and 2,
#                                                        fused and unfused sums and in the worker, breaks down at iteration 19 / 34
#                                                        (n 729, whose threads make one prefetched trip and no second, passes);
#                                                        existing: all 76 pass
#   bscal[iter & 1] for bscal[(iter - 1) & 1] in         here: every BiCGStab solve, 17 tests; existing: 3 of 76 fail - the slot holds the
#   k_bicg_p                                             zero begin_pass wrote, beta is infinite, breakdown at iteration 1
#   atol for atol * atol in k_set_threshold              here: the `atol` plan of all six stopping cases (16 iterations for 27, 9 for 16,
#                                                        6 for 8, 14 for 23); existing: all 76 pass
#   the weight of the preconditioned norm left as d      here: both preconditioned cases, history 2.7e13 x (100 envelope) from entry 0;
#   (1 / d only for bb)                                  existing: all 76 pass
import os
import subprocess
import sys

import numpy as np
import pytest

import krylov_reference as kr
from krylov_replay_worker import SIZE_KINDS, case_of, device_operator, device_solve

pytestmark = pytest.mark.gpu
LD = np.longdouble
EPS = kr.EPS
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 120
DEFAULTS = {"cg_fused": -1, "update_blocks": 1024, "cg_fuse_sums": 1, "cg_graph": -1, "cg_batch": 32, "cg_mirror": 1}
_OPS, _REFS, _RUNS = {}, {}, {}
_children, _failed = {}, []


class _options:
    """cg_fused = 0 and the given options for the block, the defaults behind it"""

    def __init__(self, gpu, **kw):
        self.gpu, self.kw = gpu, dict(kw, cg_fused=0)

    def __enter__(self):
        for k, v in self.kw.items():
            self.gpu.set_option(k, v)

    def __exit__(self, *exc):
        for k in self.kw:
            self.gpu.set_option(k, DEFAULTS[k])


def _op(gpu, name):
    if name not in _OPS:
        _OPS[name] = device_operator(gpu, name)
    return _OPS[name]


def _ref(gpu, name, kind, point=0, k_min=None, **kw):
    """The placed solve of (case, kind): {"rtol", "k", "thr", "factor", "bb", "R": the three replays at that rtol, "P": placed()}.
    Computed once from the device's matrix and right-hand side and shared."""
    key = (name, kind, point, k_min, tuple(sorted((k, v if isinstance(v, str) else id(v)) for k, v in kw.items())))
    if key not in _REFS:
        op = _op(gpu, name)
        P = kr.placed(kind, op["csr"], op["bh"], k_min=k_min, **kw)
        k, thr, factor = P["points"][point]
        rtol = kr.rtol_for(thr, P["bb"])
        _REFS[key] = {"rtol": rtol, "k": k, "thr": thr, "factor": factor, "bb": P["bb"], "P": P,
                      "R": kr.replays(kind, op["csr"], op["bh"], rtol=rtol, max_iter=kr.PLACE_ITERATIONS, **kw)}
    return _REFS[key]


def _hold_history(tag, hist, h_ref, env):
    """every entry of the device history within 100 x envelope of the extended replay's; -> the largest deviation / (100 envelope)"""
    m = len(hist)
    assert m <= len(h_ref) and m <= len(env), (tag, m, len(h_ref))
    assert np.all(env[:m] <= kr.QUALIFY), (tag, "an entry that does not qualify", env[:m].max())
    dev = np.abs(hist.astype(LD) / h_ref[:m] - 1).astype(np.float64)
    ratio = dev / (100.0 * env[:m])
    assert np.all(ratio <= 1.0), (tag, int(np.argmax(ratio)), float(ratio.max()), dev[:8])
    return float(ratio.max())


def _hold(tag, st, hist, x, ref):
    h_ld, it_ld, status_ld, x_ld = ref["R"]["ld"]
    x_64 = ref["R"]["f64"][3]
    assert status_ld == 1 and it_ld == ref["k"]
    worst = _hold_history(tag, hist, h_ld, ref["R"]["env"])
    xtol = max(100.0 * float(np.abs(x_64 - x_ld).max()), 64 * EPS * float(np.abs(x_ld).max()))
    xerr = float(np.abs(x - x_ld).max())
    print("%-34s iterations %3d entries %3d  history / (100 env) %.3g  x err / tol %.3g" % (tag, st["iterations"], len(hist), worst, xerr / xtol))
    assert st["iterations"] == it_ld and len(hist) == it_ld + 1, (tag, st["iterations"], it_ld)
    assert st["converged"] == 1, (tag, st)
    assert xerr <= xtol, (tag, xerr, xtol)


def _run(gpu, n, kind, blocks, fuse=1):
    """the placed solve of `kind` at size n with update_blocks = blocks, once per process"""
    key = (n, kind, blocks, fuse)
    if key not in _RUNS:
        name = case_of(n, kind)
        ref = _ref(gpu, name, kind)
        with _options(gpu, update_blocks=blocks, cg_fuse_sums=fuse):
            _RUNS[key] = device_solve(gpu, _op(gpu, name), kind, rtol=ref["rtol"], max_iter=kr.PLACE_ITERATIONS)
    return _RUNS[key]


# ---- (a) BiCGStab against the replay ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["bicgstab", "bicgstab_none"])
@pytest.mark.parametrize("name", ["adv390", "adv1859", "tri375", "lame390"])
def test_bicgstab_against_the_replay(gpu, name, kind):
    op = _op(gpu, name)
    A = op["csr"]
    asym = abs(A - A.T).max() / abs(A).max()
    if name == "lame390":
        assert asym <= 1e-12
    else:
        assert asym > 1e-3, (name, asym)
    ref = _ref(gpu, name, kind)
    assert ref["k"] >= 12 and ref["factor"] >= kr.PLACE_FACTOR
    with _options(gpu):
        st, hist, x = device_solve(gpu, op, kind, rtol=ref["rtol"], max_iter=kr.PLACE_ITERATIONS)
    _hold("%s %s" % (name, kind), st, hist, x, ref)


# ---- (b) one workgroup against many ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", kr.SIZES)
def test_one_workgroup_against_many(gpu, n):
    grids = (1, 2, 1024) if n == max(kr.SIZES) else (1, 1024)
    for kind in SIZE_KINDS:
        ref = _ref(gpu, case_of(n, kind), kind)
        assert ref["k"] >= kr.MIN_ENTRIES[kind] and ref["factor"] >= kr.PLACE_FACTOR
        runs = {g: _run(gpu, n, kind, g) for g in grids}
        for g, (st, hist, x) in runs.items():
            if kind in ("pipelined", "bicgstab") or g == 1024:
                _hold("n %d %s update_blocks %d" % (n, kind, g), st, hist, x, ref)
        if kind in ("cg_scaled", "cg_unscaled"):
            st0, hist0, x0 = runs[1024]
            for g, (st, hist, x) in runs.items():
                assert st["iterations"] == st0["iterations"], (n, kind, g)
                assert np.array_equal(hist, hist0), (n, kind, g, int((hist != hist0).sum()))
                assert np.array_equal(x, x0), (n, kind, g, int((x != x0).sum()), float(np.abs(x - x0).max()))


# ---- (c) the sums from k_sum_partials -------------------------------------------------------------------------------------------------
def test_unfused_sums_on_one_gpu(gpu):
    n = 1859
    for kind in SIZE_KINDS:
        ref = _ref(gpu, case_of(n, kind), kind)
        for g in (1, 1024):
            st, hist, x = _run(gpu, n, kind, g, fuse=0)
            _hold("n %d %s update_blocks %d unfused" % (n, kind, g), st, hist, x, ref)
            assert st["iterations"] == _run(gpu, n, kind, g)[0]["iterations"]


# ---- (d) FS_UPDATE_NT ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("krylov_replay")


def _child(gpu, workdir, nt):
    if nt in _children:
        return _children[nt]
    if _failed:
        pytest.fail("not started: the child FS_UPDATE_NT=%s failed before" % _failed[0])
    rtols = str(workdir / "rtols.npz")
    if not os.path.exists(rtols):
        np.savez(rtols, **{"%d/%s" % (n, kind): _ref(gpu, case_of(n, kind), kind)["rtol"] for n in kr.SIZES for kind in SIZE_KINDS})
    env = {k: v for k, v in os.environ.items() if k not in ("FS_UPDATE_NT", "FS_CG_FUSED", "FS_CG_PIPELINED", "FS_CG_GRAPH", "FS_CG_BATCH")}
    env["FS_UPDATE_NT"] = nt
    f = str(workdir / ("nt%s.npz" % nt))
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "krylov_replay_worker.py"), f, rtols], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _failed.append(nt)
        pytest.fail("FS_UPDATE_NT=%s: no end after %d s\n%s" % (nt, CHILD_TIMEOUT, (e.stdout or b"").decode(errors="replace")[-3000:]))
    log = p.stdout.decode(errors="replace")
    if p.returncode != 0:
        _failed.append(nt)
        pytest.fail("FS_UPDATE_NT=%s: exit status %d\n%s" % (nt, p.returncode, log[-3000:]))
    assert log.rstrip().endswith("ok"), log[-3000:]
    with np.load(f) as z:
        _children[nt] = {k: z[k] for k in z.files}
    return _children[nt]


def test_nontemporal_updates_change_no_bit(gpu, workdir):
    a = _child(gpu, workdir, "0")
    b = _child(gpu, workdir, "1")
    assert sorted(a) == sorted(b) and len(a) == 8 + 3 * len(kr.SIZES) * len(SIZE_KINDS)
    for k in a:
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (k, int((a[k] != b[k]).sum()))
    # ... and what this process computes with one workgroup (no vector here is large enough for nontemporal accesses)
    for n in kr.SIZES:
        for kind in SIZE_KINDS:
            assert np.array_equal(a[case_of(n, kind) + "/values"], _op(gpu, case_of(n, kind))["csr"].data)
            st, hist, x = _run(gpu, n, kind, 1)
            tag = "%d/%s" % (n, kind)
            assert int(a[tag + "/iterations"]) == st["iterations"] and np.array_equal(a[tag + "/hist"], hist) and np.array_equal(a[tag + "/x"], x), tag


# ---- (e) stopping rules and stats ---------------------------------------------------------------------------------------------------
STOP_CASES = [("box729", "cg_scaled", "unpreconditioned"), ("box729", "cg_unscaled", "unpreconditioned"), ("adv729", "bicgstab", "unpreconditioned"),
              ("box729", "pipelined", "unpreconditioned"), ("box729", "cg_scaled", "preconditioned"), ("box729", "pipelined", "preconditioned")]


def _norm_kw(norm):
    return {} if norm == "unpreconditioned" else {"norm": norm}


def _weights(op, norm):
    """the weights of the residual norm: 1 or 1 / d, in extended precision"""
    return LD(1) / op["csr"].diagonal().astype(LD) if norm == "preconditioned" else np.ones(op["n"], LD)


def _stops_at_the_threshold(tag, st, hist, thr, k):
    """the first entry at or below the threshold and not before, on the device's own history"""
    it = st["iterations"]
    print("%-52s iterations %3d  hist[it] / thr %.3f  min(hist[:it]) / thr %.3f" % (tag, it, float(hist[it] / thr), float(hist[:it].min() / thr)))
    assert st["converged"] == 1 and it == k and len(hist) == it + 1, (tag, st["converged"], it, k, len(hist))
    assert hist[it] <= thr and np.all(hist[:it] > thr), (tag, hist[it], thr)


@pytest.mark.parametrize("name,kind,norm", STOP_CASES)
def test_stopping_rules_and_stats(gpu, name, kind, norm):
    op = _op(gpu, name)
    kw = _norm_kw(norm)
    first, second = _ref(gpu, name, kind, 0, 3, **kw), _ref(gpu, name, kind, 1, 3, **kw)
    assert first["factor"] >= 2.0 and second["factor"] >= 2.0 and first["k"] != second["k"]
    bb = first["bb"]
    hi, lo = (first, second) if first["thr"] > second["thr"] else (second, first)       # (the larger threshold stops first)
    tag = "%s %s %s" % (name, kind, norm)
    # rtol only, atol only, both set
    plans = [("rtol", first["rtol"], 0.0, first["k"]), ("atol", 0.0, float(np.sqrt(first["thr"])), first["k"]),
             ("rtol > atol", hi["rtol"], float(np.sqrt(lo["thr"])), hi["k"]), ("atol > rtol", lo["rtol"], float(np.sqrt(hi["thr"])), hi["k"])]
    free = first["P"]["free"]
    with _options(gpu):
        for what, rtol, atol, k in plans:
            st, hist, x = device_solve(gpu, op, kind, rtol=rtol, atol=atol, max_iter=kr.PLACE_ITERATIONS, **kw)
            thr = max(LD(rtol) * LD(rtol) * bb, LD(atol) * LD(atol))
            _stops_at_the_threshold(tag + " " + what, st, hist, thr, k)
            _hold_history(tag + " " + what, hist, free["ld"][0], free["env"])
            if what != "rtol":
                continue
            # what the stats say, against the host
            bnorm = float(np.sqrt(bb))
            assert abs(st["bnorm"] - bnorm) <= 4 * EPS * bnorm, (tag, st["bnorm"], bnorm)
            rel = float(np.sqrt(LD(hist[st["iterations"]]) / (LD(st["bnorm"]) * LD(st["bnorm"]))))
            assert abs(st["rel_residual"] - rel) <= 4 * EPS * rel, (tag, st["rel_residual"], rel)
            A = op["csr"]
            wt = _weights(op, norm)
            bl, xl = op["bh"].astype(LD), x.astype(LD)
            r = bl - kr._Op(A, LD) @ xl
            true_rel = float(np.sqrt(((wt * r) ** 2).sum() / bb))
            size = np.abs(bl) + kr._Op(abs(A), LD) @ np.abs(xl)
            bound = float((np.diff(A.indptr).max() + 2) * EPS * np.sqrt(((wt * size) ** 2).sum() / bb))
            print("%-52s bnorm %.1e  rel_residual %.1e  true_rel_residual %.3e against %.3e, |difference| / bound %.3g" % (
                tag, abs(st["bnorm"] / bnorm - 1), abs(st["rel_residual"] / rel - 1), st["true_rel_residual"], true_rel,
                abs(st["true_rel_residual"] - true_rel) / bound))
            assert abs(st["true_rel_residual"] - true_rel) <= bound, (tag, st["true_rel_residual"], true_rel, bound)


def test_iteration_limit_and_batches(gpu):
    """rtol = atol = 0, max_iter = 7: seven iterations, the eighth history entry from the launch that only checks, converged == 0;
    scaled CG with every batch length as plain launches and as captured graphs (which read their limit from the device): one history
    and one x.  cg_mirror = 0 makes the batches of 1 and 3 real graph launches (with the progress words a batch is cg_sub = 16
    launches, more than this solve has)."""
    for name, kind in (("box729", "cg_scaled"), ("box729", "cg_unscaled"), ("box729", "pipelined"), ("adv729", "bicgstab")):
        free = _ref(gpu, name, kind, 0, 3)["P"]["free"]
        with _options(gpu):
            st, hist, x = device_solve(gpu, _op(gpu, name), kind, rtol=0.0, atol=0.0, max_iter=7)
        assert st["iterations"] == 7 and st["converged"] == 0 and len(hist) == 8, (kind, st["iterations"], st["converged"], len(hist))
        worst = _hold_history("%s %s max_iter 7" % (name, kind), hist, free["ld"][0], free["env"])
        R7 = kr.replays(kind, _op(gpu, name)["csr"], _op(gpu, name)["bh"], rtol=0.0, atol=0.0, max_iter=7)
        (h7, it7, status7, x_ld), x_64 = R7["ld"], R7["f64"][3]
        assert it7 == 7 and status7 == 3 and np.array_equal(h7, free["ld"][0][:8])
        xtol = max(100.0 * float(np.abs(x_64 - x_ld).max()), 64 * EPS * float(np.abs(x_ld).max()))          # (as in _hold)
        xerr = float(np.abs(x - x_ld).max())
        print("%s %s max_iter 7: history / (100 env) %.3g, x err / tol %.3g" % (name, kind, worst, xerr / xtol))
        assert xerr <= xtol, (kind, xerr, xtol)
        if kind != "cg_scaled":
            continue
        for mirror in (1, 0):
            for graph in (0, 1):
                for batch in (1, 3, 32):
                    with _options(gpu, cg_graph=graph, cg_mirror=mirror):
                        st2, hist2, x2 = device_solve(gpu, _op(gpu, name), kind, rtol=0.0, atol=0.0, max_iter=7, batch=batch)
                    what = (mirror, graph, batch)
                    assert st2["iterations"] == 7 and st2["converged"] == 0, (what, st2)
                    assert np.array_equal(hist2, hist) and np.array_equal(x2, x), (what, int((hist2 != hist).sum()), int((x2 != x).sum()))


@pytest.mark.parametrize("kind", ["cg_scaled", "cg_unscaled", "bicgstab"])
def test_nonzero_guess(gpu, kind):
    name = case_of(729, kind)
    op = _op(gpu, name)
    # a random guess: the history from the same x0
    x0 = np.random.default_rng(17).standard_normal(op["n"])
    ref = _ref(gpu, name, kind, x0=x0)
    assert ref["k"] >= kr.MIN_ENTRIES[kind] and ref["factor"] >= kr.PLACE_FACTOR
    with _options(gpu):
        st, hist, x = device_solve(gpu, op, kind, x0=x0, rtol=ref["rtol"], max_iter=kr.PLACE_ITERATIONS)
        _hold("%s %s random guess" % (name, kind), st, hist, x, ref)
        # the solution of a finished solve as the guess of a solve ten times looser: nothing to do
        zero = _ref(gpu, name, kind)
        _, _, xs = device_solve(gpu, op, kind, rtol=zero["rtol"], max_iter=kr.PLACE_ITERATIONS)
        st2, hist2, x2 = device_solve(gpu, op, kind, x0=xs, rtol=10 * zero["rtol"], max_iter=kr.PLACE_ITERATIONS)
    assert st2["iterations"] == 0 and st2["converged"] == 1 and len(hist2) == 1, st2
    if kind == "cg_scaled":            # x / (1 / sqrt d) going in, (1 / sqrt d) x coming out: two roundings
        assert np.all(np.abs(x2 - xs) <= 2 * EPS * np.abs(xs)), float((np.abs(x2 - xs) / np.abs(xs)).max() / EPS)
    else:
        assert np.array_equal(x2, xs)

