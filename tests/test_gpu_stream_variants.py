"""The variants of the streaming product (fs_krylov_stream.inc, product kind 0) that launch_spmv picks by problem size, forced at
small sizes through the switches that pin them: FS_SPMV_PAIRS (k_dia_pair_spmv on the paired DIA slices + k_sell_spmv on the rest,
one partials array), FS_SPMV_NT (nontemporal loads), FS_PAIR_BLOCKS, and the options spmv_unroll (2 / 4 / 8 / 16: another
row_tail each), spmv_unroll4 (1 / 2 / 4) and spmv_blocks (8 / 1024).  The switches are read once per process, so
stream_variants_worker.py runs once per setting, one process after another; what it can decide alone (every product twice with the
same bits, finite, within 4 eps |A| |x| of the extended-precision host product, kind 0; poisoned tails; the solves converged with
the true residual at the tolerance) it asserts itself, and the comparisons ACROSS settings are made here over the files it writes.

Bit-equalities asserted, all of which held on the MI355X:
  FS_SPMV_NT 0 / 1                            products, solutions, iteration counts, residual histories (only the loads differ)
  spmv_blocks 8 / 1024                        products (the grid decides who computes a row, not how)
  spmv_unroll 2/4/8/16, spmv_unroll4 1/2/4    products, and at unroll 4 / 16 solutions and histories (dia_round / sell_round /
                                              block_round add the entries of a row in their order, whatever the round length)
  FS_SPMV_PAIRS 0 / 1, FS_PAIR_BLOCKS 8       products (k_dia_pair_spmv: one accumulator per row, entries in the order of the
                                              offset list - "same per-row summation order", as its header says)
Solutions and histories are NOT compared bit for bit across FS_SPMV_PAIRS: the dot partials are summed per workgroup, and another
grid is another order of summation; there the iteration counts are equal and the histories follow the same host recurrence."""
# Measured on the MI355X: the largest err / (eps |A| |x|) over all rows - the same figure for every unroll, grid and setting of the
# switches, since the products are the same arrays - and next to it that of plain fp64 row sums on the host (bound for both: 4).
#   p1_200x4x2 2.131 / 2.131   p1_255x3x2 1.919 / 2.670   p1_255x4x9 1.997 / 1.997   p1_file 1.588 / 1.588   p1_shuffled 1.464 / 1.837
#   p2_20x3x3 2.366 / 2.513    p2_file 3.138 / 3.138      v3_7x6x5 1.682 / 1.682     v3_file 2.211 / 2.103   v2_rectangle 1.107 / 1.594
#   th_3x3x3 2.120 / 2.120    p2_200x2x2 2.561 / 2.612
# Pairs, single slices with FS_SPMV_PAIRS=1: p1_200x4x2 21, 6; p1_255x3x2 24, 0 (no second launch); p1_255x4x9 100, 0; p1_file 0, 17;
# p1_shuffled 0, 12; p2_20x3x3 0, 32; p2_file 0, 113; p2_200x2x2 50, 57 (of its 157 slices 28 have no row longer than 16 entries,
# 18 a row longer than 32, 4 a row longer than 48).
# Iterations in every setting: CG with and without the diagonal scaling and pipelined CG 81 (host recurrence: 81), BiCGStab 20; on 8
# workgroups (solve8) 95 (host: 95).  Histories against the host recurrence over 20 entries: 1.7e-14 (CG), 1.4e-13 (pipelined);
# BiCGStab with pairs against without: 3.3e-10.
# What the cases are for was tried on k_dia_pair_spmv with two deliberate mistakes: prev_hi carried from the wrong entry of a round
# fails p2_200x2x2 alone (384 rows, no P1 row has more than 15 entries); the single slices' dot partials written over the pairs'
# (part_base 0) breaks the first CG solve down.
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from oracle import fem_oracle as fo

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RTOL = 1e-10                              # of the worker's solves
CHILD_TIMEOUT = 240
# tag: the environment of the child
SETTINGS = {
    "pairs0_nt0": {"FS_SPMV_PAIRS": "0", "FS_SPMV_NT": "0"},
    "pairs1_nt0": {"FS_SPMV_PAIRS": "1", "FS_SPMV_NT": "0"},
    "pairs0_nt1": {"FS_SPMV_PAIRS": "0", "FS_SPMV_NT": "1"},
    "pairs1_nt1": {"FS_SPMV_PAIRS": "1", "FS_SPMV_NT": "1"},
    # 8 workgroups for the pair kernel: every workgroup walks several chunks, the last XCD's range is cut by the end of the list
    "pairs1_nt0_blocks8": {"FS_SPMV_PAIRS": "1", "FS_SPMV_NT": "0", "FS_PAIR_BLOCKS": "8"},
}
BASE = "pairs0_nt0"
SCALAR_CASES = ("p1_200x4x2", "p1_255x3x2", "p1_255x4x9", "p1_file", "p1_shuffled", "p2_20x3x3", "p2_file", "p2_200x2x2")
CASES = SCALAR_CASES + ("v3_7x6x5", "v3_file", "v2_rectangle", "th_3x3x3")
# group: (solves, unrolls).  "solve": the box of 3015 rows; "solve8": 200 slices on 8 workgroups (see the worker)
SOLVES = {"solve": (("cg_scaled", "cg_unscaled", "pipelined", "bicgstab"), (4, 16)), "solve8": (("cg_scaled", "cg_unscaled", "pipelined"), (4,))}

_runs = {}              # tag: (arrays, log)
_failed = []            # the first child that failed: no child is started after it


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("stream_variants")


def _child(workdir, tag):
    if tag in _runs:
        return _runs[tag]
    if _failed:
        pytest.fail("not started: the child %s failed before" % _failed[0])
    env = {k: v for k, v in os.environ.items() if k not in ("FS_SPMV_PAIRS", "FS_SPMV_NT", "FS_PAIR_BLOCKS", "FS_POOL_MAX_MB")}
    env.update(SETTINGS[tag], FS_SPACE_DEBUG="1")
    f = str(workdir / (tag + ".npz"))
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "stream_variants_worker.py"), f], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _failed.append(tag)
        pytest.fail("%s: no end after %d s\n%s" % (tag, CHILD_TIMEOUT, (e.stdout or b"").decode(errors="replace")[-3000:]))
    log = p.stdout.decode(errors="replace")
    if p.returncode != 0:
        _failed.append(tag)
        pytest.fail("%s: exit status %d\n%s" % (tag, p.returncode, log[-3000:]))
    assert log.rstrip().endswith("ok"), log[-3000:]
    with np.load(f) as z:
        _runs[tag] = ({k: z[k] for k in z.files}, log)
    return _runs[tag]


def _all(workdir):
    return {tag: _child(workdir, tag) for tag in SETTINGS}


def _pair_counts(log):
    """case: (pairs, single slices) from the line the library prints when it splits the slices of a space."""
    counts, case = {}, None
    for line in log.splitlines():
        if line.startswith("case "):
            case = line.split()[1]
        m = re.search(r"two-rows-per-lane product: (\d+) pairs, (\d+) single slices", line)
        if m and case not in counts:
            counts[case] = (int(m.group(1)), int(m.group(2)))
    return counts


def _worst(log, what):
    """case: the largest ratio of the lines 'worst CASE VARIANT RATIO' / 'plain CASE RATIO'."""
    worst = {}
    for line in log.splitlines():
        w = line.split()
        if w and w[0] == what:
            worst[w[1]] = max(worst.get(w[1], 0.0), float(w[-1]))
    return worst


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_every_variant_matches_the_host_product(workdir, tag):
    """One process per setting: what the worker asserts (see above), and here: the two-rows-per-lane product ran where it was forced -
    pairs AND single slices in one product on the box whose slices straddle its lines - and nowhere else."""
    arrays, log = _child(workdir, tag)
    for what in ("plain", "worst"):
        worst = _worst(log, what)
        assert sorted(worst) == sorted(CASES), (what, sorted(worst))
        print(tag, what, " ".join("%s %.3f" % kv for kv in sorted(worst.items())))
        assert max(worst.values()) <= 4.0
    counts = _pair_counts(log)
    print(tag, "pairs, single slices:", counts)
    if SETTINGS[tag]["FS_SPMV_PAIRS"] == "0":
        assert not counts, counts
        return
    assert sorted(c for c in counts if not c.startswith("solve")) == sorted(SCALAR_CASES), sorted(counts)
    pairs, singles = counts["p1_200x4x2"]
    assert pairs > 0 and singles > 0 and 2 * pairs + singles == 48, (pairs, singles)                 # 3015 rows: 47 slices + 7 rows
    assert counts["solve_mass_10000"] == counts["solve_mass_100000"] == counts["p1_200x4x2"]         # (spaces of the same mesh)
    assert counts["solve8_mass_10000"] == counts["p1_255x4x9"]
    pairs, singles = counts["p1_255x3x2"]
    assert pairs > 0 and 2 * pairs + singles == 48, (pairs, singles)
    pairs, singles = counts["p1_255x4x9"]
    # >= 17 chunks of 4 pairs, not a multiple of 8: 8 workgroups take several chunks each, the last XCD's range ends early
    assert 2 * pairs + singles == 200 and (pairs + 3) // 4 >= 17 and ((pairs + 3) // 4) % 8 != 0, (pairs, singles)
    # a pair is two consecutive complete DIA slices with one offset list: the rows of a mesh in file order share none
    for case in ("p1_file", "p1_shuffled"):
        assert counts[case][0] == 0 and counts[case][1] > 0, (case, counts[case])
    for case in ("p2_20x3x3", "p2_file"):             # (split slices, two lists each, are never paired)
        assert counts[case][1] > 0, (case, counts[case])
    # CG2 with whole slices inside a mesh line: pairs whose rows span several 16-entry rounds of k_dia_pair_spmv (the width of a
    # slice is at least its longest row: more paired slices than there are slices of rows of 16 entries or fewer)
    m = re.search(r"slices p2_200x2x2 (\d+) longest row <= 16: (\d+) > 32: (\d+) > 48: (\d+)", log)
    n_slices, le16, gt32, gt48 = (int(g) for g in m.groups())
    pairs, singles = counts["p2_200x2x2"]
    print(tag, "p2_200x2x2: slices", n_slices, "with a longest row <= 16:", le16, "> 32:", gt32, "> 48:", gt48)
    assert 2 * pairs + singles == n_slices == 157 and singles > 0 and 2 * pairs > le16, (pairs, singles, n_slices, le16)
    assert log.count("poisoned ") == len(SCALAR_CASES) and "poisoned p1_200x4x2 n 3015 odd" in log and "poisoned p2_20x3x3 n 2009 odd" in log


def _products(arrays):
    return {k: v for k, v in arrays.items() if k.startswith("y/")}


def test_nontemporal_loads_change_no_bit(workdir):
    """FS_SPMV_NT = 1 replaces the loads of values and columns by nontemporal ones: products, solutions, iteration counts and
    residual histories are the same arrays."""
    runs = _all(workdir)
    for pairs in ("0", "1"):
        a, b = runs["pairs%s_nt0" % pairs][0], runs["pairs%s_nt1" % pairs][0]
        assert sorted(a) == sorted(b)
        for k in a:
            assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), (pairs, k)


def test_grid_unroll_and_pairing_change_no_bit_of_a_product(workdir):
    """Who computes a row (spmv_blocks, FS_PAIR_BLOCKS, pairs or single slices) and how many of its entries are in flight
    (spmv_unroll, spmv_unroll4, the 16-entry rounds of k_dia_pair_spmv) do not change the order in which the entries of a row are
    added: every variant of a product in every process is the same array."""
    runs = _all(workdir)
    ref = _products(runs[BASE][0])
    n_variants = {case: 6 if case == "th_3x3x3" else 8 for case in CASES}
    assert len(ref) == sum(n_variants.values())
    for case in CASES:
        first = ref["y/%s/u%d/b8" % (case, 1 if case == "th_3x3x3" else 2)]
        for tag, (arrays, _) in runs.items():
            ys = {k: v for k, v in _products(arrays).items() if k.split("/")[1] == case}
            assert len(ys) == n_variants[case], (tag, case, sorted(ys))
            for k, v in ys.items():
                assert v.shape == first.shape and np.array_equal(v, first), (tag, k, int((v != first).sum()))


def test_fused_dot_solves_follow_the_host_recurrence(workdir):
    """CG with the diagonal scaling (DOTS 3), without it (DOTS 1), the pipelined recurrence (DOTS 4) and BiCGStab (DOTS 2) on the
    box whose product is pairs + single slices, with the plane x = 0 held, at spmv_unroll 4 and 16 in every process: the iteration
    count of the plain setting at unroll 4; the residual history follows the oracle's recurrence as in
    test_config2_family_cg_parity (first 20 entries, rtol 1e-6); the same history and solution at both unrolls.  The oracle has no
    BiCGStab: its history is held to the plain setting's instead, at the same tolerance, over the entries both have.

    The worker chooses the mass term so that the solves are short (see there): on the operator of the products (mass 0.7, CG 1091
    iterations in every setting) BiCGStab took 836 iterations with FS_SPMV_PAIRS=0 and 737 with 1, with mass 1e4 61 and 55 - the
    two histories are equal to 1e-16 over their first five entries and drift apart by a factor of 10 every 2.5 iterations, which
    is BiCGStab's answer to another order of summing the dot partials, not a wrong dot."""
    runs = _all(workdir)
    base = runs[BASE][0]
    for group, (kinds, unrolls) in SOLVES.items():
        A = sp.csr_matrix((base[group + "/A_va"], base[group + "/A_ci"], base[group + "/A_rp"]))
        _, it_cg, hist_cg = fo.pcg_jacobi_single_reduction(A, base[group + "/b"], rtol=RTOL)
        _, it_pipe, hist_pipe = fo.pcg_jacobi_pipelined(A, base[group + "/b"], rtol=RTOL)
        print(group, "oracle iterations", it_cg, it_pipe)
        reference = {"cg_scaled": hist_cg, "cg_unscaled": hist_cg, "pipelined": hist_pipe}
        if "bicgstab" in kinds:
            reference["bicgstab"] = base[group + "/bicgstab/u4/hist"]
        for tag, (arrays, _) in runs.items():
            for k in ("/A_va", "/A_ci", "/A_rp", "/b"):
                assert np.array_equal(arrays[group + k], base[group + k]), (tag, group + k)
            for kind in kinds:
                first = "%s/%s/u%d" % (group, kind, unrolls[0])
                for unroll in unrolls:
                    key = "%s/%s/u%d" % (group, kind, unroll)
                    its, h = int(arrays[key + "/iterations"]), arrays[key + "/hist"]
                    assert its == int(base[first + "/iterations"]), (tag, key, its, int(base[first + "/iterations"]))
                    assert np.array_equal(h, arrays[first + "/hist"]), (tag, key)
                    assert np.array_equal(arrays[key + "/x"], arrays[first + "/x"]), (tag, key)
                    ho = np.asarray(reference[kind])
                    m = min(len(h), len(ho), 20)
                    assert m >= (10 if kind == "bicgstab" else 20), (tag, key, len(h), len(ho))
                    print(tag, key, "iterations", its, "history: largest relative deviation over %d entries %.2e" % (m, np.abs(h[:m] / ho[:m] - 1.0).max()))
                    assert np.allclose(h[:m], ho[:m], rtol=1e-6), (tag, key)
