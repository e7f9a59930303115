"""The kernels of the AMG V-cycle (fs_amg.hip: k_bcsr_spmv / _grp / _node, k_restrict, k_prolong_add / _grp, k_cheb_first / _next and
their _bt twins, k_dense_apply) against a host replay of the same hierarchy: amg.apply(r, z) is a fixed sequence of sparse products
and element-wise updates of operators that the inspection hooks return (level_matrix, level_info()["lambda_max"],
coarse_inverse()), so amg_reference.vcycle_replay reproduces it to rounding and carries a derived componentwise bound for the
difference (see there; test_amg_reference_host.py holds the replay itself to a dense extended-precision cycle on the CPU).

The switches that pick the kernels are read once per process, so amg_vcycle_worker.py runs once per setting, one process after
another, never two at a time, none after one has failed.  What a process can decide alone it asserts itself: the Galerkin and
near-null-space checks of test_gpu_amg._check_hierarchy, lambda_max <= min(1.1 lambda_true, Gershgorin), z overwritten (NaN before
every apply), two applications with the same bits, |z - z_ref| <= e_z in every component.  Here: every case ran in every setting,
the tightness condition max(e_z) <= 1e-9 max|z_ref| over all of them, the coverage conditions over all reports, and
FS_AMG_NO_ROW_GROUPS against the default bit for bit.

The library's selection rule, restated (coarse_level_spmv): below level 0 a level of 6 x 6 blocks with nnz >= 4 nn takes the wave
per node (fp32 values where fp32 storage is on), else one with nnz >= 8 nn takes 16 lanes per scalar row, else a thread per row;
FS_AMG_NO_NODE_WAVES / FS_AMG_NO_ROW_GROUPS take the first / second away."""
# Measured on the MI355X.  The largest err / e_z per case over the seven settings and three right-hand sides, and next to it the
# largest max(e_z) / max|z_ref|, the tightness figure (condition: 1e-9); both are the same to two digits in every setting:
#   scalar_9x7x5 0.018, 9.1e-13        scalar_file 0.037, 7.4e-13         vector_nb3_10x5x4 0.019, 4.6e-13
#   vector_rbm_13x3x4 0.0004, 5.4e-12  ..._clamp_x 0.015, 4.3e-11         vector_cg2_6x4x4 0.013, 2.0e-11
#   levels1 0.058, 4.6e-15             levels2 0.001, 4.4e-13             levels3 = steps2 = vector_rbm_13x3x4
#   steps1 0.056, 1.0e-12              steps3 0.015, 1.4e-11              scalar_cube_cheb_coarse 0.021, 1.6e-12
# (the bound is a worst case over every rounding of the cycle; a device that is right sits well inside it).  With the bounds
# chained operation by operation through the smoother, as amg_reference.py first did, the tightness figures were 1.3e-9
# (vector_rbm_13x3x4), 1.1e-8 (clamp_x), 4.4e-9 (CG2), 3.9e-7 (steps3) and 1.2e-7 (cube): see its header.
# Children: 1.9 to 2.0 s each (the first of a session 10.5 s).  Cube edge of the Chebyshev-coarse case: 30 (29 791 rows, level 1
# 2 597; edge 29: 2 378 rows on level 1 and a dense inverse; edge 28: 2 141).
# lambda_true / (1.1 lambda_max) over all cases, levels and settings: 0.826 to 0.945 - no level under-estimates.
# Boxes changed for the coverage conditions: vector, no near-null space (7, 4, 3) -> (10, 5, 4) (level 1 of the smaller box has 78
# blocks on 10 nodes: no k_bcsr_spmv_grp<3>); CG2 (4, 2, 2) -> (6, 4, 4) (9 nodes on level 1: no 6 x 6 block row beyond 22 blocks).
# The scalar box holds its planes x = 0, 1 (with z held, five cells deep, no node is two couplings away from a held one, which
# the near-null-space check of _check_hierarchy needs).
# Three deliberate mistakes in scratch builds of fs_amg.hip, each against this file and tests/test_gpu_amg.py:
#   k_restrict reading only the first 64 entries of a column    here: scalar_9x7x5 outside the bound (err / e_z 1.3e9, 384 rows);
#                                                               test_gpu_amg.py: 6 of 10 fail too (R != P^T: CG stalls)
#   the two rows of a lane swapped in the fp32 branch of        here: lambda_max of level 1 of vector_rbm_13x3x4 above its bound (the power
#   k_bcsr_spmv_node                                            iteration runs the same kernel); test_gpu_amg.py: 10 of 10 pass
#   k_cheb_next with rho * rho for rho_new * rho                here: scalar_9x7x5 outside the bound (err / e_z 3.9e10); test_gpu_amg.py: 10 pass
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHILD_TIMEOUT = 240
SWITCHES = ("FS_AMG_FP32", "FS_AMG_NO_NODE_WAVES", "FS_AMG_NO_ROW_GROUPS", "FS_AMG_SPGEMM_BLOCK", "FS_AMG_SERIAL_QR", "FS_AMG_DEBUG",
            "FS_AMG_LMAX_DICT")
SETTINGS = {
    "default": {},
    "fp64_storage": {"FS_AMG_FP32": "0"},
    "no_node_waves": {"FS_AMG_NO_NODE_WAVES": "1"},
    "no_row_groups": {"FS_AMG_NO_ROW_GROUPS": "1"},
    "thread_per_row": {"FS_AMG_NO_NODE_WAVES": "1", "FS_AMG_NO_ROW_GROUPS": "1"},
    "spgemm_block": {"FS_AMG_SPGEMM_BLOCK": "1"},
    "serial_qr": {"FS_AMG_SERIAL_QR": "1"},
}
CASES = ("scalar_9x7x5", "scalar_file", "vector_nb3_10x5x4", "vector_rbm_13x3x4", "vector_rbm_13x3x4_clamp_x", "vector_cg2_6x4x4",
         "vector_rbm_levels1", "vector_rbm_levels2", "vector_rbm_levels3", "vector_rbm_steps1", "vector_rbm_steps2", "vector_rbm_steps3",
         "scalar_cube_cheb_coarse")

_runs = {}              # tag: (arrays, reports, log)
_failed = []            # the first child that failed: no child is started after it


@pytest.fixture(scope="module")
def workdir(tmp_path_factory):
    return tmp_path_factory.mktemp("amg_vcycle")


def _child(workdir, tag):
    if tag in _runs:
        return _runs[tag]
    if _failed:
        pytest.fail("not started: the child %s failed before" % _failed[0])
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(SETTINGS[tag])
    f = str(workdir / (tag + ".npz"))
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "amg_vcycle_worker.py"), f], env=env, cwd=ROOT,
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=CHILD_TIMEOUT)
    except subprocess.TimeoutExpired as e:
        _failed.append(tag)
        pytest.fail("%s: no end after %d s\n%s" % (tag, CHILD_TIMEOUT, (e.stdout or b"").decode(errors="replace")[-3000:]))
    log = p.stdout.decode(errors="replace")
    if p.returncode != 0:
        _failed.append(tag)
        pytest.fail("%s: exit status %d\n%s" % (tag, p.returncode, log[-4000:]))
    assert log.rstrip().endswith("ok"), log[-3000:]
    reports = {}
    for line in log.splitlines():
        if line.startswith("report "):
            rep = json.loads(line[len("report "):])
            reports[rep["case"]] = rep
    with np.load(f) as z:
        _runs[tag] = ({k: z[k] for k in z.files}, reports, log)
    return _runs[tag]


def _all(workdir):
    return {tag: _child(workdir, tag) for tag in SETTINGS}


@pytest.mark.parametrize("tag", list(SETTINGS))
def test_the_cycle_is_the_replay_to_rounding(workdir, tag):
    """One process per setting: what the worker asserts (see above); here that every case and right-hand side reported, inside its
    bound, and that the process took seconds."""
    _, reports, log = _child(workdir, tag)
    assert sorted(reports) == sorted(CASES), sorted(reports)
    for case in CASES:
        rep = reports[case]
        assert sorted(rep["rhs"]) == ["normal", "ones", "unit"], (case, sorted(rep["rhs"]))
        worst = max(f["ratio"] for f in rep["rhs"].values())
        tight = max(f["tight"] for f in rep["rhs"].values())
        print(tag, case, "rows", rep["n"], "levels", [(L["bs"], L["nn"], L["family"]) for L in rep["levels"]],
              "err / e_z %.3f" % worst, "max(e_z) / max|z| %.1e" % tight, "%.1f s" % rep["seconds"])
        assert worst <= 1.0, (tag, case, worst)
        for l, L in enumerate(rep["levels"]):
            if "lam_ratio" in L:
                print(tag, case, "level", l, "lambda_true / (1.1 lambda_max) %.4f" % L["lam_ratio"])
    assert reports["scalar_cube_cheb_coarse"]["dense_coarse"] is False and reports["vector_rbm_levels1"]["dense_coarse"] is False
    assert all(reports[c]["dense_coarse"] for c in CASES if c not in ("scalar_cube_cheb_coarse", "vector_rbm_levels1"))
    assert [len(reports["vector_rbm_levels%d" % k]["levels"]) for k in (1, 2, 3)] == [1, 2, 3]
    assert [reports["vector_rbm_steps%d" % k]["steps"] for k in (1, 2, 3)] == [1, 2, 3]
    seconds = float([line for line in log.splitlines() if line.startswith("seconds ")][-1].split()[1])
    print(tag, "child: %.1f s" % seconds)
    assert seconds <= 60.0, (tag, seconds)


def test_the_bound_is_tight(workdir):
    """max(e_z) <= 1e-9 max|z_ref| in every case, setting and right-hand side: a bound that has grown loose hides failures."""
    runs = _all(workdir)
    loose = {}
    for tag, (_, reports, _) in runs.items():
        for case, rep in reports.items():
            for what, f in rep["rhs"].items():
                if not f["tight"] <= 1e-9:
                    loose[(tag, case, what)] = "%.1e" % f["tight"]
    assert not loose, loose


def _levels(runs):
    for tag, (_, reports, _) in runs.items():
        for case, rep in reports.items():
            for l, L in enumerate(rep["levels"]):
                yield tag, case, l, L


def test_every_kernel_of_the_cycle_ran(workdir):
    """The coverage conditions: without them the cases could quietly stop reaching a path.  A level product counts where the level is
    below the fine one and the dense inverse does not stand in for it; a transfer where its level has a prolongator."""
    runs = _all(workdir)
    products, transfers = {}, {}
    for tag, case, l, L in _levels(runs):
        if L["family"] is not None:
            key = (L["family"], L["bs"]) + (("float" if L["a32"] else "double",) if L["family"] == "node" else ())
            products.setdefault(key, (tag, case, l))
        if "p_shape" in L:
            transfers.setdefault((tuple(L["p_shape"]), "float" if L["p32"] else "double"), (tag, case, l))
    print("products", products)
    print("transfers", transfers)
    for key in [("node", 6, "float"), ("node", 6, "double")] + [(f, bs) for f in ("grp", "row") for bs in (1, 3, 6)]:
        assert key in products, ("no level ran the product", key, sorted(products))
    # k_restrict<1,1>, <3,3>, <3,6>, <6,6> with k_prolong_add (run-time shape) for the first two and k_prolong_add_grp for the others
    for key in [((1, 1), "double"), ((3, 3), "double"), ((3, 6), "double"), ((3, 6), "float"), ((6, 6), "double"), ((6, 6), "float")]:
        assert key in transfers, ("no level ran the transfer", key, sorted(transfers))
    lv = list(_levels(runs))
    # the strided loops: more than one pass of the fp32 node loop (64 lanes, 3 per block: 21 blocks and a third per pass), of the
    # restriction's loop over a column (64 lanes) and less than one; a last, partial group of 4 waves (nodes per workgroup of
    # k_bcsr_spmv_node and k_restrict) and of 16 nodes (k_prolong_add_grp)
    assert any(L["family"] == "node" and L["a32"] and L["longest_row"] > 22 for _, _, _, L in lv)
    assert any(L.get("p_col_max", 0) > 64 for _, _, _, L in lv)
    assert any(0 < L.get("p_col_min", 64) < 64 for _, _, _, L in lv)
    assert any(L["nn"] % 4 != 0 for _, _, _, L in lv) and any(L["nn"] % 16 != 0 for _, _, _, L in lv)


def test_row_groups_touch_only_the_cycle(workdir):
    """FS_AMG_NO_ROW_GROUPS=1 replaces k_bcsr_spmv_grp in the V-cycle alone (the set-up's products do not read it): the hierarchy
    is the default's bit for bit - every A, P, lambda_max and the dense inverse.  The other settings change the summation order of
    the set-up and are each held to their own replay only."""
    runs = _all(workdir)
    a, b = runs["default"][0], runs["no_row_groups"][0]
    assert sorted(a) == sorted(b)
    compared = 0
    for k in a:
        if "/z/" in k:
            continue
        assert a[k].shape == b[k].shape and np.array_equal(a[k], b[k]), k
        compared += 1
    assert compared > 5 * len(CASES)
