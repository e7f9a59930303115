"""Run by tests/test_gpu_amg_setup.py, one process per setting of FS_AMG_SERIAL_QR / FS_AMG_SPGEMM_BLOCK / FS_AMG_FP32 /
FS_AMG_NO_NODE_WAVES / FS_AMG_LMAX_DICT (the library reads them once per process): the hierarchy that fs_amg_setup builds against
the host replay of the set-up (amg_setup_reference.py), level by level.

For every level l with a prolongator, ONE coarsening step is replayed from the device's own A_l, B_l and lambda_max_l (so that an
error of one stage does not blur the next) and compared: aggregates, node counts, the patterns of P_l and A_{l+1} and the dead
coarse dofs exactly; B_{l+1}, P_l and lambda_max_l to rounding, inside tolerances derived in amg_setup_reference.py.  The number
of levels and the dense inverse are held to the stopping rules.  The Galerkin values stay with test_gpu_amg._check_hierarchy.
The replay must not have made an ambiguous decision on any level: that is asserted first.

Output lines the caller reads: "report {json}" per case, "ok" at the end; what is compared ACROSS processes goes into the .npz
file argv[1].  argv[2] == "measure": a miss is reported instead of asserted.  argv[3]: the cases to run, comma separated."""
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import amg_vcycle_worker as vw  # noqa: E402  (its operators; it initialises the device)
from amg_vcycle_worker import B, fo  # noqa: E402
from fenicssolver_amd._lib import BackendError  # noqa: E402
import amg_reference as ar  # noqa: E402
import amg_setup_reference as sr  # noqa: E402
from test_gpu_amg import _check_hierarchy  # noqa: E402

T0 = time.time()
MEASURE = len(sys.argv) > 2 and sys.argv[2] == "measure"
ONLY = sys.argv[3].split(",") if len(sys.argv) > 3 else None
FP32 = os.environ.get("FS_AMG_FP32", "1")[:1] != "0"
NODE_WAVES = "FS_AMG_NO_NODE_WAVES" not in os.environ
SPGEMM = "block" if "FS_AMG_SPGEMM_BLOCK" in os.environ else "wave"
QR = "serial" if "FS_AMG_SERIAL_QR" in os.environ else "wave"
out = {}
misses = []


def say(*a):
    print(*a, flush=True)


def hold(cond, *what):
    if not cond:
        if not MEASURE:
            raise AssertionError(what)
        misses.append(repr(what)[:300])
        say("miss", what)


def with_options(make, **more):
    def wrapped():
        V, A, K, nullspace, nb, B0, kw = make()
        return V, A, K, nullspace, nb, B0, dict(kw, **more)
    return wrapped


def case_thin_box():
    co, ce = fo.box_mesh((0, 0, 0), (1, 1, 0.1), 6, 6, 12)
    V, A, K = vw.scalar_p1(co, ce, 3, 2)
    return V, A, K, None, 1, np.ones((V.n_owned, 1)), dict(coarse_size=20)


def case_far_origin():
    """vector_rbm with the rotations about a far point: live columns with nrm / orig below 1e-6 (see far_rigid_body_modes)."""
    V, A, K, _, nb, _, kw = vw.vector_rbm(strength_threshold=0.2, max_levels=2)()
    ns = sr.far_rigid_body_modes(fo.box_mesh((0, 0, 0), (4.0, 1.0, 1.0), 13, 3, 4)[0])
    return V, A, K, ns, nb, ns.T.copy(), kw


BOX = vw.CASES["scalar_9x7x5"]
CASES = {k: vw.CASES[k] for k in ("scalar_9x7x5", "scalar_file", "vector_nb3_10x5x4", "vector_rbm_13x3x4", "vector_rbm_13x3x4_clamp_x",
                                  "vector_cg2_6x4x4")}
CASES.update({
    "scalar_9x7x5_theta_-1": with_options(BOX, strength_threshold=-1.0),
    "scalar_9x7x5_theta_0.25": with_options(BOX, strength_threshold=0.25),
    "scalar_9x7x5_theta_0.5": with_options(BOX, strength_threshold=0.5),
    "scalar_9x7x5_eig_1": with_options(BOX, eig_steps=1),
    "scalar_9x7x5_eig_2": with_options(BOX, eig_steps=2),
    "scalar_9x7x5_eig_15": with_options(BOX, eig_steps=15),
    "scalar_thin_6x6x12": case_thin_box,
    "vector_rbm_levels1": vw.vector_rbm(max_levels=1),
    "vector_rbm_levels2": vw.vector_rbm(max_levels=2),
    "vector_rbm_coarse_size_1": vw.vector_rbm(coarse_size=1),
    "vector_rbm_theta_0.25": vw.vector_rbm(strength_threshold=0.25),
    "vector_rbm_far_origin": case_far_origin,
})
# the near-null-space part of _check_hierarchy needs every node near a checked row in an aggregate without a dead column
GALERKIN_ONLY = ("scalar_9x7x5_theta_0.25", "vector_rbm_theta_0.25")


def galerkin_values(amg, n_levels):
    """The Galerkin part of test_gpu_amg._check_hierarchy alone."""
    for l in range(n_levels - 1):
        Al, P, Ac = amg.level_matrix(l, "A"), amg.level_matrix(l, "P"), amg.level_matrix(l + 1, "A")
        ref = (P.T @ Al @ P).tocsr()
        d = abs(Ac - ref).tolil()
        for k in np.nonzero(np.asarray(abs(ref).sum(axis=1)).ravel() == 0)[0]:
            assert Ac[k, k] == 1.0
            d[k, k] = 0.0
        assert d.tocsr().max() <= 1e-11 * abs(ref).max(), l
        assert abs(Ac - Ac.T).max() <= 1e-11 * abs(Ac).max(), l


def run(name, make):
    t_case = time.time()
    V, A, A0, nullspace, nb, B0, kw = make()
    amg = B.AMG(A, nullspace=nullspace, **kw)
    n_levels = amg.info()["levels"]
    theta = sr.default_theta(kw.get("strength_threshold", 0.0))
    eig_steps = kw.get("eig_steps", 0) or 15
    dense = amg.coarse_inverse() is not None
    report = {"case": name, "n": V.n_owned, "levels": [], "dense_coarse": dense, "spgemm": SPGEMM, "qr": QR, "stop": None}
    info = [amg.level_info(l) for l in range(n_levels)]
    blocks = [amg.level_blocks(l, "A") for l in range(n_levels)]
    rows_last = info[-1]["n_nodes"] * info[-1]["block_size"]
    hold(dense == sr.has_dense_inverse(n_levels, rows_last), name, "dense inverse", dense, n_levels, rows_last)
    for l in range(n_levels):
        li = info[l]
        bs, nn = li["block_size"], li["n_nodes"]
        rp, ci, val = blocks[l]
        lev = {"bs": bs, "nn": nn, "nnz": len(ci), "longest_row": int(np.diff(rp).max()), "lmax": li["lambda_max"]}
        report["levels"].append(lev)
        hold(len(rp) == nn + 1 and val.shape[1:] == (bs, bs), name, l, "shape of A")
        hold(sr.columns_strictly_ascending(rp, ci), name, l, "columns of A not strictly ascending")
        a32 = l > 0 and ar.operator_is_fp32(bs, len(ci), nn, FP32, NODE_WAVES)
        lev["a32"] = a32
        last_by_rule = sr.is_last_level(l + 1, nn * bs, kw.get("max_levels", 0), kw.get("coarse_size", 0))
        hold(not (last_by_rule and l + 1 < n_levels), name, l, "a level below one that the level rules make the last")
        Bl = amg.level_nullspace(l, nb)
        if last_by_rule:
            dinv, _, _, gersh, _ = sr.diagonal(rp, ci, val)
            lmax, lam, lmax_bound = sr.power_iteration(rp, ci, val, dinv, gersh, eig_steps, a32)
            step = None
            report["stop"] = "level rule"
        else:
            step = sr.coarsen_step(rp, ci, val, Bl, theta, nb, eig_steps, a32, li["lambda_max"], want_coarse=False)
            lmax, lmax_bound = step["lmax"], step["lmax_bound"]
            hold(step["n_ambiguous"] == 0, name, l, "ambiguous decisions", step["ambiguous"])
            m = step["margins"]
            r = m["live_ratios"]
            lev.update(strength_margin=m["strength"], pass2_margin=m["pass2"], coupled_not_strong=step["coupled_not_strong"],
                       live_ratio_min=float(r.min()) if r.size else None)
            if l == n_levels - 1:
                hold(step["stop"] is not None, name, l, "the replay goes on where the library stopped")
                report["stop"] = step["stop"]
            else:
                hold(step["stop"] is None, name, l, "the library goes on where the replay stops", step["stop"])
        # lambda_max, two-sided
        tol_l = 16.0 * sr.LMAX_SPREAD * float(lmax)
        err_l = abs(li["lambda_max"] - float(lmax))
        lev.update(lmax_ratio=err_l / tol_l, lmax_tight=tol_l / float(lmax), lmax_carried=lmax_bound / float(lmax))
        out["%s/%d/lmax" % (name, l)] = np.float64(li["lambda_max"])
        hold(err_l <= tol_l, name, l, "lambda_max", li["lambda_max"], float(lmax), err_l / tol_l)
        if step is None or step["stop"] is not None:
            continue
        # ---- exact ------------------------------------------------------------------------------------------------------------
        agg = amg.level_aggregates(l)
        prp, pci, pval = amg.level_blocks(l, "P")
        crp, cci, cval = blocks[l + 1]
        n_agg = step["n_agg"]
        same = np.array_equal(agg, step["agg"])
        hold(same, name, l, "aggregates differ", int((agg != step["agg"]).sum()), np.flatnonzero(agg != step["agg"])[:8])
        hold(info[l + 1]["n_nodes"] == n_agg and info[l + 1]["block_size"] == nb and li["p_block_cols"] == nb, name, l, "n_agg / block shapes",
             info[l + 1]["n_nodes"], n_agg)
        hold(pval.shape[1:] == (bs, nb) and len(prp) == nn + 1, name, l, "shape of P")
        hold(sr.columns_strictly_ascending(prp, pci), name, l, "columns of P not strictly ascending")
        p_same = np.array_equal(prp, step["pptr"]) and np.array_equal(pci, step["pcol"])
        hold(p_same, name, l, "pattern of P differs")
        hold(np.array_equal(crp, step["cptr"]) and np.array_equal(cci, step["ccol"]), name, l, "pattern of the coarse operator differs")
        for k, v in (("agg", agg), ("pptr", prp), ("pcol", pci), ("cptr", crp), ("ccol", cci)):
            out["%s/%d/%s" % (name, l, k)] = v
        crow = np.repeat(np.arange(len(crp) - 1), np.diff(crp))
        diag = np.zeros((len(crp) - 1, nb))
        diag[crow[cci == crow]] = np.einsum("eii->ei", cval[cci == crow])
        unit = np.flatnonzero(diag.reshape(-1) == 1.0)
        hold(np.array_equal(unit, step["dead"]), name, l, "unit coarse diagonals are not the dead dofs", unit[:8], step["dead"][:8])
        rows_a = step["agg_rows"]
        lev.update(n_agg=n_agg, mis_rounds=step["mis_rounds"], pass2_nodes=step["pass2_nodes"], ties_by_index=step["ties_by_index"],
                   agg_rows_min=int(rows_a.min()), agg_rows_max=int(rows_a.max()), dead=int(len(step["dead"])),
                   unaggregated=int((agg < 0).sum()), nearly_dead=step["nearly_dead"], kappa_max=float(step["agg_kappa"].max()))
        if not (same and p_same):
            continue
        # ---- to rounding ----------------------------------------------------------------------------------------------------------
        Bc = amg.level_nullspace(l + 1, nb).reshape(n_agg, nb, nb)
        tol_r = sr.qr_tolerance(rows_a, step["agg_kappa"], step["agg_bmax"])
        err_r = np.abs(Bc - step["R"]).reshape(n_agg, -1).max(axis=1)
        scale_r = np.abs(step["R"]).reshape(n_agg, -1).max(axis=1)
        hold(np.all((Bc == 0.0)[~np.broadcast_to(step["live"][:, None, :], Bc.shape)]), name, l, "a dead column of B_c is not zero")
        e_t = sr.QR_C * sr.EPS * rows_a * step["agg_kappa"]
        bound_p = sr.prolongator_bound(rp, ci, val, step["dinv"], agg, n_agg, step["T"], e_t, li["lambda_max"])
        err_p = np.abs(pval - step["pval"])
        lev.update(r_ratio=float((err_r / np.maximum(tol_r, 1e-300)).max()), r_tight=float((tol_r / np.maximum(scale_r, 1e-300)).max()),
                   p_ratio=float((err_p / np.maximum(bound_p, 1e-300)).max()), p_tight=float(bound_p.max() / np.abs(step["pval"]).max()))
        say("figure", name, l, json.dumps({k: lev[k] for k in ("r_ratio", "r_tight", "p_ratio", "p_tight", "lmax_ratio", "lmax_tight")}))
        hold(np.all(err_r <= tol_r), name, l, "B_{l+1} against R", lev["r_ratio"])
        hold(np.all(err_p <= bound_p), name, l, "P outside its bound", lev["p_ratio"], int((err_p > bound_p).sum()))
    try:                                        # the last level has no prolongator, hence no aggregates: an error, not stale numbers
        amg.level_aggregates(n_levels - 1)
        hold(False, name, "level_aggregates of the last level did not fail")
    except BackendError as e:
        hold("no prolongator" in str(e), name, "level_aggregates of the last level", str(e))
    if n_levels >= 2:
        if name in GALERKIN_ONLY:
            galerkin_values(amg, n_levels)
        else:
            _check_hierarchy(amg, A0, B0 if B0 is not None else amg.level_nullspace(0, nb), nb)
    report["seconds"] = round(time.time() - t_case, 2)
    say("report", json.dumps(report))
    amg.close()


if __name__ == "__main__":
    for name, make in CASES.items():
        if ONLY is None or name in ONLY:
            try:
                run(name, make)
            except Exception:
                if not MEASURE:
                    raise
                import traceback
                say("case failed", name, traceback.format_exc())
    np.savez(sys.argv[1], **out)
    say("misses", len(misses))
    say("seconds", round(time.time() - T0, 1))
    say("ok")
