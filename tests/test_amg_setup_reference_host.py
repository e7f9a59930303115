"""The host replay of the AMG set-up (amg_setup_reference.py) proved on the CPU before the device is held to it
(test_gpu_amg_setup.py): run through all levels on the oracle's matrices of the cases of the GPU test - the host forms
A_{l+1} = P^T A_l P itself - and checked against what defines the method:
  * MIS(2): roots pairwise more than two strong couplings apart; every node with a strong coupling within two couplings of a root,
    and in an aggregate; aggregates connected in the strength graph; aggregates numbered in the order of their roots
  * QR: T R = B on the live columns, T^T T = I there, dead columns exactly zero, R upper triangular with a non-negative diagonal
  * P B_c = B wherever A B = 0 (on nodes whose neighbourhood is aggregated)
  * lam <= lambda_true <= 1.1 lam, lambda_true by a dense eigenvalue solve.  The upper half holds on every level whose lambda_max
    the V-cycle reads (lambda_true / (1.1 lam) 0.91 to 0.97).  It does NOT hold on the last level of vector_rbm_13x3x4_clamp_x
    (3 nodes, 18 rows: lam 2.0146, lambda_true 2.3028, ratio 1.039): fifteen steps from the hashed seed are not enough there.
    That level is solved by the dense inverse, its lambda_max is never read, so the assertion leaves out last levels with a
    dense inverse and prints their figure instead.
  * no ambiguous decision on any level (amg_setup_reference.AMBIGUOUS): the condition for comparing integer stages exactly
  * one coarsening step in float64 against the same step in np.longdouble and in float64 with every sum reversed, from identical
    inputs: the integer stages identical, the floating-point stages inside the tolerances that the device is held to.  The spreads
    printed here are what those tolerances were checked against (header of test_gpu_amg_setup.py).
The CG2 operator of the GPU test has no oracle matrix (the worker reads it back from the device) and is not run here."""
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

from oracle import fem_oracle as fo

import amg_reference as ar
import amg_setup_reference as sr

LD = np.longdouble
DATA = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "data")


# ---- the oracle's matrices of the cases of amg_setup_worker.py --------------------------------------------------------------------
def _scalar(mesh, seed, axis):
    co, ce = mesh
    kc = np.random.default_rng(seed).uniform(0.5, 1.5, len(ce))
    K = fo.assemble_p1_scalar(co, ce, kc)
    t = co[:, axis]
    tol = 1e-9 * (t.max() - t.min())
    dofs = np.nonzero((t <= t.min() + tol) | (t >= t.max() - tol))[0].astype(np.int32)
    K, _ = fo.apply_dirichlet(K, np.zeros(K.shape[0]), dofs, np.zeros(len(dofs)), True)
    return K.tocsr(), 1, 1, np.ones((K.shape[0], 1))


def _box():
    return _scalar(fo.box_mesh((0, 0, 0), (1, 1, 1), 9, 7, 5), 0, 0)


def _thin():
    return _scalar(fo.box_mesh((0, 0, 0), (1, 1, 0.1), 6, 6, 12), 3, 2)


def _file():
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(DATA, "mesh.xml"))
    return _scalar((co, ce.astype(np.int32)), 1, 2)


def _elasticity(dims, clamp=None, rigid=True, far=False):
    co, ce = fo.box_mesh((0, 0, 0), (4.0, 1.0, 1.0), *dims)
    K = fo.assemble_p1_elasticity(co, ce, 2e11, 0.27)
    left = np.nonzero(co[:, 0] == 0)[0]
    dofs = (left[:, None] * 3 + (np.arange(3) if clamp is None else np.asarray(clamp))).ravel().astype(np.int32)
    if clamp is not None:
        xm = co[:, 0].max()
        na = np.nonzero((co[:, 0] == xm) & (co[:, 1] == 0) & (co[:, 2] == 0))[0][0]
        nb_ = np.nonzero((co[:, 0] == xm) & (co[:, 1] == 1) & (co[:, 2] == 0))[0][0]
        dofs = np.unique(np.concatenate([dofs, [na * 3 + 1, na * 3 + 2, nb_ * 3 + 2]])).astype(np.int32)
    K, _ = fo.apply_dirichlet(K, np.zeros(K.shape[0]), dofs, np.zeros(len(dofs)), True)
    if far:
        return K.tocsr(), 3, 6, sr.far_rigid_body_modes(co).T.copy()
    if rigid:
        return K.tocsr(), 3, 6, fo.rigid_body_modes(co).T.copy()
    return K.tocsr(), 3, 3, np.tile(np.eye(3), (K.shape[0] // 3, 1))


CASES = {
    "scalar_9x7x5": (_box, dict(coarse_size=20)),
    "scalar_9x7x5_theta_-1": (_box, dict(coarse_size=20, strength_threshold=-1.0)),
    "scalar_9x7x5_theta_0.25": (_box, dict(coarse_size=20, strength_threshold=0.25)),
    "scalar_9x7x5_theta_0.5": (_box, dict(coarse_size=20, strength_threshold=0.5)),
    "scalar_9x7x5_eig_1": (_box, dict(coarse_size=20, eig_steps=1)),
    "scalar_9x7x5_eig_2": (_box, dict(coarse_size=20, eig_steps=2)),
    "scalar_thin_6x6x12": (_thin, dict(coarse_size=20)),
    "scalar_file": (_file, dict(coarse_size=20)),
    "vector_nb3_10x5x4": (lambda: _elasticity((10, 5, 4), rigid=False), dict(coarse_size=10)),
    "vector_rbm_13x3x4": (lambda: _elasticity((13, 3, 4)), dict(coarse_size=30)),
    "vector_rbm_13x3x4_clamp_x": (lambda: _elasticity((13, 3, 4), clamp=(0,)), dict(coarse_size=30)),
    "vector_rbm_levels1": (lambda: _elasticity((13, 3, 4)), dict(coarse_size=30, max_levels=1)),
    "vector_rbm_levels2": (lambda: _elasticity((13, 3, 4)), dict(coarse_size=30, max_levels=2)),
    "vector_rbm_coarse_size_1": (lambda: _elasticity((13, 3, 4)), dict(coarse_size=1)),
    "vector_rbm_far_origin": (lambda: _elasticity((13, 3, 4), far=True), dict(coarse_size=30, strength_threshold=0.2, max_levels=2)),
    "vector_rbm_theta_0.25": (lambda: _elasticity((13, 3, 4)), dict(coarse_size=30, strength_threshold=0.25)),
}


@pytest.fixture(scope="module", params=list(CASES), ids=list(CASES))
def replayed(request):
    make, kw = CASES[request.param]
    K, bs, nb, B0 = make()
    rp, ci, val = sr.blocks_from_csr(K, bs)
    levels, dense = sr.setup_replay(rp, ci, val, B0, nb, fp32_of_level=lambda l, b, nnz, nn: ar.operator_is_fp32(b, nnz, nn), **kw)
    return request.param, kw, nb, levels, dense


def _strength_graph(step):
    nn = step["nn"]
    return sp.csr_matrix((np.ones(len(step["scol"]), dtype=np.int64), step["scol"], step["sptr"]), shape=(nn, nn))


def test_the_level_rules(replayed):
    name, kw, nb, levels, dense = replayed
    print(name, [(L["nn"], L["bs"], len(L["ci"]), L["stop"]) for L in levels], "dense inverse", dense)
    expect = {"scalar_9x7x5_theta_0.5": (1, "no strong coupling"), "vector_rbm_levels1": (1, "level rule"),
              "vector_rbm_levels2": (2, "level rule"), "vector_rbm_far_origin": (2, "level rule"), "vector_rbm_coarse_size_1": (4, "no strong coupling"),
              "scalar_9x7x5_theta_0.25": (2, "no strong coupling"), "vector_rbm_theta_0.25": (2, "no strong coupling")}
    if name in expect:
        assert (len(levels), levels[-1]["stop"]) == expect[name]
    else:
        assert len(levels) >= 3 and levels[-1]["stop"] == "level rule"
    assert dense == (len(levels) > 1)
    for L in levels[:-1]:
        assert L["step"]["n_agg"] * nb < L["nn"] * L["bs"]


def test_aggregation_is_a_distance_two_independent_set_with_connected_aggregates(replayed):
    name, kw, nb, levels, dense = replayed
    for l, L in enumerate(levels):
        s = L["step"]
        if s is None or "agg" not in s:
            continue
        S = _strength_graph(s)
        assert (S != S.T).nnz == 0                      # symmetric operator: symmetric strength graph
        S2 = (S + S @ S).tocsr()
        root = np.flatnonzero(s["root"])
        R2 = S2[root][:, root].tolil()
        R2.setdiag(0)
        assert R2.tocsr().count_nonzero() == 0, (name, l, "two roots within two couplings")
        has = np.diff(s["sptr"]) > 0
        reach = np.asarray((S2 + sp.identity(s["nn"], dtype=np.int64, format="csr"))[:, root].sum(axis=1)).ravel() > 0
        assert np.all(reach[has]) and np.all(s["agg"][has] >= 0) and np.all(s["agg"][~has] == -1), (name, l)
        assert np.array_equal(s["agg"][root], np.arange(s["n_agg"])), (name, l, "aggregates not numbered in the order of their roots")
        for a in range(s["n_agg"]):
            m = np.flatnonzero(s["agg"] == a)
            assert len(m) >= 1 and connected_components(S[m][:, m], directed=False)[0] == 1, (name, l, a)
        print(name, "level", l, "MIS rounds", s["mis_rounds"], "aggregates", s["n_agg"], "pass-2 nodes", s["pass2_nodes"],
              "ties by index", s["ties_by_index"], "coupled but not strongly", s["coupled_not_strong"])


def test_no_decision_is_ambiguous(replayed):
    name, kw, nb, levels, dense = replayed
    for l, L in enumerate(levels):
        s = L["step"]
        if s is None:
            continue
        r = s["margins"]["live_ratios"]
        print(name, "level", l, "margins: strength", s["margins"]["strength"], "pass 2", s["margins"]["pass2"],
              "nrm / orig", (float(r.min()), float(r.max())) if r.size else None)
        assert s["n_ambiguous"] == 0, (name, l, s["ambiguous"])


def test_the_qr_and_the_smoothed_prolongator(replayed):
    name, kw, nb, levels, dense = replayed
    for l, L in enumerate(levels[:-1]):
        s = L["step"]
        bs, nn, n_agg = L["bs"], L["nn"], s["n_agg"]
        T, R, live, ident = s["T"], s["R"], s["live"], s["ident"]
        B = np.where(ident[:, None], 0.0, L["B"].reshape(nn * bs, nb))
        tol = sr.qr_tolerance(s["agg_rows"], s["agg_kappa"], s["agg_bmax"])
        for a in range(n_agg):
            rows = (np.flatnonzero(s["agg"] == a)[:, None] * bs + np.arange(bs)).ravel()
            Q, lv = T[rows], live[a]
            assert np.all(Q[:, ~lv] == 0.0) and np.all(R[a][:, ~lv] == 0.0), (name, l, a, "dead column not zero")
            assert np.all(np.tril(R[a], -1) == 0.0) and np.all(np.diag(R[a]) >= 0.0) and np.all((np.diag(R[a]) > 0) == lv)
            assert np.abs(Q[:, lv].T @ Q[:, lv] - np.eye(lv.sum())).max() <= sr.QR_C * sr.EPS * len(rows) * s["agg_kappa"][a], (name, l, a)
            assert np.abs(Q @ R[a] - B[rows])[:, lv].max() <= tol[a], (name, l, a, np.abs(Q @ R[a] - B[rows])[:, lv].max(), tol[a])
        # P B_c = B where A B = 0: the node, its neighbours and theirs see A B = 0 and are aggregated
        A = sr.blocks_to_csr(L["rp"], L["ci"], L["val"], nn)
        P = sr.blocks_to_csr(s["pptr"], s["pcol"], s["pval"], n_agg)
        Bl = L["B"].reshape(nn * bs, nb)
        ok = ((np.abs(A @ Bl) <= 1e-9 * (abs(A) @ np.abs(Bl)) + 1e-300).all(axis=1) & ~ident).reshape(nn, bs).all(axis=1) & (s["agg"] >= 0)
        ok &= live.all(axis=1)[np.where(s["agg"] >= 0, s["agg"], 0)]          # (a dead column is a vector the aggregate cannot carry)
        G = sp.csr_matrix((np.ones(len(L["ci"])), L["ci"], L["rp"]), shape=(nn, nn))
        good = ok & (np.asarray(G @ (~ok).astype(float)).ravel() == 0)
        rows = np.repeat(good, bs)
        if l == 0 and name not in ("scalar_thin_6x6x12", "scalar_9x7x5_theta_0.25", "vector_rbm_theta_0.25"):
            assert rows.any(), (name, "no row to check the near-null space on")
        if rows.any():
            assert np.abs((P @ R.reshape(-1, nb))[rows] - Bl[rows]).max() <= 1e-8 * np.abs(Bl).max(), (name, l)
        print(name, "level", l, "rows of the aggregates %d to %d" % (s["agg_rows"].min(), s["agg_rows"].max()), "dead columns", len(s["dead"]),
              "condition up to %.1e" % s["agg_kappa"].max(), "rows with P B_c = B checked", int(rows.sum()))
        assert np.array_equal(s["dead"], s["dead_by_value"]), (name, l, "a dead column is not a zero coarse diagonal, or the reverse")


def test_lambda_max_brackets_the_eigenvalue(replayed):
    name, kw, nb, levels, dense = replayed
    steps = kw.get("eig_steps", 15)
    for l, L in enumerate(levels):
        A = sr.blocks_to_csr(L["rp"], L["ci"], L["val"], L["nn"])
        if l > 0 and ar.operator_is_fp32(L["bs"], len(L["ci"]), L["nn"]):
            A = ar.rounded_to_fp32(A)
        d = A.diagonal()
        s = 1.0 / np.sqrt(np.where(d != 0, np.abs(d), 1.0))
        true = float(np.linalg.eigvalsh(s[:, None] * (0.5 * (A + A.T)).toarray() * s[None, :])[-1])
        lam, lmax, gersh = float(L["lam"]), float(L["lmax"]), ar.gershgorin_bound(A)
        print(name, "level", l, "lam %.6f lambda_true %.6f lambda_max %.6f Gershgorin %.4f lambda_true / (1.1 lam) %.4f bound %.1e"
              % (lam, true, lmax, gersh, true / (1.1 * lam), L["lmax_bound"] / lmax))
        assert 0.0 < lam <= true * (1.0 + 1e-12), (name, l, lam, true)
        assert lmax == min(1.1 * lam, float(L["step"]["gersh"]) if L["step"] else lmax), (name, l)
        assert lmax <= gersh * (1.0 + 1e-12)
        # (one or two steps: the Rayleigh quotient of the seed, nowhere near.  A last level with a dense inverse: the cycle never
        # reads its lambda_max, and on 12 to 18 rows fifteen steps from the hashed seed can stay 4 % short - see the module's header)
        if steps == 15 and not (dense and l == len(levels) - 1):
            assert true <= 1.1 * lam, (name, l, "lambda_max under-estimates", true, 1.1 * lam)


SPREAD = {}


def test_the_replay_in_other_arithmetic(replayed):
    """One step from the float64 hierarchy's own A_l, B_l and lambda_max_l, in np.longdouble and with every sum reversed."""
    name, kw, nb, levels, dense = replayed
    theta, steps = sr.default_theta(kw.get("strength_threshold", 0.0)), kw.get("eig_steps", 15)
    for l, L in enumerate(levels[:-1]):
        s = L["step"]
        fp32 = l > 0 and ar.operator_is_fp32(L["bs"], len(L["ci"]), L["nn"])
        tol_r = sr.qr_tolerance(s["agg_rows"], s["agg_kappa"], s["agg_bmax"])
        e_t = sr.QR_C * sr.EPS * s["agg_rows"] * s["agg_kappa"]
        bound_p = sr.prolongator_bound(L["rp"], L["ci"], L["val"], s["dinv"], s["agg"], s["n_agg"], s["T"], e_t, s["lmax"])
        for what, dtype, reverse in (("longdouble", LD, False), ("reversed", np.float64, True)):
            o = sr.coarsen_step(L["rp"], L["ci"], L["val"], L["B"], theta, nb, steps, fp32, s["lmax"], dtype, reverse)
            assert o["stop"] is None and o["n_ambiguous"] == 0
            for k in ("ident", "sptr", "scol", "root", "agg", "live", "pptr", "pcol", "cptr", "ccol", "dead", "dead_by_value"):
                assert np.array_equal(o[k], s[k]), (name, l, what, k)
            assert (o["mis_rounds"], o["n_agg"]) == (s["mis_rounds"], s["n_agg"])
            err_r = np.abs(np.asarray(o["R"] - s["R"], dtype=np.float64)).reshape(s["n_agg"], -1).max(axis=1)
            c_needed = float((err_r / np.maximum(tol_r / sr.QR_C, 1e-300)).max())
            err_p = np.abs(np.asarray(o["pval"] - s["pval"], dtype=np.float64))
            ratio_p = float((err_p / np.maximum(bound_p, 1e-300)).max())
            spread = abs(float(o["lmax"]) - float(s["lmax"])) / float(s["lmax"])
            tight_r = float((tol_r / np.maximum(np.abs(s["R"]).reshape(s["n_agg"], -1).max(axis=1), 1e-300)).max())
            tight_p = float(bound_p.max() / np.abs(s["pval"]).max())
            print(name, "level", l, what, "QR constant needed %.3f" % c_needed, "P err / bound %.4f" % ratio_p,
                  "lambda_max spread %.1e (carried bound %.1e)" % (spread, s["lmax_bound"] / float(s["lmax"])),
                  "tightness R %.1e P %.1e" % (tight_r, tight_p))
            SPREAD[(name, l, what)] = (c_needed, ratio_p, spread)
            assert c_needed <= sr.QR_C, (name, l, what, c_needed)
            assert ratio_p <= 1.0, (name, l, what, ratio_p)
            assert spread <= sr.LMAX_SPREAD, (name, l, what, spread)
            assert abs(float(o["lmax"]) - float(s["lmax"])) <= s["lmax_bound"]
            assert tight_r <= 1e-9 and tight_p <= 1e-9, (name, l, tight_r, tight_p)


def test_a_wrong_set_up_is_told_apart():
    """What the replay is for: the mistakes of the issue, made in the replay, change what the device is compared with."""
    K, bs, nb, B0 = _box()
    rp, ci, val = sr.blocks_from_csr(K, bs)
    ok = sr.coarsen_step(rp, ci, val, B0, 0.25, nb)
    # theta where theta^2 belongs: other strong couplings, hence other aggregates
    dinv, ident, dnorm, gersh, _ = sr.diagonal(rp, ci, val)
    sptr, scol, _, _, _ = sr.strength(rp, ci, val, dnorm, np.sqrt(0.25))
    assert len(scol) != len(ok["scol"])
    # omega = 1 / lambda_max: P outside its bound
    e_t = sr.QR_C * sr.EPS * ok["agg_rows"] * ok["agg_kappa"]
    bound = sr.prolongator_bound(rp, ci, val, dinv, ok["agg"], ok["n_agg"], ok["T"], e_t, ok["lmax"])
    wrong = sr.smooth_prolongator(rp, ci, val, dinv, ok["agg"], ok["n_agg"], ok["T"], ok["lmax"] * 4.0 / 3.0)[2]
    assert (np.abs(wrong - ok["pval"]) > bound).any()
    # a power iteration one step short
    short = sr.power_iteration(rp, ci, val, dinv, 1e9, 14)[0]
    full = sr.power_iteration(rp, ci, val, dinv, 1e9, 15)[0]
    assert abs(short - full) > 16 * sr.LMAX_SPREAD * full
