"""Run by tests/test_gpu_amg_vcycle.py, one process per setting of FS_AMG_FP32 / FS_AMG_NO_NODE_WAVES / FS_AMG_NO_ROW_GROUPS /
FS_AMG_SPGEMM_BLOCK / FS_AMG_SERIAL_QR (the library reads them once per process): amg.apply(r, z) of small hierarchies against the host
replay of the same hierarchy (amg_reference.vcycle_replay), which is rebuilt from the inspection hooks of the AMG object.

Per case: the Galerkin and near-null-space checks of test_gpu_amg._check_hierarchy; every lambda_max against the eigenvalue it bounds;
for three right-hand sides z filled with NaN, the cycle applied twice (same bits), z finite and within the replay's bound in every
component (how tight the bound is goes into the report: the caller asserts it over all cases).  Everything that has to be compared ACROSS processes goes into the .npz file argv[1].

Output lines the caller reads: "report {json}" per case (the levels, which kernels they ran, the figures), "ok" at the end.
argv[2] == "measure": a result outside its bound is reported ("miss") instead of asserted, a case that fails does not end the run."""
import json
import os
import sys
import time

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from fenicssolver_amd import backend as B  # noqa: E402
from oracle import fem_oracle as fo  # noqa: E402
import amg_reference as ar  # noqa: E402
from test_gpu_amg import _check_hierarchy, _elasticity  # noqa: E402

T0 = time.time()
MEASURE = len(sys.argv) > 2 and sys.argv[2] == "measure"
ONLY = sys.argv[3].split(",") if len(sys.argv) > 3 else None
FP32 = os.environ.get("FS_AMG_FP32", "1")[:1] != "0"
NODE_WAVES = "FS_AMG_NO_NODE_WAVES" not in os.environ
ROW_GROUPS = "FS_AMG_NO_ROW_GROUPS" not in os.environ
DATA = os.path.join(ROOT, "tests", "golden", "data")
CUBE_EDGE = 30              # the two-level scalar cube: see test_gpu_amg_vcycle.py
EIG_ROWS = 20000            # levels up to this size have their eigenvalue computed

B.init(0)
out = {}


def say(*a):
    print(*a, flush=True)


# ---- the operators ------------------------------------------------------------------------------------------------------------------
def scalar_p1(co, ce, seed, axis):
    """Variable-coefficient P1 stiffness with the two end planes of an axis held (the near-null-space check needs nodes two
    couplings away from a held one); the oracle's matrix next to it."""
    kc = np.random.default_rng(seed).uniform(0.5, 1.5, len(ce))
    V = B.DeviceSpace(B.DeviceMesh(co, ce))
    A = B.DeviceMatrix(V)
    A.assemble(stiffness=("cell", kc))
    K = fo.assemble_p1_scalar(co, ce, kc)
    t = co[:, axis]
    tol = 1e-9 * (t.max() - t.min())
    dofs = np.nonzero((t <= t.min() + tol) | (t >= t.max() - tol))[0].astype(np.int32)
    assert 0 < len(dofs) < len(co) // 2
    A.apply_dirichlet(None, dofs, np.zeros(len(dofs)), symmetric=True)
    K, _ = fo.apply_dirichlet(K, np.zeros(K.shape[0]), dofs, np.zeros(len(dofs)), True)
    return V, A, K.tocsr()


def case_scalar_box():
    co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), 9, 7, 5)
    V, A, K = scalar_p1(co, ce, 0, 0)
    return V, A, K, None, 1, np.ones((V.n_owned, 1)), dict(coarse_size=20)


def case_scalar_file():
    co, ce = fo.read_dolfin_xml_mesh(os.path.join(DATA, "mesh.xml"))
    V, A, K = scalar_p1(co, ce.astype(np.int32), 1, 2)
    return V, A, K, None, 1, np.ones((V.n_owned, 1)), dict(coarse_size=20)


def case_vector_nb3():
    V, A, b, K, bb, rbm = _elasticity(B, dims=(10, 5, 4))
    B0 = np.tile(np.eye(3), (V.n_owned // 3, 1))
    return V, A, K, None, 3, B0, dict(coarse_size=10)


def vector_rbm(clamp=None, **kw):
    def make():
        V, A, b, K, bb, rbm = _elasticity(B, dims=(13, 3, 4), clamp_components=clamp)
        return V, A, K, rbm, 6, rbm.T.copy(), dict(dict(coarse_size=30), **kw)
    return make


def case_vector_cg2():
    co, ce = fo.box_mesh((0, 0, 0), (2.0, 1.0, 1.0), 6, 4, 4)
    V = B.DeviceSpace(B.DeviceMesh(co, ce), 3, 2)
    A = B.DeviceMatrix(V)
    A.assemble(lame=fo.lame(2e11, 0.27))
    on = co[:, 0] == 0
    ed = V.edges()
    nodes = np.concatenate([np.nonzero(on)[0], len(co) + np.nonzero(on[ed[:, 0]] & on[ed[:, 1]])[0]])
    dofs = (nodes[:, None] * 3 + np.arange(3)).ravel().astype(np.int32)
    A.apply_dirichlet(None, dofs, np.zeros(len(dofs)), symmetric=True)
    rp, ci, va, shape = A.to_csr()
    return V, A, sp.csr_matrix((va, ci, rp), shape=shape), "rigid_body", 6, None, dict(coarse_size=30)


def case_cube():
    co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), CUBE_EDGE, CUBE_EDGE, CUBE_EDGE)
    V, A, K = scalar_p1(co, ce, 2, 2)
    return V, A, K, None, 1, np.ones((V.n_owned, 1)), dict(max_levels=2)


CASES = {
    "scalar_9x7x5": case_scalar_box,
    "scalar_file": case_scalar_file,
    "vector_nb3_10x5x4": case_vector_nb3,
    "vector_rbm_13x3x4": vector_rbm(),
    "vector_rbm_13x3x4_clamp_x": vector_rbm((0,)),
    "vector_cg2_6x4x4": case_vector_cg2,
    "vector_rbm_levels1": vector_rbm(max_levels=1),
    "vector_rbm_levels2": vector_rbm(max_levels=2),
    "vector_rbm_levels3": vector_rbm(max_levels=3),
    "vector_rbm_steps1": vector_rbm(smoother_steps=1),
    "vector_rbm_steps2": vector_rbm(smoother_steps=2),
    "vector_rbm_steps3": vector_rbm(smoother_steps=3),
    "scalar_cube_cheb_coarse": case_cube,
}


def levels_rows(amg, n_levels):
    li = amg.level_info(n_levels - 1)
    return li["n_nodes"] * li["block_size"]


def block_counts(M, br, bc):
    """(blocks per block row, blocks per block column) of a scalar CSR copy of a block matrix."""
    c = M.tocoo()
    pairs = np.unique(np.stack([c.row // br, c.col // bc], axis=1), axis=0)
    return np.bincount(pairs[:, 0], minlength=M.shape[0] // br), np.bincount(pairs[:, 1], minlength=M.shape[1] // bc)


def run(name, make):
    t_case = time.time()
    V, A, A0, nullspace, nb, B0, kw = make()
    steps = kw.get("smoother_steps", 2)
    amg = B.AMG(A, nullspace=nullspace, **kw)
    n_levels = amg.info()["levels"]
    cinv = amg.coarse_inverse()
    report = {"case": name, "n": V.n_owned, "levels": [], "dense_coarse": cinv is not None, "steps": steps}
    if name == "scalar_cube_cheb_coarse":       # more than 2500 rows on the last level: five Chebyshev sweeps instead of k_dense_apply
        assert n_levels == 2 and amg.level_info(1)["n_nodes"] > 2500 and cinv is None, (n_levels, amg.level_info(1)["n_nodes"])
    if "max_levels" in kw and name != "scalar_cube_cheb_coarse":
        assert n_levels == kw["max_levels"], (name, n_levels)
    assert (cinv is None) == (n_levels == 1 or levels_rows(amg, n_levels) > 2500)
    levels = []
    for l in range(n_levels):
        li = amg.level_info(l)
        bs, nn, nnz = li["block_size"], li["n_nodes"], li["nnz_blocks"]
        Al = amg.level_matrix(l, "A")
        P = amg.level_matrix(l, "P") if l + 1 < n_levels else None
        a32 = l > 0 and ar.operator_is_fp32(bs, nnz, nn, FP32, NODE_WAVES)
        p32 = P is not None and ar.transfers_are_fp32(bs, li["p_block_cols"], FP32)
        levels.append({"A": Al, "P": P, "lmax": li["lambda_max"], "a32": a32, "p32": p32})
        for k, M in (("A", Al), ("P", P)):
            if M is not None:
                out["%s/%d/%s_data" % (name, l, k)], out["%s/%d/%s_indices" % (name, l, k)] = M.data, M.indices
                out["%s/%d/%s_indptr" % (name, l, k)], out["%s/%d/%s_shape" % (name, l, k)] = M.indptr, np.array(M.shape)
        out["%s/%d/lmax" % (name, l)] = np.float64(li["lambda_max"])
        rows, _ = block_counts(Al, bs, bs)
        lev = {"bs": bs, "nn": nn, "nnz": nnz, "a32": a32, "lmax": li["lambda_max"], "longest_row": int(rows.max()),
               # the product kernels of a level below the fine one, unless the dense inverse stands in for the whole level
               "family": ar.product_family(bs, nnz, nn, NODE_WAVES, ROW_GROUPS) if l > 0 and not (cinv is not None and l == n_levels - 1) else None}
        if P is not None:
            _, cols = block_counts(P, bs, li["p_block_cols"])
            lev.update(p_shape=[bs, li["p_block_cols"]], p32=p32, p_col_max=int(cols.max()), p_col_min=int(cols.min()))
        # lambda_max = min(1.1 * a Rayleigh quotient of D^-1 A_l, Gershgorin): never above either (A_l as the power iteration reads it)
        if Al.shape[0] <= EIG_ROWS:
            lam, gersh = ar.largest_jacobi_eigenvalue(ar.rounded_to_fp32(Al) if a32 else Al), ar.gershgorin_bound(Al)
            lev.update(lam_true=lam, gersh=gersh, lam_ratio=lam / (1.1 * li["lambda_max"]))
            assert 0.0 < li["lambda_max"] <= min(1.1 * lam, gersh) * (1.0 + 1e-12), (name, l, li["lambda_max"], lam, gersh)
        report["levels"].append(lev)
    if cinv is not None:
        assert cinv.shape == (levels[-1]["A"].shape[0],) * 2
        out["%s/cinv" % name] = cinv
        resid = np.abs(cinv @ levels[-1]["A"].toarray() - np.eye(len(cinv))).max()
        report["cinv_residual"] = float(resid)
        assert resid <= 1e-8, (name, "the dense inverse does not invert the coarsest operator", resid)
    if n_levels >= 2:
        _check_hierarchy(amg, A0, B0 if B0 is not None else amg.level_nullspace(0, nb), nb)
    n = V.n_owned
    rng = np.random.default_rng(7)
    unit = np.zeros(n)
    unit[-1] = 1.0
    prepared = ar.prepare(levels)
    r, z = B.DeviceVector(n), B.DeviceVector(V.n_local)
    report["rhs"] = {}
    for what, rv in (("normal", rng.standard_normal(n)), ("unit", unit), ("ones", np.ones(n))):
        r.set(rv)
        zs = []
        for _ in range(2):
            z.fill(np.nan)                      # the zero-guess sweep has to overwrite all of it
            amg.apply(r, z)
            zs.append(z.get()[:n])
        assert np.array_equal(zs[0], zs[1], equal_nan=True), (name, what, "two applications differ", int((zs[0] != zs[1]).sum()))
        z_ref, e_z = ar.vcycle_replay(prepared, rv, steps, cinv)
        err = np.abs(zs[0] - z_ref)
        fig = {"ratio": float(np.nanmax(err / np.maximum(e_z, 1e-300))) if np.isfinite(zs[0]).any() else float("nan"),
               "tight": float(e_z.max() / np.abs(z_ref).max()), "rel_err": float(np.nanmax(err) / np.abs(z_ref).max())}
        say("figure", name, what, json.dumps(fig))
        try:
            ar.check_cycle(zs[0], z_ref, e_z, (name, what))
        except AssertionError as e:
            if not MEASURE:
                raise
            fig["miss"] = str(e)[:300]
        report["rhs"][what] = fig
        out["%s/z/%s" % (name, what)] = zs[0]
    report["seconds"] = round(time.time() - t_case, 2)
    say("report", json.dumps(report))
    for h in (r, z, amg):
        h.close()


if __name__ == "__main__":          # (amg_setup_worker.py imports the builders above)
    for name, make in CASES.items():
        if ONLY is None or name in ONLY:
            try:
                run(name, make)
            except Exception:
                if not MEASURE:
                    raise
                import traceback
                say("case failed", name, traceback.format_exc())
    if ONLY is None and NODE_WAVES and ROW_GROUPS and FP32 and not any(k in os.environ for k in ("FS_AMG_SPGEMM_BLOCK", "FS_AMG_SERIAL_QR")):
        # the edge of the cube is the smallest whose level 1 has more than 2500 rows: one less, and the dense inverse is back
        co, ce = fo.box_mesh((0, 0, 0), (1, 1, 1), CUBE_EDGE - 1, CUBE_EDGE - 1, CUBE_EDGE - 1)
        V, A, K = scalar_p1(co, ce, 2, 2)
        amg = B.AMG(A, max_levels=2)
        say("cube", CUBE_EDGE - 1, "level 1 rows", amg.level_info(1)["n_nodes"])
        assert amg.coarse_inverse() is not None and amg.level_info(1)["n_nodes"] <= 2500
    np.savez(sys.argv[1], **out)
    say("seconds", round(time.time() - T0, 1))
    say("ok")
