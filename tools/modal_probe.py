"""Modal analysis at configs[2] (BoxMesh (0,0,0)-(10,1,1), 472 x 59 x 59, P1, 5.1 M DOF, clamped at x = 0): LOBPCG with the AMG
V-cycle for 6 and 20 modes - iterations, ms per iteration and its split (block products, Gram, V-cycles, the rest: combinations and
host work) - and the block product of m = 8 and 16 columns against m single products (host clock around synchronised loops),
with the bytes each moves against the 8 TB/s peak.  Kernel times: run it once more under `rocprofv3 --kernel-trace --stats`.

    python tools/modal_probe.py [--tol 1e-6] [--modes 6 20] [--reps 20] [--out modal_probe.json]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fenicssolver_amd import backend as B  # noqa: E402
from oracle import fem_oracle as fo  # noqa: E402

PEAK = 8.0e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tol", type=float, default=1e-6)
    ap.add_argument("--modes", type=int, nargs="+", default=[6, 20])
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    B.init(0)
    nx, ny, nz = 472, 59, 59
    V = B.DeviceSpace(B.DeviceMesh.box(nx, ny, nz, (0.0, 0.0, 0.0), (10.0, 1.0, 1.0)), 3, 1)
    mu, lm = fo.lame(2e11, 0.3)
    K, M = B.DeviceMatrix(V), B.DeviceMatrix(V)
    K.assemble(lame=(mu, lm))
    M.assemble(lame=(0.0, 0.0), mass=7800.0)
    nodes = np.arange((nx + 1) * (ny + 1) * (nz + 1))
    cons = ((nodes[nodes % (nx + 1) == 0])[:, None] * 3 + np.arange(3)).ravel().astype(np.int32)
    K.apply_dirichlet(None, cons, np.zeros(cons.size), symmetric=True)
    out = {"n_dof": V.n_owned, "tol": a.tol, "solves": [], "products": []}
    amg = B.AMG(K, nullspace="rigid_body")
    for nm in a.modes:
        lam, _, st = B.eigen_solve(K, M, nm, amg=amg, constrained=cons, tol=a.tol)
        it = max(st["iterations"], 1)
        rest = st["solve_ms"] - st["block_product_ms"] - st["gram_ms"] - st["precond_ms"]
        out["solves"].append({"n_modes": nm, "converged": st["n_converged"], "iterations": st["iterations"],
                              "max_rel_residual": st["max_rel_residual"], "solve_ms": st["solve_ms"],
                              "ms_per_iteration": st["solve_ms"] / it, "block_product_ms_per_it": st["block_product_ms"] / it,
                              "gram_ms_per_it": st["gram_ms"] / it, "vcycle_ms_per_it": st["precond_ms"] / it,
                              "combine_and_host_ms_per_it": rest / it, "f1_hz": float(np.sqrt(lam[0]) / (2 * np.pi))})
    amg.close()
    n = V.n_owned
    rng = np.random.default_rng(1)
    for m in (8, 16):
        X = [B.DeviceVector(V.n_local, rng.standard_normal(V.n_local)) for _ in range(m)]
        Y = [B.DeviceVector(n) for _ in range(m)]
        B.spmv_multi(K, X, Y)
        B.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            B.spmv_multi(K, X, Y)
        B.synchronize()
        t_multi = (time.perf_counter() - t0) / a.reps * 1e3
        for j in range(m):
            K.spmv(X[j], Y[j])
        B.synchronize()
        t0 = time.perf_counter()
        for _ in range(a.reps):
            for j in range(m):
                K.spmv(X[j], Y[j])
        B.synchronize()
        t_single = (time.perf_counter() - t0) / a.reps * 1e3
        # required bytes: values (9 per block entry) + 4-byte columns once, x read and y written per column
        val_bytes = (V.sell_entries // 9) * (9 * 8 + 4)          # sell_entries counts scalar entries: 9 per 3 x 3 block
        req_multi = val_bytes * ((m + 7) // 8) + m * 16 * n
        req_single = m * (val_bytes + 16 * n)
        out["products"].append({"m": m, "multi_ms": t_multi, "singles_ms": t_single, "ratio": t_multi / t_single,
                                "multi_frac_of_peak": req_multi / (t_multi * 1e-3) / PEAK,
                                "singles_frac_of_peak": req_single / (t_single * 1e-3) / PEAK,
                                "note": "host clock around synchronised loops; fs_spmv_multi includes packing the columns into a block"})
    s = json.dumps(out, indent=1)
    print(s)
    if a.out:
        with open(a.out, "w") as f:
            f.write(s)


if __name__ == "__main__":
    main()
