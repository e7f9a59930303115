"""DG1 advection-diffusion on the MI355X: assembly, the cell-block product, BiCGStab with block / point Jacobi and the CG1 projection
on uniform boxes of about 1 M and 10 M DOF (ScalarTransportDGSolver).

    python tools/dg_probe.py [--sizes 35,75] [--out profiles/dg_probe.json]

Box n x n x n has 6 n^3 cells and 24 n^3 DOF.  The system is the exact-linear-state problem of tests/test_gpu_dg.py (Dirichlet on
the whole boundary, kappa = 1, beta = (0.1, 0.05, 0.02), alpha = 500).  Product: mean of 50 launches timed with HIP events inside
one loop of synchronised calls (fs_spmv), i.e. launch + kernel; bytes: fs_krylov_stats.spmv_bytes (algorithmic)."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

PEAK = 8.0e12


def run(n):
    from fenicssolver_amd import backend as B
    from fenicssolver_amd.fem import BoxMesh, Point, FunctionSpace
    mesh = BoxMesh(Point(0.0, 0.0, 0.0), Point(1.0, 1.0, 1.0), n, n, n)
    V = FunctionSpace(mesh, "DG", 1)
    t = time.perf_counter()
    rec = V.device()
    setup_ms = (time.perf_counter() - t) * 1e3
    ndof = V.dim()
    a, t0 = np.array([0.8, 1.3, -0.6]), 2.0
    c, kappa, beta = 3.0, 1.0, np.array([0.1, 0.05, 0.02])
    src = np.full(ndof, c * float(beta @ a))
    A = B.DeviceDGMatrix(rec.space)
    b = B.DeviceVector(ndof)
    kw = dict(conductivity=kappa * c, capacity=c, velocity=beta, alpha=500.0, source=src[rec.device_to_dof])
    A.assemble_transport(b, **kw)
    B.synchronize()
    reps = 5
    t = time.perf_counter()
    for _ in range(reps):
        A.assemble_transport(b, **kw)
    assembly_ms = (time.perf_counter() - t) * 1e3 / reps
    dofs = V.facet_nodes(np.nonzero(mesh.exterior_facets())[0])
    Tstar = V.node_coordinates() @ a + t0
    A.apply_dirichlet(b, rec.dof_to_device[dofs], Tstar[dofs])
    x = B.DeviceVector(ndof, np.random.default_rng(0).standard_normal(ndof))
    y = B.DeviceVector(ndof)
    A.spmv(x, y)
    B.synchronize()
    t = time.perf_counter()
    for _ in range(50):
        A.spmv(x, y)
    spmv_call_us = (time.perf_counter() - t) * 1e6 / 50
    out = dict(n=n, cells=mesh.num_cells(), dof=ndof, space_setup_ms=setup_ms, assembly_ms=assembly_ms, spmv_call_us=spmv_call_us)
    for pc in ("block_jacobi", "jacobi"):
        x.fill(0.0)
        st = B.dg_krylov_solve(A, b, x, rtol=1e-12, max_iter=20000, precond=pc)
        err = float(np.abs(x.get(ndof)[rec.dof_to_device] - Tstar).max() / np.abs(Tstar).max())
        out[pc] = dict(iterations=st["iterations"], converged=st["converged"], solve_ms=st["solve_ms"],
                       ms_per_iteration=st["solve_ms"] / max(st["iterations"], 1), spmv_us=st["spmv_ms"] * 1e3,
                       spmv_bytes=st["spmv_bytes"], bytes_per_row=st["spmv_bytes"] / ndof,
                       spmv_fraction_of_8TBs=(st["spmv_bytes"] / (st["spmv_ms"] * 1e-3)) / PEAK if st["spmv_ms"] > 0 else None,
                       true_rel_residual=st["true_rel_residual"], max_rel_error=err)
    # projection
    if rec.cg1 is None:
        rec.cg1 = B.DeviceSpace(rec.mesh, 1, 1)
    nv = mesh.num_vertices()
    bp = B.DeviceVector(nv)
    B.assemble_dg_projection(rec.space, x, rec.cg1, bp)
    B.synchronize()
    t = time.perf_counter()
    for _ in range(reps):
        B.assemble_dg_projection(rec.space, x, rec.cg1, bp)
    out["projection_rhs_ms"] = (time.perf_counter() - t) * 1e3 / reps
    t = time.perf_counter()
    M = B.DeviceMatrix(rec.cg1)
    M.assemble(mass=1.0)
    p = B.DeviceVector(nv)
    st = B.krylov_solve(M, bp, p, rtol=1e-12, max_iter=2000, precond="jacobi", method="cg")
    out["projection_ms"] = (time.perf_counter() - t) * 1e3 + out["projection_rhs_ms"]
    out["projection_cg_iterations"] = st["iterations"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="35,75")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    from fenicssolver_amd import backend as B
    B.init(0)
    res = [run(int(s)) for s in args.sizes.split(",")]
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
