"""BASELINE.json configs[2] (vector P1 cantilever, 5.1 M DOF) three ways: homogeneous Lame constants, per-cell (mu, lambda) pairs
that all hold those constants (FS_COEF_CELL_LAME), and two materials (E ratio 20 across x = 5, different nu).  For each: the
assembly time (host clock around a synchronise, after a warm-up, best and mean of --reps), AMG set-up time, iteration count and
solve time.  Kernel times come from a separate run under rocprofv3 --kernel-trace --stats.  One JSON line per variant.

    python tools/elasticity_materials_probe.py [--size 2] [--reps 5]      (sizes: 0 = 118x15x15, 1 = 236x30x30, 2 = configs[2])
"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np                                     # noqa: E402
from fenicssolver_amd import backend as B              # noqa: E402

SIZES = ((118, 15, 15), (236, 30, 30), (472, 59, 59))


def lame(E, nu):
    return E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=2)
    ap.add_argument("--reps", type=int, default=5)
    args = ap.parse_args()
    B.init(0)
    nx, ny, nz = SIZES[args.size]
    mesh = B.DeviceMesh.box(nx, ny, nz, (0, 0, 0), (10., 1., 1.))
    V = B.DeviceSpace(mesh, 3)
    xyz, cells, _ = mesh.get(True, True, False)
    left = xyz[cells.astype(np.int64)][:, :, 0].mean(axis=1) < 5.0
    del cells
    nodes = np.arange((nx + 1) * (ny + 1) * (nz + 1))
    clamp = nodes[nodes % (nx + 1) == 0]
    dofs = (clamp[:, None] * 3 + np.arange(3)).ravel()
    m1, m2 = lame(2e11, 0.27), lame(1e10, 0.35)
    variants = [("homogeneous", m1),
                ("per_cell_equal", ("cell", np.tile(m1, (len(left), 1)))),
                ("two_materials", ("cell", np.where(left[:, None], np.array(m1)[None], np.array(m2)[None])))]
    for name, lm in variants:
        A = B.DeviceMatrix(V)
        A.assemble(lame=lm)                            # warm-up (gather tables, code objects)
        B.synchronize()
        ts = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            A.assemble(lame=lm)
            B.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        b, x = B.DeviceVector(V.n_owned), B.DeviceVector(V.n_owned)
        B.assemble_vector(V, b, vector_value=(0, 0, -7800 * 10.))
        A.apply_dirichlet(b, dofs, 0.0, True)
        t0 = time.perf_counter()
        amg = B.AMG(A, nullspace="rigid_body")
        B.synchronize()
        t1 = time.perf_counter()
        st = amg.solve(b, x, rtol=1e-8)
        t2 = time.perf_counter()
        print(json.dumps({"variant": name, "dofs": int(V.n_owned), "cells": int(len(left)),
                          "assembly_ms_best": round(min(ts), 3), "assembly_ms_mean": round(float(np.mean(ts)), 3),
                          "amg_setup_ms": round((t1 - t0) * 1e3, 1), "iterations": int(st["iterations"]),
                          "converged": int(st["converged"]), "true_rel_residual": float(st["true_rel_residual"]),
                          "solve_ms": round((t2 - t1) * 1e3, 1)}), flush=True)
        amg.close()
        A.close()


if __name__ == "__main__":
    main()
