"""Timing of the hyperelastic kernels at BASELINE configs[2] size (472 x 59 x 59 cantilever, 5.11 M DOF) next to the linear
elasticity gather on the same mesh: tangent assembly, internal-force assembly (with the energy / inversion pass), and one Newton
step (assembly + CG-AMG with a fresh hierarchy).  Device times are HIP-synchronised host clocks, median of --reps calls.

    python tools/hyperelastic_probe.py [--reps 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _median_ms(fn, reps):
    from fenicssolver_amd import backend
    fn()
    backend.synchronize()
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        backend.synchronize()
        t.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(t))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    args = ap.parse_args()
    from fenicssolver_amd import backend
    backend.init()
    dm = backend.DeviceMesh.box(472, 59, 59, (0.0, 0.0, 0.0), (8.0, 1.0, 1.0))
    V = backend.DeviceSpace(dm, 3, 1)
    mu, lmbda = 3.8e6, 5.8e6
    nv = V.n_owned // 3
    co = dm.get(want_coords=True, want_cells=False, want_gids=False)[0]
    u = backend.DeviceVector(V.n_local, (0.01 * np.stack([np.sin(co[:, 0]), co[:, 0] * co[:, 1], -0.05 * co[:, 0] ** 2], axis=1)).ravel())
    K = backend.DeviceMatrix(V)
    A = backend.DeviceMatrix(V)
    r = backend.DeviceVector(V.n_owned)
    out = {"n_dofs": V.n_owned}
    out["linear_gather_ms"] = _median_ms(lambda: A.assemble(lame=(mu, lmbda)), args.reps)
    out["tangent_ms"] = _median_ms(lambda: backend.assemble_hyperelastic(V, u, (mu, lmbda), K=K), args.reps)
    out["force_and_cells_ms"] = _median_ms(lambda: backend.assemble_hyperelastic(V, u, (mu, lmbda), r=r, energy=True), args.reps)
    # one Newton step: tangent + force, clamp x = 0, CG + AMG (rigid-body modes) to 1e-8 with a fresh hierarchy
    co3 = co.reshape(-1, 3)
    clamp = np.nonzero(np.abs(co3[:, 0]) < 1e-12)[0]
    dofs = (clamp[:, None] * 3 + np.arange(3)).ravel()
    t0 = time.perf_counter()
    backend.assemble_hyperelastic(V, u, (mu, lmbda), K=K, r=r)
    rhs = backend.DeviceVector(V.n_owned)
    rhs.axpy(-1.0, r)
    K.apply_dirichlet(rhs, dofs, 0.0, symmetric=True)
    amg = backend.AMG(K, nullspace="rigid_body")
    x = backend.DeviceVector(V.n_local)
    st = amg.solve(rhs, x, rtol=1e-8, max_iter=500, norm="preconditioned")
    backend.synchronize()
    out["newton_step_ms"] = (time.perf_counter() - t0) * 1e3
    out["newton_step_amg_setup_ms"] = amg.info()["setup_ms"]
    out["newton_step_cg_ms"] = st["solve_ms"]
    out["newton_step_cg_iterations"] = st["iterations"]
    amg.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
