"""The tangent and internal-force kernels of the four hyperelastic energies on the 80^3-cell box (81^3 nodes, 1.59 M dofs), next to the
isotropic linear gather on the same mesh: --reps assemblies of each, constant parameters for all four energies and per-cell rows for
Mooney-Rivlin.  Meant to run under a kernel trace, which gives the per-kernel times the README quotes:

    rocprofv3 --kernel-trace --stats -d out -- python tools/hyperelastic_models_probe.py [--reps 5]

Without the profiler it prints HIP-synchronised host clocks (median of --reps calls) as one JSON line.
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
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cells", type=int, default=80)
    args = ap.parse_args()
    from fenicssolver_amd import backend
    backend.init()
    n = args.cells
    dm = backend.DeviceMesh.box(n, n, n, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    V = backend.DeviceSpace(dm, 3, 1)
    nc = dm.info()[1]
    co = dm.get(want_coords=True, want_cells=False, want_gids=False)[0].reshape(-1, 3)
    u = backend.DeviceVector(V.n_local, (0.02 * np.stack([np.sin(2 * co[:, 0] + co[:, 1]), co[:, 0] * co[:, 2], np.cos(co[:, 1])], axis=1)).ravel())
    K, A, r = backend.DeviceMatrix(V), backend.DeviceMatrix(V), backend.DeviceVector(V.n_owned)
    lame = (3.8, 5.8)
    cases = [("neo_hookean", dict(lame=lame)), ("st_venant_kirchhoff", dict(lame=lame, model="st_venant_kirchhoff")),
             ("mooney_rivlin", dict(lame=None, model="mooney_rivlin", params=(1.2, 0.4, 6.0))),
             ("yeoh", dict(lame=None, model="yeoh", params=(1.5, -0.1, 0.02, 6.0))),
             ("mooney_rivlin_per_cell", dict(lame=None, model="mooney_rivlin", params=("cell", np.tile([1.2, 0.4, 6.0], (nc, 1)))))]
    out = {"n_dofs": V.n_owned, "n_cells": nc}
    out["linear_gather_ms"] = _median_ms(lambda: A.assemble(lame=lame), args.reps)
    for name, kw in cases:
        info = backend.assemble_hyperelastic(V, u, K=K, r=r, **kw)
        assert info["n_inverted"] == 0
        out[name + "_tangent_ms"] = _median_ms(lambda: backend.assemble_hyperelastic(V, u, K=K, **kw), args.reps)
        out[name + "_force_and_cells_ms"] = _median_ms(lambda: backend.assemble_hyperelastic(V, u, r=r, **kw), args.reps)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
