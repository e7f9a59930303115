"""The fused step of the explicit finite-strain marcher (k_hdyn_step) on the 80^3-cell box (81^3 nodes, 1.59 M dofs) for the four energies
with constant parameters and Mooney-Rivlin with per-cell rows, next to what it replaces, in the same process: the internal-force gather
of fs_assemble_hyperelastic launched on its own (k_hyper_force_gather / k_hm_force) and the step of the linear explicit marcher (one
product with K and k_dynx_update).

    python tools/hyperelastic_dynamics_probe.py [--reps 5] [--steps 200]
        device time per step of --steps-step batches (HIP events around the batch: fs_march_info.device_ms), median of --reps batches after a
        warm-up batch, and the synchronised host clock of a force call; one JSON line
    rocprofv3 --kernel-trace --stats -d out -- python tools/hyperelastic_dynamics_probe.py --reps 2
        the per-kernel times (tools/kernel_stats_csv.py turns the database into profiles/hyperelastic_dynamics_kernel_stats.csv)
"""
import argparse
import ctypes as C
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--cells", type=int, default=80)
    args = ap.parse_args()
    from fenicssolver_amd import backend, _lib as L
    backend.init()
    n, steps = args.cells, args.steps
    dm = backend.DeviceMesh.box(n, n, n, (0.0, 0.0, 0.0), (1.0, 1.0, 1.0))
    V = backend.DeviceSpace(dm, 3, 1)
    nc = dm.info()[1]
    nd = V.n_owned
    co = dm.get(want_coords=True, want_cells=False, want_gids=False)[0].reshape(-1, 3)
    u0 = (0.02 * np.stack([np.sin(2 * co[:, 0] + co[:, 1]), co[:, 0] * co[:, 2], np.cos(co[:, 1])], axis=1)).ravel()
    lame = (3.8, 5.8)
    # the lumped mass of rho = 1
    M = backend.DeviceMatrix(V)
    M.assemble(lame=(0.0, 0.0), mass=1.0)
    ones, md = backend.DeviceVector(V.n_local, np.ones(V.n_local)), backend.DeviceVector(nd)
    M.spmv(ones, md)
    m = md.get()[:nd].copy()
    M.close()
    dt = 0.2 * (1.0 / n) / math.sqrt(lame[1] + 2.0 * lame[0])               # a fifth of h / c_p: below the stable bound of this mesh
    face = np.nonzero(np.abs(co[:, 0]) < 1e-12)[0]
    dofs = (face[:, None] * 3 + np.arange(3)[None, :]).ravel().astype(np.int32)
    vals = u0[dofs]
    sf, sg = np.ones(steps), np.ones(steps)
    cases = [("neo_hookean", dict(lame=lame)), ("st_venant_kirchhoff", dict(lame=lame, model="st_venant_kirchhoff")),
             ("mooney_rivlin", dict(lame=None, model="mooney_rivlin", params=(1.2, 0.4, 6.0))),
             ("yeoh", dict(lame=None, model="yeoh", params=(1.5, -0.1, 0.02, 6.0))),
             ("mooney_rivlin_per_cell", dict(lame=None, model="mooney_rivlin", params=("cell", np.tile([1.2, 0.4, 6.0], (nc, 1)))))]
    out = {"n_dofs": nd, "n_cells": nc, "steps_per_batch": steps, "reps": args.reps, "dt": dt}

    def batches(advance):
        advance()                                                          # warm-up: code objects, the receiver-free flags
        t = []
        for _ in range(args.reps):
            o = advance()
            assert o["n_nonfinite"] == 0
            t.append(1e3 * o["device_ms"] / steps)
        return {"median_us": float(np.median(t)), "all_us": [round(x, 2) for x in t]}

    # the linear explicit marcher on the same mesh, mass and step
    K = backend.DeviceMatrix(V)
    K.assemble(lame=lame)
    lin = backend.ExplicitDynamicsState(V)
    lin.configure(dt, 0.1, m, dirichlet_dofs=dofs, dirichlet_values=vals)
    lin.start(K, u0, np.zeros(nd))
    out["linear_explicit_step"] = batches(lambda: lin.advance(K, sf, sg, traces=False, energy=False, info=True))
    ud, r = backend.DeviceVector(V.n_local, u0), backend.DeviceVector(nd)
    for name, kw in cases:
        st = backend.HyperelasticDynamicsState(V, **kw)
        st.configure(dt, 0.1, m, dirichlet_dofs=dofs, dirichlet_values=vals)
        st.start(u0, np.zeros(nd))
        out[name + "_fused_step"] = batches(lambda: st.advance(sf, sg, traces=False, energy=False, info=True))
        # the force gather of fs_assemble_hyperelastic on its own, at the state the march has reached: no tangent, no cell pass (info = NULL)
        u_now = st.get()[0]
        ud.set(np.concatenate([u_now, np.zeros(V.n_local - nd)]))
        keep = []
        form = backend._hyper_form("hyperelastic_dynamics_probe", V, kw.get("lame"), kw.get("model", "neo_hookean"), kw.get("params"), False, keep)
        call = lambda: L.check(L.load().fs_assemble_hyperelastic(V.h, None, r.h, ud.h, C.byref(form), L.FS_HYPER_FORCE, None), "force")
        call()
        t = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            for _ in range(20):
                call()                                                     # (each call waits for the device)
            t.append((time.perf_counter() - t0) * 1e6 / 20)
        out[name + "_force_call_host_clock_us"] = float(np.median(t))
        st.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
