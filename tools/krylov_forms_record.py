#!/usr/bin/env python3
"""Record what every single-GPU iteration form of fs_krylov_solve returns, as hashes: one JSON line per solve.

Two records made from two commits are compared line by line (`diff`): a host-side change of the solver that reorders a launch or
drops an argument changes a hash.  The solves are the seven of tests/test_gpu_cg_guard.py::_solves (converged, iteration limits
1 / 2 / 36 / 37, nonzero guess, repeat) under each setting of SETTINGS below.  `launches` is recorded only where the progress
words are off (option cg_mirror = 0 or FS_CG_MIRROR=0): with them it depends on host timing.

    python tools/krylov_forms_record.py --out profiles/NAME.jsonl
    python tools/krylov_forms_record.py --host-leg 200        # wall clock of 200 back-to-back default solves of the 24^3 box
"""
import argparse
import hashlib
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

from fenicssolver_amd import backend as gpu  # noqa: E402
from test_gpu_cg_guard import NAMES, _box_system, _solves  # noqa: E402

DEFAULTS = {"cg_mirror": 1, "cg_pair": 1, "cg_guard": 1, "cg_fused": -1, "cg_graph": -1, "row_dictionary": 1, "box_iter": 0,
            "box_iter_min_rows": 400000, "lattice_order": -1, "lattice_check": 0}

# (name, box, options, keyword arguments of krylov_solve, rtol of the converged solve)
CUBES = [("defaults", {}), ("cg_mirror=0", {"cg_mirror": 0}), ("cg_pair=0", {"cg_pair": 0}), ("cg_guard=0", {"cg_guard": 0}),
         ("cg_fused=0", {"cg_fused": 0}), ("cg_fused=0,cg_graph=0", {"cg_fused": 0, "cg_graph": 0}),
         ("cg_fused=0,row_dictionary=0", {"cg_fused": 0, "row_dictionary": 0})]
SETTINGS = [(name, dims, opts, {}, rtol) for dims, rtol in (((12, 12, 12), 1e-8), ((40, 40, 40), 1e-12)) for name, opts in CUBES]
SETTINGS += [(name, (40, 3, 3), {}, kw, 1e-10) for name, kw in (
    ("diagonal_scale=False", {"diagonal_scale": False}), ("precond=none", {"precond": "none"}), ("method=bicgstab", {"method": "bicgstab"}),
    ("pipelined=True", {"pipelined": True}), ("norm=preconditioned", {"norm": "preconditioned"}))]
# (the marching-window iteration with its row minimum lowered, as tests/test_gpu_kernels.py does)
SETTINGS += [("box_iter=1", (24, 24, 24), {"box_iter": 1, "box_iter_min_rows": 0, "cg_fused": 1}, {}, 1e-10)]
# (scalar CG2 with option lattice_order = 1, one- and two-launch, as tests/test_gpu_p2.py does: the lines of the 8^3 box are shorter than
# a slice, so it keeps the space's own numbering; the 32^3 box - the size of that test - is solved in lattice order)
SETTINGS += [(name, dims, dict(opts, lattice_order=1, lattice_check=1), {}, 1e-10) for dims in ((8, 8, 8), (32, 32, 32))
             for name, opts in (("cg2,lattice_order=1", {}), ("cg2,lattice_order=1,cg_fused=0", {"cg_fused": 0}))]


class _WithArguments:
    """The backend with fixed extra keyword arguments on krylov_solve and the whole stats dict of the last solve kept."""

    def __init__(self, kw):
        self.kw, self.stats = kw, []

    def __getattr__(self, name):
        return getattr(gpu, name)

    def krylov_solve(self, A, b, x, **kw):
        try:
            st = gpu.krylov_solve(A, b, x, **dict(kw, **self.kw))
        except gpu.BackendError as e:      # (a breakdown is a result too: BiCGStab at an iteration limit of 1)
            st = {"error": str(e)}
        self.stats.append(st)
        return dict({k: 0 for k in ("iterations", "converged", "bnorm", "rel_residual", "true_rel_residual", "row_classes", "fused_iteration")}, **st)


def _cg2_system(dims):
    """_box_system on the scalar CG2 space: zero load, the vertices of the two z faces held at 350 and 300."""
    nx, ny, nz = dims
    mesh = gpu.DeviceMesh.box(nx, ny, nz)
    V = gpu.DeviceSpace(mesh, 1, degree=2)
    A = gpu.DeviceMatrix(V)
    A.assemble(stiffness=20.0)
    b = gpu.DeviceVector(V.n_owned)
    b.fill(0.0)
    plane = (nx + 1) * (ny + 1)
    dofs = np.concatenate([np.arange(plane), nz * plane + np.arange(plane)]).astype(np.int32)
    A.apply_dirichlet(b, dofs, np.concatenate([np.full(plane, 350.0), np.full(plane, 300.0)]), symmetric=True)
    return mesh, V, A, b


def _sha(a):
    """sha256 of the array's bytes, its first 16 hex digits (64 bits: ample for a line-by-line comparison, and the record stays small)."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def record(out):
    mirror_off_env = os.environ.get("FS_CG_MIRROR") == "0"
    for name, dims, opts, kw, rtol in SETTINGS:
        mesh, V, A, b = _cg2_system(dims) if name.startswith("cg2") else _box_system(gpu, dims)
        g = _WithArguments(kw)
        try:
            for k, v in opts.items():
                gpu.set_option(k, v)
            solves = _solves(g, V, A, b, rtol)
        finally:
            for k in opts:
                gpu.set_option(k, DEFAULTS[k])
        for what, (keep, hist, x, form), st in zip(NAMES, solves, g.stats):
            line = {"box": "x".join(map(str, dims)), "setting": name, "solve": what, "x": _sha(x), "history": _sha(hist), "form": form}
            for k in ("iterations", "converged", "fused_iteration", "product_kind", "row_classes", "classes_kept", "lattice_order", "error"):
                if k in st:
                    line[k] = st[k]
            if (mirror_off_env or opts.get("cg_mirror") == 0) and "launches" in st:
                line["launches"] = st["launches"]
            out.write(json.dumps(line, separators=(",", ":")) + "\n")
        out.flush()


def host_leg(n):
    """n back-to-back default solves of the 24^3 box: launch overhead is most of the time."""
    mesh, V, A, b = _box_system(gpu, (24, 24, 24))
    x = gpu.DeviceVector(V.n_local)
    for _ in range(5):
        st = gpu.krylov_solve(A, b, x, rtol=1e-10, max_iter=5000)
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        st = gpu.krylov_solve(A, b, x, rtol=1e-10, max_iter=5000)
    gpu.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"host_leg_solves": n, "seconds": dt, "ms_per_solve": 1e3 * dt / n, "iterations": st["iterations"]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="-", help="file for the record (default: standard output)")
    ap.add_argument("--host-leg", type=int, default=0, metavar="N", help="time N default solves of the 24^3 box instead")
    args = ap.parse_args()
    gpu.init(0)
    if args.host_leg:
        host_leg(args.host_leg)
    elif args.out == "-":
        record(sys.stdout)
    else:
        with open(args.out, "w") as f:
            record(f)
