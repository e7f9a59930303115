#!/usr/bin/env python3
"""Record what fs_saddle_solve leaves behind, as hashes: one JSON line per solve.

Two records made from two commits are compared line by line (`diff`): a host-side change of the solver that reorders a launch,
drops an argument or mixes up a workspace buffer changes a hash or a count.  The solves are the cases of
tests/test_gpu_saddle_replay.py (CASES, one saddle_solve / large_deformation_solve call each, rtol = atol = 0) and its three
converging runs, then three Taylor-Hood cases again with FS_SADDLE_GRAPH=1 in the environment (the preconditioner replayed as a
captured graph, which no test exercises).  Per line: the case, the four integers iterations / converged / columns_used /
second_passes, rel_residual and vel_lmax as hex floats, and SHA-256 of x and of every array of backend.saddle_last_cycle()
("used": the columns of H, cs, sn, gamma, y that the cycle wrote, for a workspace whose tails hold what the allocator left).

    python tools/saddle_cycle_record.py --out profiles/NAME.jsonl
    python tools/saddle_cycle_record.py --only cube3_steady3,cube3_transient,ld3,tri2d_transient     # plan "one" of these systems
    python tools/saddle_cycle_record.py --host-leg 200        # wall clock of 200 back-to-back solves of cube4_steady1, plan "one"
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
from test_gpu_saddle_replay import CASES, CONVERGING, PLANS, SEED, _rhs, _stopping_point, _system  # noqa: E402

GRAPH_CASES = [("cube3_steady1", "normal", "one"), ("cube4_steady3", "normal", "one"), ("cube4_transient", "normal", "one")]


def _sha(a):
    """sha256 of the array's bytes, its first 16 hex digits (64 bits: ample for a line-by-line comparison, and the record stays small)."""
    return hashlib.sha256(np.ascontiguousarray(a).tobytes()).hexdigest()[:16]


def _solve(S, b, x0, **kw):
    """One call on system S: the record line without its case."""
    n = S["n"]
    bd, xd = gpu.DeviceVector(n, b), gpu.DeviceVector(n, x0)
    try:
        st = S["solve"](bd, xd, **kw)
    except gpu.BackendError as e:
        return {"error": str(e)}
    finally:
        x = xd.get()[:n]
        for h in (bd, xd):
            h.close()
    c = gpu.saddle_last_cycle()
    line = {"iterations": st["iterations"], "converged": st["converged"], "columns_used": c["kuse"] if c else -1,
            "second_passes": c["second_passes"] if c else -1, "rel_residual": float(st["rel_residual"]).hex(),
            "vel_lmax": float(c["vel_lmax"]).hex() if c else "", "x": _sha(x)}
    if c:
        k = c["kuse"]
        hess = c["R"][:k + 1, :k][~np.tri(k + 1, k, -2, dtype=bool)]        # column j: rows 0 .. j + 1
        line.update({a: _sha(c[a]) for a in ("V", "Z", "cs", "sn", "gamma", "y")}, H=_sha(c["R"]),
                    used=_sha(np.concatenate([hess, c["cs"][:k], c["sn"][:k], c["gamma"][:k + 1], c["y"][:k]])))
    return line


def _case(sysname, what, plan):
    """The call of test_gpu_saddle_replay._run."""
    S = _system(gpu, sysname)
    x0 = np.zeros(S["n"])
    if plan == "restart_guess":
        x0 = 0.1 * np.random.default_rng(SEED + 100).standard_normal(S["n"])
        x0[S["dummy"]] = 0.0
    return _solve(S, _rhs(S, what), x0, rtol=0.0, atol=0.0, nonzero_guess=plan == "restart_guess", **PLANS[plan])


def record(out, only):
    def emit(case, line):
        out.write(json.dumps(dict({"case": case}, **line), separators=(",", ":")) + "\n")
        out.flush()

    if only:
        for sysname in only:
            emit("-".join((sysname, "normal", "one")), _case(sysname, "normal", "one"))
        return
    for c in CASES:
        emit("-".join(c), _case(*c))
    for name, seed in CONVERGING.items():
        S = _system(gpu, name)
        b, i, rtol = _stopping_point(S, seed)[:3]
        emit(name + "-converging", _solve(S, b, np.zeros(S["n"]), rtol=rtol, atol=0.0, max_iter=100, restart=100))
    os.environ["FS_SADDLE_GRAPH"] = "1"          # (the library reads it on every call)
    try:
        for c in GRAPH_CASES:
            emit("-".join(c) + "-FS_SADDLE_GRAPH", _case(*c))
    finally:
        del os.environ["FS_SADDLE_GRAPH"]


def host_leg(n_solves):
    """n back-to-back 20-iteration solves of cube4_steady1: the host enqueues one iteration ahead of the GPU, so the time between its
    launches is most of the time."""
    S = _system(gpu, "cube4_steady1")
    n = S["n"]
    bd, xd = gpu.DeviceVector(n, _rhs(S, "normal")), gpu.DeviceVector(n, np.zeros(n))
    kw = dict(rtol=0.0, atol=0.0, **PLANS["one"])
    st = S["solve"](bd, xd, **kw)
    gpu.synchronize()
    t0 = time.perf_counter()
    for _ in range(n_solves):
        st = S["solve"](bd, xd, **kw)
    gpu.synchronize()
    dt = time.perf_counter() - t0
    print(json.dumps({"host_leg_solves": n_solves, "seconds": dt, "ms_per_solve": 1e3 * dt / n_solves, "iterations": st["iterations"]}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--out", default="-", help="file for the record (default: standard output)")
    ap.add_argument("--only", default="", metavar="SYSTEMS", help="comma list of systems: their (normal, one) case only, no converging or graph runs")
    ap.add_argument("--host-leg", type=int, default=0, metavar="N", help="time N solves of cube4_steady1 instead")
    args = ap.parse_args()
    gpu.init(0)
    only = [s for s in args.only.split(",") if s]
    if args.host_leg:
        host_leg(args.host_leg)
    elif args.out == "-":
        record(sys.stdout, only)
    else:
        with open(args.out, "w") as f:
            record(f, only)
