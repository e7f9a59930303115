"""Anisotropic elasticity on one box: what the stiffness assembly costs beside the isotropic per-cell-Lame gather, and what an
orthotropic material does to the AMG-CG solve of a cantilever.  Writes profiles/anisotropic_probe.json in three steps:

    python tools/anisotropic_probe.py assembly [cells per side = 80] [repetitions = 10] --out=assembly.json
        every variant in ONE process, a warm-up assembly first: the isotropic gather with one (mu, lambda) pair per cell (the
        baseline: 16 B of material per source), the new kernel with one material, with three regions, with three regions and
        per-cell frames.  Call times are a host clock around a synchronise and INCLUDE the upload of the per-cell arrays; the
        kernel times come from running this step under `rocprofv3 --kernel-trace --stats -d DIR -o assembly -- python ...`.
    python tools/anisotropic_probe.py solve [nx = 160] [ny = nz = 32] --out=solve.json
        the cantilever 10 x 1 x 1 (clamped at x = 0, loaded at the tip, profiler off): isotropic, orthotropic with E1/E2 = 14 and the
        fibres along the beam, the same with the fibres across it - AMG set-up, CG iterations, solve time.
    python tools/anisotropic_probe.py collect DIR assembly.json solve.json
        the per-kernel averages of the trace database in DIR, merged with the two files.  It reads the sqlite database rocprofv3
        writes (rocpd format: the view `kernels` with the columns `name`, `start`, `end` in ns), as tools/kernel_stats_csv.py does; a
        rocprofv3 that writes another format needs `--output-format rocpd`.

The issue behind this tool asked for HIP events with everything in one process.  The isotropic baseline can only be reached through
fs_assemble_matrix, which uploads its per-cell pairs inside the call, so events around it would time the upload; the kernel trace
gives the kernel alone for both, and the solves run apart because tracing slows the host.
"""
import copy
import glob
import json
import os
import sys
import time
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np                                     # noqa: E402

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
CFRP = {'elastic_moduli': [140e9, 10e9, 8e9], 'poisson_ratios': [0.3, 0.25, 0.4], 'shear_moduli': [5e9, 4.5e9, 3e9]}


def _library(Cv):
    p = [0, 1, 2, 5, 4, 3]
    return np.asarray(Cv)[np.ix_(p, p)]


def assembly(n, reps):
    from fenicssolver_amd import backend as B
    from fenicssolver_amd.LinearElasticitySolver import isotropic_stiffness, orthotropic_stiffness
    B.init(0)
    mesh = B.DeviceMesh.box(n, n, n)
    V = B.DeviceSpace(mesh, 3)
    xyz, cells, _ = mesh.get()
    nc = len(cells)
    x = xyz[cells.astype(np.int64)][:, :, 0].mean(axis=1)
    idx = np.minimum((3 * x).astype(np.int32), 2)
    rng = np.random.default_rng(0)
    Q = np.linalg.qr(rng.standard_normal((nc, 3, 3)))[0]
    Q[:, :, 2] *= np.sign(np.linalg.det(Q))[:, None]
    table = np.stack([_library(orthotropic_stiffness(CFRP['elastic_moduli'], CFRP['poisson_ratios'], CFRP['shear_moduli'])),
                      _library(orthotropic_stiffness([40e9, 12e9, 9e9], [0.28, 0.3, 0.42], [4e9, 3.5e9, 3.2e9])),
                      _library(isotropic_stiffness(3.5e9, 0.35))])
    E, nu = 2e11, 0.27
    pairs = np.tile([E / (2 * (1 + nu)), E * nu / ((1 + nu) * (1 - 2 * nu))], (nc, 1))
    variants = [("isotropic_per_cell_lame", lambda A: A.assemble(lame=("cell", pairs))),
                ("anisotropic_one_material", lambda A: A.assemble_anisotropic((table[:1], None, None))),
                ("anisotropic_three_regions", lambda A: A.assemble_anisotropic((table, idx, None))),
                ("anisotropic_three_regions_frames", lambda A: A.assemble_anisotropic((table, idx, Q)))]
    out = {"cells_per_side": n, "dofs": int(V.n_owned), "cells": int(nc), "stored_values": int(V.sell_entries), "repetitions": reps,
           "call_ms": {}}
    A = B.DeviceMatrix(V)
    for name, run in variants:
        run(A)                                         # warm-up: gather tables, code objects
        B.synchronize()
        ts = []
        for _ in range(reps):
            t0 = time.perf_counter()
            run(A)
            B.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
        out["call_ms"][name] = {"best": round(min(ts), 3), "mean": round(float(np.mean(ts)), 3)}
    return out


def cantilever(n, material):
    from fenicssolver_amd import backend as B
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(10, 1, 1), *n)
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0, 0, 0))}
    bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 10)), 'boundary_id': 2, 'type': 'stress', 'value': Constant((0, 0, -1e6))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = dict({'name': 'beam', 'density': 1600.0, 'thermal_expansion_coefficient': 0.0}, **material)
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['solver_parameters'] = {'krylov_relative_tolerance': 1e-8, 'maximum_iterations': 5000}
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = None
    solver = LinearElasticitySolver(s)
    B.synchronize()
    t0 = time.perf_counter()
    u = solver.solve()
    B.synchronize()
    wall = (time.perf_counter() - t0) * 1e3
    st = {k: (float(v) if isinstance(v, float) else int(v)) for k, v in solver.last_solve_stats.items()
          if isinstance(v, (int, float, np.integer, np.floating)) and not isinstance(v, bool)}
    st["solve_call_wall_ms"] = round(wall, 1)
    st["tip_deflection"] = float(np.abs(u.node_values()[:, 2]).max())
    return st


def solve(n):
    from fenicssolver_amd import backend as B
    B.init(0)
    across = [[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]          # axis 1 (the fibres) along y
    cases = [("isotropic", {'elastic_modulus': 140e9, 'poisson_ratio': 0.3}),
             ("orthotropic_fibres_along_the_beam", {'orthotropic': dict(CFRP)}),
             ("orthotropic_fibres_across_the_beam", {'orthotropic': dict(CFRP), 'material_orientation': across})]
    out = {"cells": list(n), "dofs": 3 * (n[0] + 1) * (n[1] + 1) * (n[2] + 1)}
    out["warm_up"] = cantilever(n, cases[0][1])         # first solve of the process: pattern build, allocations
    for name, material in cases:
        out[name] = cantilever(n, material)
    return out


def collect(trace_dir, assembly_json, solve_json):
    import sqlite3
    asm = json.load(open(assembly_json))
    db = sqlite3.connect(glob.glob(os.path.join(trace_dir, "**", "*.db"), recursive=True)[0])
    rows = db.cursor().execute("select name, end - start from kernels where name like '%elasticity_gather%' or "
                               "name like '%aniso_gather%' order by start").fetchall()
    # the variants ran one after the other, a warm-up call and then the repetitions each (two of them share a kernel name)
    per = asm["repetitions"] + 1
    names = list(asm["call_ms"])
    if len(rows) != per * len(names):
        raise SystemExit("expected %d assembly launches in the trace, found %d" % (per * len(names), len(rows)))
    kernels = {}
    for k, name in enumerate(names):
        chunk = rows[per * k:per * (k + 1)]
        if len({r[0] for r in chunk}) != 1:
            raise SystemExit("variant %s: its launches carry several kernel names" % name)
        t = np.array([r[1] for r in chunk[1:]]) / 1e3
        kernels[name] = {"kernel": chunk[0][0], "launches_timed": len(t), "first_us": round(chunk[0][1] / 1e3, 1),
                         "avg_us": round(float(t.mean()), 1), "min_us": round(float(t.min()), 1), "max_us": round(float(t.max()), 1)}
    res = {"how": "assembly_kernels: rocprofv3 --kernel-trace --stats of the assembly step, one process, the warm-up launch of every "
                  "variant apart (first_us); call_ms: host clock around a synchronise, uploads of the per-cell arrays included; solve: "
                  "a run of its own with the profiler off",
           "assembly": asm, "assembly_kernels": kernels, "solve": json.load(open(solve_json))}
    path = os.path.join(ROOT, "profiles", "anisotropic_probe.json")
    with open(path, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print("wrote", path)


def _emit(result, out):
    if out:
        with open(out, "w") as fh:
            json.dump(result, fh)
    print(json.dumps(result))


if __name__ == "__main__":
    out = next((a[6:] for a in sys.argv if a.startswith("--out=")), None)      # (a profiler may write to stdout as well)
    sys.argv = [a for a in sys.argv if not a.startswith("--out=")]
    what = sys.argv[1] if len(sys.argv) > 1 else "assembly"
    if what == "assembly":
        _emit(assembly(int(sys.argv[2]) if len(sys.argv) > 2 else 80, int(sys.argv[3]) if len(sys.argv) > 3 else 10), out)
    elif what == "solve":
        nx = int(sys.argv[2]) if len(sys.argv) > 2 else 160
        ny = int(sys.argv[3]) if len(sys.argv) > 3 else 32
        _emit(solve((nx, ny, ny)), out)
    elif what == "collect":
        collect(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        sys.exit(__doc__)
