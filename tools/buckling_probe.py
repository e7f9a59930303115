"""Linear buckling on one box: (a) the fused pencil product of 8 columns against the two block products it replaces (HIP events,
fs_spmv_multi_pencil_benchmark), (b) the phase split of a 4-mode LinearElasticitySolver.solve_buckling (static solve, K and K_G
assembly, AMG set-up, LOBPCG), with the fused product and with two passes.  Prints one JSON line.

    python tools/buckling_probe.py [cells per side = 80] [repetitions = 20]
"""
import copy
import json
import os
import sys
from collections import OrderedDict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
from fenicssolver_amd import backend

QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}
E, NU = 2e11, 0.3


def product(n, reps):
    mesh = backend.DeviceMesh.box(n, n, n)
    V = backend.DeviceSpace(mesh, 3, 1)
    mu, lm = E / (2 * (1 + NU)), E * NU / ((1 + NU) * (1 - 2 * NU))
    K, KG = backend.DeviceMatrix(V), backend.DeviceMatrix(V)
    K.assemble(lame=(mu, lm))
    xyz = mesh.get()[0]
    u = 1e-3 * np.stack([np.sin(xyz[:, 0] + 2 * xyz[:, 1]) + xyz[:, 2], np.cos(xyz[:, 1] - xyz[:, 2]) * xyz[:, 0],
                         xyz[:, 0] * xyz[:, 1] + xyz[:, 2] ** 2], axis=1).ravel()
    KG.assemble_geometric((mu, lm), backend.DeviceVector(V.n_local, u))
    out = {"dofs": V.n_owned, "stored_blocks": V.sell_entries, "rounds": []}
    for _ in range(3):                                   # three rounds in one process: the spread is part of the result
        fused, two = backend.spmv_multi_pencil_benchmark(K, KG, 8, reps)
        out["rounds"].append({"fused_ms": fused, "two_pass_ms": two})
    return out


def solve(n, two_pass):
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(1, 1, 1), n, n, n)
    bcs = OrderedDict()
    bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet', 'value': Constant((0.0, 0.0, 0.0))}
    bcs["end"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 1)), 'boundary_id': 2, 'type': 'pressure', 'value': 1e6}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': E, 'poisson_ratio': NU, 'density': 7800.0, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['solver_settings']['buckling_settings'] = {'number_of_modes': 4, 'tolerance': 1e-6}
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = None
    solver = LinearElasticitySolver(s)
    if two_pass:
        inner = backend.buckling_solve
        backend.buckling_solve = lambda *a, **k: inner(*a, two_pass=True, **k)
    try:
        solver.solve_buckling()
    finally:
        if two_pass:
            backend.buckling_solve = inner
    return {"factors": solver.buckling_factors.tolist(), "stats": solver.buckling_stats}


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 80
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    backend.init(0)
    res = {"cells_per_side": n, "product_8_columns": product(n, reps)}
    print(json.dumps(res), flush=True)
    res["solve_warm_up"] = solve(n, False)["stats"]       # first solve of the process: pattern build, allocations
    res["solve_fused"] = solve(n, False)
    res["solve_two_pass"] = solve(n, True)
    print(json.dumps(res))
