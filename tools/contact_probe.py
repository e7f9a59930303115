"""Frictionless contact on one box: the punch of the contact tests - the box (0,0,0)-(1,1,0.25), its top face pushed down by 2e-3
against a rigid sphere of radius 5 under its face z = 0 - through LinearElasticitySolver.solve() at n^3 cells (n = 80: 1.59 M dofs,
6561 candidates).  Prints the active-set iterations and, per iteration, the milliseconds of the copy + Dirichlet elimination, the
AMG set-up (with the upload of the rotated near-null space), the CG solve and the update kernel (host clock around a device
synchronise), and for scale the mean time of one product with K' (fs_spmv_benchmark, HIP events) in the same process.  One JSON line.

    python tools/contact_probe.py [cells per side = 80] [repetitions of the product = 20]
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
    mesh = backend.DeviceMesh.box(n, n, n, (0.0, 0.0, 0.0), (1.0, 1.0, 0.25))
    V = backend.DeviceSpace(mesh, 3, 1)
    K = backend.DeviceMatrix(V)
    K.assemble(lame=(E / (2 * (1 + NU)), E * NU / ((1 + NU) * (1 - 2 * NU))))
    xyz = mesh.get()[0]
    base = np.flatnonzero(xyz[:, 2] == 0.0)
    rng = np.random.default_rng(0)
    nrm = np.tile([0.0, 0.0, -1.0], (len(base), 1)) + 0.2 * rng.standard_normal((len(base), 3))      # generic frames: full blocks
    frames = backend.ContactFrames(V, base, nrm)
    K.rotate_nodes(frames)
    x, y = backend.DeviceVector(V.n_local, rng.standard_normal(V.n_local)), backend.DeviceVector(V.n_owned)
    rounds = [K.spmv_benchmark(x, y, reps) for _ in range(3)]           # three rounds in one process: the spread is part of the result
    return {"dofs": V.n_owned, "candidates": int(len(base)), "stored_blocks": V.sell_entries, "spmv_ms_rounds": rounds}


def solve(n):
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, Expression, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(1, 1, 0.25), n, n, n)
    bcs = OrderedDict()
    bcs["top"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0.25)), 'boundary_id': 1, 'type': 'Dirichlet',
                  'value': Constant((0.0, 0.0, -2e-3))}
    bcs["base"] = {'boundary': AutoSubDomain(lambda x: near(x[2], 0.0)), 'boundary_id': 2, 'type': 'contact', 'normal': (0.0, 0.0, -1.0),
                   'value': Expression("(pow(x[0] - 0.5, 2) + pow(x[1] - 0.5, 2)) / 10", degree=2)}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': E, 'poisson_ratio': NU, 'density': 7800.0, 'thermal_expansion_coefficient': 0.0}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = None
    solver = LinearElasticitySolver(s)
    solver.solve()
    nodes, lam = solver.contact_forces()
    st = dict(solver.contact_stats)
    st.update(candidates=int(len(nodes)), active=int((lam > 0.0).sum()), total_force=float(lam.sum()))
    return st


if __name__ == "__main__":
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 80
    reps = int(sys.argv[2]) if len(sys.argv) > 2 else 20
    backend.init(0)
    res = {"cells_per_side": n, "product": product(n, reps)}
    print(json.dumps(res), flush=True)
    res["solve"] = solve(n)
    print(json.dumps(res))
