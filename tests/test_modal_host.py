"""Modal analysis of LinearElasticitySolver on the host side (no GPU): modal_settings defaults and range checks, the refusals
that must come before any device call, and the ctypes structs of the eigensolver against the header."""
import copy
import os
import re
from collections import OrderedDict

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
QUIET = {"logging_level": 50, "logging_file": None, "plotting_freq": 0, "saving_freq": 0}


def _solver(clamped=True, modal=None, n=(4, 2, 2)):
    from fenicssolver_amd.fem import BoxMesh, Point, VectorFunctionSpace, AutoSubDomain, Constant, near
    from fenicssolver_amd import SolverBase as SB
    from fenicssolver_amd.LinearElasticitySolver import LinearElasticitySolver
    mesh = BoxMesh(Point(0, 0, 0), Point(4, 1, 1), *n)
    bcs = OrderedDict()
    if clamped:
        bcs["fixed"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 0)), 'boundary_id': 1, 'type': 'Dirichlet',
                        'value': Constant((0, 0, 0))}
    bcs["tip"] = {'boundary': AutoSubDomain(lambda x: near(x[0], 4)), 'boundary_id': 2, 'type': 'stress', 'value': Constant((0, 0, -1e6))}
    s = copy.deepcopy(SB.default_case_settings)
    s['material'] = {'name': 'steel', 'elastic_modulus': 2e11, 'poisson_ratio': 0.3, 'density': 7800,
                     'thermal_expansion_coefficient': 2e-6}
    s['function_space'] = VectorFunctionSpace(mesh, "Lagrange", 1)
    s['boundary_conditions'] = bcs
    s['solver_settings']['reference_values'] = {'temperature': 293}
    if modal is not None:
        s['solver_settings']['modal_settings'] = modal
    s['report_settings'] = dict(QUIET)
    s['temperature_distribution'] = None
    return LinearElasticitySolver(s)


@pytest.fixture
def no_device(monkeypatch):
    """Every entry point that would reach the GPU fails the test."""
    from fenicssolver_amd import backend
    from fenicssolver_amd import fem

    def boom(*a, **k):
        raise AssertionError("a device call was made before the refusal")
    for name in ("DeviceMatrix", "DeviceVector", "DeviceSpace", "DeviceMesh", "AMG", "eigen_solve", "init"):
        monkeypatch.setattr(backend, name, boom)
    monkeypatch.setattr(fem.FunctionSpace, "device", boom, raising=False)
    return boom


def test_modal_settings_defaults():
    assert _solver().modal_settings() == {'number_of_modes': 6, 'tolerance': 1e-8, 'max_iterations': 500, 'shift': 0.0}
    ms = _solver(modal={'number_of_modes': 12, 'shift': 2.5}).modal_settings()
    assert ms['number_of_modes'] == 12 and ms['shift'] == 2.5 and ms['tolerance'] == 1e-8


@pytest.mark.parametrize("bad", [{'number_of_modes': 0}, {'number_of_modes': 33}, {'number_of_modes': 2.5},
                                 {'number_of_modes': True}, {'tolerance': 0.0}, {'tolerance': -1e-8},
                                 {'max_iterations': 0}, {'shift': -1.0}, {'shift': 'big'}, {'modes': 4}])
def test_modal_settings_range_checks(bad, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError):
        _solver(modal=bad).solve_modal()


def test_free_free_without_shift_is_refused_before_any_device_call(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    with pytest.raises(SolverError, match="shift"):
        _solver(clamped=False).solve_modal()


def test_too_many_modes_for_the_free_dofs(no_device):
    from fenicssolver_amd.SolverBase import SolverError
    # 2 x 1 x 1 cells: 12 vertices, 4 of them clamped -> 24 free dofs
    with pytest.raises(SolverError, match="free dofs"):
        _solver(modal={'number_of_modes': 24}, n=(2, 1, 1)).solve_modal()


def test_several_ranks_are_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    from fenicssolver_amd import parallel
    solver = _solver()
    monkeypatch.setattr(parallel, "world", lambda: (0, 2))
    with pytest.raises(SolverError, match="one rank"):
        solver.solve_modal()


def test_periodic_space_is_refused_before_any_device_call(monkeypatch, no_device):
    from fenicssolver_amd.SolverBase import SolverError
    solver = _solver()
    monkeypatch.setattr(solver.function_space, "periodic_pairs", lambda: (np.array([0]), np.array([1])), raising=False)
    with pytest.raises(SolverError, match="periodic"):
        solver.solve_modal()


def _header_struct(name):
    header = open(os.path.join(ROOT, "include", "fenicssolver_amd.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (name, name), header, flags=re.S).group(1)
    return [tuple(d.split()) for d in (x.strip() for x in body.split(";")) if d]


@pytest.mark.parametrize("name", ["fs_eigen_opts", "fs_eigen_stats"])
def test_eigen_structs_match_the_header(name):
    import ctypes as C
    from fenicssolver_amd import _lib
    ctype = {"int": C.c_int, "double": C.c_double, "uint64_t": C.c_uint64, "int64_t": C.c_int64}
    fields = _header_struct(name)
    py = getattr(_lib, name)._fields_
    assert [f[1] for f in fields] == [p[0] for p in py]
    assert [ctype[f[0]] for f in fields] == [p[1] for p in py]


def test_modal_entry_points_are_bound():
    from fenicssolver_amd import _lib
    for name in ("fs_spmv_multi", "fs_vector_gram", "fs_eigen_solve"):
        assert name in _lib.SIGNATURES
    assert hasattr(_lib.load(), "fs_eigen_solve")
