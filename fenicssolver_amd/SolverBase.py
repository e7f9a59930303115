"""SolverBase — shared runtime of the solvers, MI355X back end.

Drop-in counterpart of FenicsSolver/SolverBase.py (reference): same constructor
(one settings dict, else SolverError), same attributes users touch afterwards
(material, transient_settings, initial_values, boundary_facets, subdomains,
result, ...), same method names, same settings keys and
the same time loop (SolverBase.py:484-546).  What differs is what happens inside
solve_linear_problem / solve_amg (SolverBase.py:592-672): instead of handing a
UFL form to DOLFIN/FFC/PETSc, the operator specification built by
generate_form() is assembled and solved on the GPU through libfsamd.so
(hand-written HIP, fp64).  There is no CPU fall-back: without the library or a
gfx950 device these methods raise.

Documented deviations:
  Q2  The reference silently ignores its Krylov settings and solves by sparse LU, i.e. it returns
      the exact discrete solution.  Here the solve is Jacobi-PCG (AMG-PCG in solve_amg) run to an
      LU-equivalent accuracy by default: relative tolerance min(relative_tolerance, 1e-12) on the
      preconditioned residual norm (config 1: 1e-9 absolute on T ~ 300-350; the recurrence is restarted
      from the true residual until fp64 gives no more).  solver_parameters['krylov_relative_tolerance']
      loosens it for users who want the iterations back.
  Q4  get_time_step with a 'time_series' returns t[i+1]-t[i] (the reference
      subtracts t[i] from itself).
  Q14 plot()/save() cadence is kept (steady runs never save), save() writes PVD/VTU.
"""
from __future__ import annotations

import copy
import logging
import numbers
import os
import time

import numpy as np

from .fem import (SolverError, Mesh, MeshFunction, FunctionSpace, VectorFunctionSpace, Function, Constant,
                  Expression, DirichletBC, interpolate, project, nodal_values, is_constant_value)
from . import forms, case, solid_steps

__all__ = ["SolverError", "SolverBase", "default_report_settings", "default_solver_parameters",
           "default_case_settings"]

default_report_settings = {"logging_level": logging.DEBUG, "logging_file": None,
                           "plotting_freq": 10, "plotting_interactive": True, "plotting_file": None,
                           "saving_freq": 10, "result_filename": None}

# keys of the reference (SolverBase.py:69-72) + the ones this back end honours
default_solver_parameters = {"relative_tolerance": 1e-5,
                             "maximum_iterations": 500,
                             "monitor_convergence": True,
                             }
default_case_settings = {'solver_name': None,
                         'case_name': 'test', 'case_folder': "./", 'case_file': None,
                         'mesh': None, 'fe_degree': 1, 'fe_family': "CG",
                         'function_space': None, 'periodic_boundary': None,
                         'boundary_conditions': None,
                         'body_source': None,
                         'surface_source': None,
                         'initial_values': {},
                         'material': {},
                         'solver_settings': {
                             'transient_settings': {'transient': False, 'starting_time': 0, 'time_step': 0.01,
                                                    'ending_time': 0.03},
                             'reference_values': {},
                             'solver_parameters': default_solver_parameters,
                         },
                         "report_settings": default_report_settings
                         }

KRYLOV_RTOL_CAP = 1e-12     # default accuracy of a drop-in for an LU path (module docstring, Q2)


class SolverBase():
    """shared base class; generate_form() and update_boundary_conditions() come from the derived class"""

    def __init__(self, case_input):
        if not isinstance(case_input, dict):
            raise SolverError('case setup data must be a python dict')
        self.settings = case_input
        self.last_solve_stats = None
        self.load_settings(case_input)
        # one process per GPU (fenicssolver_amd.launch / mpirun export the rank): the counterpart of starting the
        # reference under mpirun (SolverBase.py:102-118)
        from . import parallel
        self.parallel = parallel.world()[1] > 1

    def print(self):
        import pprint
        pprint.PrettyPrinter(indent=4).pprint(self.settings)

    # ------------------------------------------------------------------ settings (fenicssolver_amd/case.py does the work)
    def load_settings(self, s):
        """Discretisation first (mesh + markers + space), then the physics blocks of the dict, then reporting."""
        self.boundary_conditions = s['boundary_conditions']
        bundle, space = case.MeshSource(s).resolve()
        self._adopt_mesh(bundle)
        if space is None:
            self.generate_function_space(s['periodic_boundary'])
        else:
            self.function_space = space
            self.is_mixed_function_space = False
        self.dimension = self.mesh.geometry().dim()
        self.topo_dimension = self.mesh.topology().dim()

        solver_settings = s['solver_settings']
        self.body_source = s.get('body_source') or None
        self.initial_values = s.get('initial_values', {})
        self.material = s['material']
        self.solver_settings = solver_settings
        self.reference_values = solver_settings['reference_values']
        self.transient_settings = solver_settings['transient_settings']
        self.transient = self.transient_settings['transient']
        self._values = case.ValueTranslator(self)

        self.report_settings = self.settings.setdefault('report_settings', default_report_settings)
        self.set_logger(self.report_settings)

    def _adopt_mesh(self, bundle):
        """mesh + its markers; facet markers a file does not carry come from the boundary conditions' SubDomains."""
        self.mesh = bundle.mesh
        if bundle.facet_markers is not None:
            self.boundary_facets = bundle.facet_markers
        else:
            self.generate_boundary_facets()
        if bundle.cell_markers is not None:
            self.subdomains = bundle.cell_markers
        elif not hasattr(self, 'subdomains'):
            self.subdomains = MeshFunction("size_t", self.mesh, self.mesh.topology().dim())

    def set_logger(self, s):
        level = s.get('logging_level', logging.DEBUG)
        logger = logging.getLogger(self.__class__.__name__)
        if not logger.handlers:
            target = s.get('logging_file')
            handler = logging.FileHandler(target) if target else logging.StreamHandler()
            handler.setLevel(level)
            handler.setFormatter(logging.Formatter('%(asctime)s - %(name)s - %(levelname)s - %(message)s'))
            logger.addHandler(handler)
        logger.setLevel(level)
        self.logger = logger

    def logger_or_print(self, msg):
        self.logger.info(msg) if hasattr(self, 'logger') else print(msg)

    # ------------------------------------------------------------------ mesh ingest
    def read_mesh(self, filename):
        """DOLFIN XML (+ _facet_region / _physical_region side files) or ASCII XDMF; HDF5 needs h5py (absent): raises."""
        self._adopt_mesh(case.read_mesh_file(filename))

    def _read_xml_mesh(self, filename):
        self._adopt_mesh(case.read_dolfin_xml(filename))

    def _read_hdf5_mesh(self, filename):
        self._adopt_mesh(case.read_hdf5(filename))

    def generate_function_space(self, periodic_boundary):
        self.is_mixed_function_space = False
        self.settings['periodic_boundary'] = periodic_boundary
        self.function_space = case.build_function_space(self.mesh, self.settings)

    def generate_boundary_facets(self):
        self.boundary_facets = case.mark_boundaries(self.mesh, self.boundary_conditions)

    # ------------------------------------------------------------------ values
    def get_initial_field(self):
        return case.initial_field(self)

    def _load_function(self, filename):
        return case.load_function_file(self.function_space, filename)

    def get_material_value(self, value):
        """numbers pass through; dim x dim nested lists become a tensor (as_matrix); per-region dicts a cell-wise field."""
        if case.is_square_matrix_of_numbers(value, self.dimension):
            return np.asarray(value, dtype=np.float64)
        if isinstance(value, dict):
            return self._translate_dict_value(value)
        return value

    def _translate_dict_value(self, value):
        return forms.VolumeCoefficient("cell", case.cellwise_from_regions(value, self.subdomains))

    def _translate_dict_value_to_function(self, value):
        raise NotImplementedError('not yet implemented')      # as in the reference (SolverBase.py:339-347)

    def translate_value(self, value, function_space=None):
        return self._values(value, function_space)

    def get_variable_name(self):
        return self.settings.get('scalar_name') or self.settings.get('vector_name') or 'unknown'

    def get_boundary_variable(self, bc, variable=None):
        return case.boundary_variable(bc, variable or self.get_variable_name())

    def get_boundary_value(self, bc, variable=None):
        # the reference calls an undefined global here (Appendix B-Q5); the evident intent:
        return self.translate_value(self.get_boundary_variable(bc, variable)['value'])

    def get_body_source(self):
        src = self.body_source
        if isinstance(src, dict):      # {'region': {'subdomain_id': i, 'value': v}}: translate every value, keep the ids
            return {k: dict(item, value=self.translate_value(item['value'])) for k, item in src.items()}
        return self.translate_value(src) if src else None

    # ------------------------------------------------------------------ time loop
    def get_time_step(self, time_iter_):
        return case.TimeGrid(self.transient_settings).step(time_iter_)

    def get_current_time(self, time_iter_=None):
        return case.TimeGrid(self.transient_settings).time(time_iter_ or self.current_step)

    def get_acceleration(self, time_iter_):
        """(SolverBase.py:477-482) second difference of the last three steps, with the reference's own scaling
        (it divides by 1/dt, "FIXME: does not work for non-uniform time step" there)."""
        assert time_iter_ >= 1
        dt, dt_prev = self.get_time_step(time_iter_), self.get_time_step(time_iter_ - 1)
        vel = (self.w_current.vector()._values() - self.w_prev.vector()._values()) / dt
        vel_prev = (self.w_prev.vector()._values() - self.w_pp.vector()._values()) / dt_prev
        a = Function(self.function_space)
        a.vector().set_local((vel - vel_prev) / (1.0 / dt))
        return a

    def init_solver(self):
        """State of the time loop: current, previous and pre-previous fields, all starting from the initial field.
        There are no symbolic trial / test functions here: forms are recognised, not compiled."""
        self.trial_function = self.test_function = None
        self.w_current = self.get_initial_field()
        self.w_prev, self.w_pp = (Function(self.function_space) for _ in range(2))
        for w in (self.w_prev, self.w_pp):
            w.assign(self.w_current)

    def solve_current_step(self):
        """The form is rebuilt every step from (current, previous); then the history rotates pp <- prev <- current and the
        new current field is solved for (SolverBase.py:484-490)."""
        F, bcs = self.generate_form(self.current_step, self.trial_function, self.test_function, self.w_current, self.w_prev)
        self.w_pp.assign(self.w_prev)
        self.w_prev.assign(self.w_current)
        self.result = self.w_current = self.solve_form(F, self.w_current, bcs)

    def _due(self, freq_key):
        """plot / save cadence of the reference: every freq-th step, never at step 0 (so steady runs never fire, B-Q14)."""
        freq = self.report_settings.get(freq_key, 0)
        return bool(freq) and freq > 0 and self.current_step > 0 and self.current_step % freq == 0

    def solve_transient(self):
        self.init_solver()
        ts = self.transient_settings
        self.current_time, self.current_step = ts['starting_time'], 0
        t_end = ts['ending_time'] if ts['transient'] else self.current_time + 1
        pvd = self.report_settings.get('result_filename') or 'result_file.pvd'
        t0 = time.perf_counter()
        while self.current_time < t_end:
            self.solve_current_step()
            self.logger.info("Current step = %d time = %g TimerSolveAll = %.4f", self.current_step, self.current_time,
                             time.perf_counter() - t0)
            if self._due('plotting_freq'):
                self.plot()
            if self._due('saving_freq'):
                self.save(pvd)
                self.logger.info("save data to file `%s` at step: %d , at time: %g", pvd, self.current_step, self.current_time)
            if not ts['transient']:
                break
            self.current_time += self.get_time_step(self.current_step)
            self.current_step += 1
        return self.w_current

    def solve(self):
        self.result = self.solve_transient()
        return self.result

    # ------------------------------------------------------------------ output
    def plot(self):
        try:
            import matplotlib  # noqa: F401
        except ImportError:
            self.logger.info("plot(): matplotlib is not installed; use save() and ParaView")
            return
        if os.environ.get("FENICSSOLVER_BATCH"):
            return
        import matplotlib.pyplot as plt
        co = self.mesh.coordinates()
        v = self.result.vertex_values()
        mag = v if v.ndim == 1 else np.linalg.norm(v, axis=1)
        fig = plt.figure()
        ax = fig.add_subplot(projection='3d')
        p = ax.scatter(co[:, 0], co[:, 1], co[:, 2], c=mag, s=4)
        fig.colorbar(p)
        plt.show()

    def save(self, result_filename):
        """PVD collection + one ASCII VTU per call (the reference streams to dolfin.File, :570-589)."""
        if self.is_mixed_function_space:
            raise SolverError('save() of mixed function spaces is not supported')
        assert result_filename[-4:] == '.pvd'
        root = result_filename[:-4]
        if not hasattr(self, '_saved_frames'):
            self._saved_frames = []
        vtu = "%s%06d.vtu" % (root, len(self._saved_frames))
        write_vtu(vtu, self.mesh, self.w_current, self.get_variable_name())
        self._saved_frames.append((getattr(self, 'current_time', 0.0), os.path.basename(vtu)))
        with open(result_filename, "w") as fh:
            fh.write('<?xml version="1.0"?>\n<VTKFile type="Collection" version="0.1">\n  <Collection>\n')
            for t, f in self._saved_frames:
                fh.write('    <DataSet timestep="%g" part="0" file="%s" />\n' % (t, f))
            fh.write('  </Collection>\n</VTKFile>\n')

    # ------------------------------------------------------------------ the hot path
    def _krylov_options(self):
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        if 'krylov_relative_tolerance' in sp:
            rtol = float(sp['krylov_relative_tolerance'])
        else:
            rtol = min(float(sp.get('relative_tolerance', KRYLOV_RTOL_CAP)), KRYLOV_RTOL_CAP)
        max_iter = int(sp.get('krylov_maximum_iterations', max(int(sp.get('maximum_iterations', 500)), 20000)))
        pc = sp.get('preconditioner', 'jacobi')
        # every name DOLFIN's krylov_solver_preconditioners() lists (the reference forwards the key, SolverBase.py:638-641)
        if pc in ('petsc_amg', 'amg', 'hypre_amg', 'ml_amg'):
            pc = 'amg'        # smoothed aggregation on the device (fs_amg_*)
        elif pc in ('default', 'jacobi', 'bjacobi', 'sor', 'ilu', 'icc', 'additive_schwarz', 'hypre_euclid', 'hypre_parasails'):
            pc = 'jacobi'     # point / block / incomplete-factorisation preconditioners other than Jacobi are not built
        elif pc in ('none', None):
            pc = 'none'
        else:
            raise SolverError("preconditioner '{}' is not supported".format(pc))
        self._krylov_method(None)          # (rejects an unknown solver name here, where the parameters are read)
        return rtol, max_iter, pc

    # names DOLFIN's LinearVariationalSolver / KrylovSolver accept for 'linear_solver' (the reference forwards any key the dolfin
    # solver knows, SolverBase.py:638-641) -> the Krylov kernel of this back end (fs_krylov_solve: CG, BiCGStab)
    _DIRECT_SOLVERS = ('default', 'lu', 'mumps', 'petsc', 'umfpack', 'superlu', 'superlu_dist', 'pastix')
    _SYMMETRIC_KRYLOV = ('cg', 'minres')
    _GENERAL_KRYLOV = ('bicgstab', 'gmres', 'tfqmr', 'richardson')

    def _krylov_method(self, automatic):
        """The Krylov kernel for this solve.  automatic: what the operator calls for ('cg' symmetric / 'bicgstab' not).  A direct
        solver name keeps that choice (run to the LU-equivalent tolerance); 'cg' / 'minres' too (CG on a non-symmetric operator
        would break down: the automatic BiCGStab stays); 'bicgstab' / 'gmres' / 'tfqmr' / 'richardson' select the method for
        general operators - BiCGStab, the one this back end has for scalar and vector spaces (it is also valid on symmetric ones)."""
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        ls = sp.get('linear_solver', 'default')
        if ls in self._DIRECT_SOLVERS or ls in self._SYMMETRIC_KRYLOV:
            return automatic
        if ls in self._GENERAL_KRYLOV:
            if ls != 'bicgstab' and automatic is not None and not getattr(self, '_warned_krylov_alias', False):
                self.logger.info("linear_solver '%s': solved with the BiCGStab kernel of the GPU back end", ls)
                self._warned_krylov_alias = True
            return 'bicgstab'
        raise SolverError("linear_solver '{}' is not a solver name DOLFIN knows ({})".format(
            ls, ', '.join(self._DIRECT_SOLVERS + self._SYMMETRIC_KRYLOV + self._GENERAL_KRYLOV)))

    def set_solver_parameters(self, solver=None):
        """Kept for API parity (SolverBase.py:628-641): returns the Krylov options this back end will use."""
        rtol, max_iter, pc = self._krylov_options()
        return {'linear_solver': 'cg', 'preconditioner': pc, 'relative_tolerance': rtol,
                'maximum_iterations': max_iter}

    def _device_solve(self, A, b, u, label, method="cg", amg=False, near_nullspace=None, operator_key=None, global_operator=None):
        """amg=True: the caller is solve_amg (AMG unless solver_parameters name another preconditioner).
        global_operator: a callable returning the UNDECOMPOSED operator on this rank's GPU (several ranks + AMG: see
        _replicated_amg_solve).
        operator_key: everything the values of A depend on (None: unknown) - an AMG hierarchy is reused only for a call
        that names the same key; a call without one always builds its own."""
        from . import backend
        rtol, max_iter, pc = self._krylov_options()
        automatic = method
        method = self._krylov_method(method)
        V = u.function_space().device()
        x = backend.DeviceVector(V.n_local)            # owned + ghost entries: the input of operator products
        sp_ = self.solver_settings.get('solver_parameters', {}) or {}
        if amg and 'preconditioner' not in sp_:
            pc = 'amg'
            method = automatic         # solve_amg is the reference's CG + AMG path (SolverBase.py:643-672): a general-solver name does not undo it
        if pc == 'amg' and method != "cg" and automatic == "cg":
            # 'gmres' / 'bicgstab' / 'tfqmr' + an AMG preconditioner on a SYMMETRIC operator: the reference would run that Krylov
            # method with GAMG; here the preconditioner is kept and the method is CG, which the operator allows
            self.logger.info("%s: linear_solver '%s' with an AMG preconditioner on a symmetric operator: CG + AMG", label, sp_.get('linear_solver'))
            method = "cg"
        if pc == 'amg' and method != "cg":
            self.logger.warning('%s: the AMG hierarchy is built for symmetric problems; using Jacobi', label)
            pc = 'jacobi'
        # PETSc's KSPCG default: convergence on the preconditioned residual norm; it is
        # also what keeps badly scaled operators (e.g. permittivities of 1e-10 next to identity rows) honest
        norm = sp_.get('norm_type', 'preconditioned' if (method == "cg" and pc in ("jacobi", "amg")) else 'unpreconditioned')
        loc = u.function_space().localizer()
        from . import parallel as _par
        # several GPUs: 'distributed' (default since round 4) - the hierarchy of the undecomposed operator on every rank, its fine
        # level working on this rank's rows; 'replicated' - every rank solves the whole gathered system (round 3: the iteration
        # count of one GPU, no speed-up); 'schwarz' - rank-local hierarchies
        mode = sp_.get('amg_decomposition', 'distributed')
        replicated = (pc == 'amg' and loc is not None and _par.world()[1] > 1 and global_operator is not None
                      and hasattr(loc, 'l2g')            # (a CG2 space on a distributed mesh has no global node numbering: Schwarz)
                      and isinstance(near_nullspace, (str, type(None)))
                      and mode in ('replicated', 'distributed'))
        if replicated:
            stats = self._replicated_amg_solve(b, x, V, loc, u.function_space()._ncomp, global_operator, operator_key,
                                               near_nullspace, rtol, min(max_iter, int(sp_.get('maximum_iterations', 500))), norm,
                                               float(sp_.get('amg_strength_threshold', 0.0)), A_local=A if mode == 'distributed' else None)
        elif pc == 'amg':
            # several GPUs, solver_parameters['amg_decomposition'] = 'schwarz': every rank builds the hierarchy of its own
            # diagonal block (additive Schwarz, no overlap, no coarse space: the iteration count grows with the number of parts)
            if near_nullspace is not None and not isinstance(near_nullspace, str) and loc is not None:
                near_nullspace = np.stack([loc.nodes(v)[:V.n_owned] for v in np.asarray(near_nullspace)])
            # The hierarchy depends on the operator only: time steps / load cases that re-assemble the SAME matrix (quasi-static
            # elasticity with time-dependent loads, LinearElasticitySolver.py:216-220 with solving_dynamics False) reuse it -
            # at configs[2] the set-up (0.15 s) costs more than the solve (0.12 s).  The key holds everything the matrix
            # values depend on; the cached hierarchy keeps its own (identical) fine matrix alive.
            key = operator_key
            hierarchy, reused = self._amg_hierarchy(A, key, near_nullspace)
            stats = hierarchy.solve(b, x, rtol=rtol, max_iter=min(max_iter, int(sp_.get('maximum_iterations', 500))),
                                    norm=norm)
            stats.update({'amg_' + k: v for k, v in hierarchy.info().items()})
            stats['amg_reused'] = reused
            if key is None:
                hierarchy.close()
        else:
            stats = backend.krylov_solve(A, b, x, rtol=rtol, max_iter=max_iter, precond=pc, method=method, norm=norm)
        self.last_solve_stats = stats
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        if sp.get('monitor_convergence'):
            self.logger.info("%s: Krylov iterations=%d converged=%d ||r||/||b||=%.3e (true %.3e) solve %.2f ms",
                             label, stats['iterations'], stats['converged'], stats['rel_residual'],
                             stats['true_rel_residual'], stats['solve_ms'])
        if stats['converged'] != 1:
            # The LU-equivalent default (1e-12) may lie below what fp64 attains on a badly conditioned operator: a solve that
            # stopped short of it but reached the accuracy this back end promised before (1e-8) is a result, with a warning -
            # not an error; a tolerance the user asked for explicitly stays binding.
            # (that is 'krylov_relative_tolerance', or the reference's own key 'relative_tolerance' below the 1e-8 of the fallback)
            user_tol = 'krylov_relative_tolerance' in sp or float(sp.get('relative_tolerance', 1.0)) < 1e-8
            if user_tol or stats['converged'] < 0 or not (stats['true_rel_residual'] <= 1e-8):
                raise SolverError('{}: Krylov solver did not converge in {} iterations (||r||/||b|| = {:.3e})'.format(
                    label, stats['iterations'], stats['true_rel_residual']))
            self.logger.warning('%s: stopped at ||r||/||b|| = %.3e after %d iterations (default tolerance %.0e not attained)',
                                label, stats['true_rel_residual'], stats['iterations'], rtol)
        per = u.function_space().periodic_pairs() if hasattr(u.function_space(), 'periodic_pairs') else None
        if per is not None:
            if loc is not None and hasattr(loc, 'tied_pairs'):      # decomposed: the local pairs (the slave rows live with their masters)
                per = loc.tied_pairs(per[0], per[1])
            x.assign_entries(per[0], per[1], block=u.function_space()._ncomp)
        if loc is None:
            u.vector()._adopt_device(x)         # stays in HBM; the host copy is fetched when somebody looks at it
        elif getattr(loc, 'is_local_view', False):
            # distributed mesh: the Function holds this rank's part, owned values and refreshed ghosts (what a DOLFIN
            # Function holds under MPI); parallel.gather_function(u) builds the global array when wanted
            from . import parallel
            if parallel.world()[1] > 1:
                backend.halo_exchange(V, x)
            if getattr(loc, 'is_identity', True):
                u.vector()._adopt_device(x)
            else:                                   # CG2 on a distributed mesh: device order -> the host's node order
                u.vector().set_local(loc.to_host(x.get()))
        else:   # every rank ends with the full field, gathered by global vertex id
            from . import parallel
            ncomp = u.function_space()._ncomp
            u.vector().set_local(parallel.gather_owned(x.get()[:V.n_owned], loc.owned_gids(), loc.n_global, ncomp))
        return u

    def _device_solve_vectors(self, A, b, x, label, amg=False, near_nullspace=None, operator_key=None):
        """A x = b with b and x DeviceVectors that stay on the device (one rank, a symmetric operator): CG + AMG (amg=True; the hierarchy
        is kept under operator_key as in _device_solve) or Jacobi-CG, with the tolerances of solver_parameters.  Returns the stats of
        the solve ('amg_reused' with a hierarchy); a solve that does not converge raises."""
        from . import backend
        rtol, max_iter, _ = self._krylov_options()
        sp_ = self.solver_settings.get('solver_parameters', {}) or {}
        norm = sp_.get('norm_type', 'preconditioned')
        if amg:
            hierarchy, reused = self._amg_hierarchy(A, operator_key, near_nullspace)
            stats = hierarchy.solve(b, x, rtol=rtol, max_iter=min(max_iter, int(sp_.get('maximum_iterations', 500))), norm=norm)
            stats['amg_reused'] = reused
            stats['amg_setup_ms'] = hierarchy.info()['setup_ms']
            if operator_key is None:
                hierarchy.close()
        else:
            stats = backend.krylov_solve(A, b, x, rtol=rtol, max_iter=max_iter, precond='jacobi', method='cg', norm=norm)
        self.last_solve_stats = stats
        if stats['converged'] != 1:
            user_tol = 'krylov_relative_tolerance' in sp_ or float(sp_.get('relative_tolerance', 1.0)) < 1e-8
            if user_tol or stats['converged'] < 0 or not (stats['true_rel_residual'] <= 1e-8):
                raise SolverError('{}: Krylov solver did not converge in {} iterations (||r||/||b|| = {:.3e})'.format(
                    label, stats['iterations'], stats['true_rel_residual']))
            self.logger.warning('%s: stopped at ||r||/||b|| = %.3e after %d iterations (default tolerance %.0e not attained)',
                                label, stats['true_rel_residual'], stats['iterations'], rtol)
        return stats

    def _amg_hierarchy(self, A, key, near_nullspace):
        """(hierarchy, reused): the smoothed-aggregation hierarchy of A, kept while the next caller names the same operator key;
        a caller with key None owns (and closes) the hierarchy it gets."""
        from . import backend
        sp_ = self.solver_settings.get('solver_parameters', {}) or {}
        cached = getattr(self, '_amg_cache', None)
        if key is not None and cached is not None and cached[0] == key:
            return cached[1], True
        if cached is not None:
            cached[1].close()
            self._amg_cache = None
        hierarchy = backend.AMG(A, nullspace=near_nullspace, strength_threshold=float(sp_.get('amg_strength_threshold', 0.0)))
        if key is not None:
            self._amg_cache = (key, hierarchy)
        return hierarchy, False

    def _replicated_amg_solve(self, b, x, V, loc, ncomp, global_operator, key, near_nullspace, rtol, max_iter, norm, theta, A_local=None):
        """solve_amg on several GPUs.  A hierarchy of the rank-local diagonal blocks (additive Schwarz) has no coarse space that
        couples the parts: on the cantilever of BASELINE configs[2] cut into 2 / 4 / 8 slabs across its length the 24
        iterations of one GPU become 166 / 321 / 495 (tools/amg_schwarz_probe.py).  What multigrid needs is the GLOBAL
        coarse problem, and a 5 M-DOF operator with its hierarchy is a few GB of the 288 GB every MI355X has: so every rank
        assembles the undecomposed operator as well (assembly is 2 ms, cheaper than any exchange of it), builds the same
        hierarchy, solves the gathered right-hand side and keeps its own entries - the iteration count of one GPU at any
        number of parts, no communication inside the solve, the speed of one GPU (not more: the preconditioner is not
        distributed; 'amg_decomposition': 'schwarz' selects the rank-local hierarchies).  The pressure Laplacian of the
        Navier-Stokes Schur complement is treated the same way (sd_precond, fs_saddle_solve.inc)."""
        from . import backend, parallel
        if getattr(self, '_amg_distributed_off', False):
            A_local = None                  # a distribution fault was seen on this solver earlier: replicated from then on
        cached = getattr(self, '_amg_cache', None)
        tag = 'replicated' if A_local is None else 'distributed'
        if key is not None and cached is not None and cached[0] == (tag, key):
            hierarchy, reused = cached[1], True
            if getattr(hierarchy, '_distributed', False) and hierarchy.A_local is not A_local:
                # same operator key, another matrix object: CG multiplies with the caller's CURRENT matrix
                hierarchy.attach_distributed_fine(A_local, loc.owned_gids())
        else:
            if cached is not None:
                cached[1].close()
                self._amg_cache = None
            Ag = global_operator()
            hierarchy, reused = backend.AMG(Ag, nullspace=near_nullspace, strength_threshold=theta), False
            hierarchy._distributed = False
            if A_local is not None and hierarchy.info()['levels'] >= 2:
                # the fine level on this rank's rows of the decomposed operator; levels >= 1 replicated (fs_amg_attach_distributed_fine)
                # (a problem so small that the hierarchy is one level is solved replicated, as in round 3)
                hierarchy.attach_distributed_fine(A_local, loc.owned_gids())
                hierarchy._distributed = True
            if key is not None:
                self._amg_cache = ((tag, key), hierarchy)
        if hierarchy._distributed:
            # CG on the decomposed operator (halo + reduced dots), one V-cycle per iteration whose fine level is distributed
            stats = hierarchy.solve(b, x, rtol=rtol, max_iter=max_iter, norm=norm)
            stats.update({'amg_' + k: v for k, v in hierarchy.info().items()})
            stats['amg_reused'], stats['amg_decomposition'] = reused, 'distributed'
            true_r, rec_r = stats.get('true_rel_residual', 0.0), stats.get('rel_residual', 0.0)
            faulty = not np.isfinite(true_r) or true_r > 100.0 * max(rec_r, rtol)
            if (stats['converged'] != 1 and stats['converged'] >= 0 and faulty) or (stats['converged'] == 1 and not np.isfinite(true_r)):
                # The distributed fine level has not run on more than one physical GPU yet.  EVIDENCE of a
                # distribution fault - the true residual b - A x far from the recurrence residual, or not a number (the status and
                # both residuals are the same on every rank: they come from reduced sums) - sends this solve and every later one
                # of this solver to the replicated hierarchy of round 3 (no communication inside the solve).  A solve that merely
                # stops at the user's maximum_iterations with consistent residuals is REPORTED as it is (the silent
                # second solve doubled the cost of a hard problem and hid it behind a warning).
                self.logger.warning('solve_amg: distributed fine level: true residual %.3g against recurrence residual %.3g after %d '
                                    'iterations; replicated hierarchy from now on', true_r, rec_r, stats['iterations'])
                self._amg_distributed_off = True
                hierarchy.close()
                self._amg_cache = None
                x.fill(0.0)
                return self._replicated_amg_solve(b, x, V, loc, ncomp, global_operator, key, near_nullspace, rtol, max_iter, norm, theta)
            if parallel.world()[1] > 1:
                backend.halo_exchange(V, x)
            if key is None:
                hierarchy.close()
            return stats
        Vg = hierarchy.A.space
        bg = parallel.gather_owned(b.get()[:V.n_owned], loc.owned_gids(), loc.n_global, ncomp)
        if bg.size != Vg.n_owned:
            raise SolverError('internal error: the undecomposed operator has {} rows, the gathered right-hand side {}'.format(Vg.n_owned, bg.size))
        bgd = backend.DeviceVector(Vg.n_owned, bg)
        xg = backend.DeviceVector(Vg.n_local)
        stats = hierarchy.solve(bgd, xg, rtol=rtol, max_iter=max_iter, norm=norm)
        stats.update({'amg_' + k: v for k, v in hierarchy.info().items()})
        stats['amg_reused'], stats['amg_decomposition'] = reused, 'replicated'
        xl = xg.get()[:Vg.n_owned].reshape(loc.n_global, ncomp)[np.asarray(loc.l2g)].reshape(-1)      # owned + ghost entries
        x.set(np.concatenate([xl, np.zeros(V.n_local - xl.size)]))
        if key is None:
            hierarchy.close()
        return stats

    @staticmethod
    def _bc_arrays(bcs):
        dofs = [bc.dofs for bc in bcs if isinstance(bc, DirichletBC)]
        vals = [bc.values for bc in bcs if isinstance(bc, DirichletBC)]
        if not dofs:
            return np.zeros(0, dtype=np.int32), np.zeros(0)
        return np.concatenate(dofs).astype(np.int32), np.concatenate(vals).astype(np.float64)

    def _facets_of(self, marker_id):
        sel = self.boundary_facets.where(marker_id)
        return self.mesh.facets()[sel]

    def _device_facets(self, F, marker_id, per_facet=None):
        """(vertex triples, per-facet values) of ds(marker_id) as this rank's device space needs them."""
        tri = self._facets_of(marker_id)
        loc = F.space.localizer()
        if loc is None:
            return tri, per_facet
        ltri, mask = loc.facets(tri)
        if per_facet is not None and np.ndim(per_facet) >= 1 and np.shape(per_facet)[0] == len(tri):
            per_facet = np.asarray(per_facet)[mask]
        return ltri, per_facet

    def assemble_system(self, F, bcs, symmetric=True, tie=True):
        """(A, b) on the device for a ScalarForm / ElasticityForm, Dirichlet conditions applied
        (dolfin.assemble_system / assemble + bc.apply; SolverBase.py:594-602, 644).  tie=False leaves a periodic
        constraint unfolded (the Newton loop adds its boundary terms first and folds then)."""
        from . import backend
        ip = getattr(F, 'ip_coefficient', 0.0)
        V = F.space.device(facet_coupling=True) if ip else F.space.device()
        loc = F.space.localizer()
        L_ = (lambda spec: spec) if loc is None else loc.spec
        A = backend.DeviceMatrix(V)
        b = backend.DeviceVector(V.n_owned)
        if isinstance(F, forms.ScalarForm):
            theta = F.theta if F.transient else 1.0
            mass = L_(F.capacity.spec(1.0 / F.dt)) if F.transient else None
            adv, adv_scale = F.advection if F.advection is not None else (None, 1.0)
            if adv is not None and loc is not None and np.ndim(adv) >= 2:
                adv = loc.cells(adv)
            pe = getattr(F, 'supg_pe', 0.0) if adv is not None else 0.0
            # Constant coefficients in a time loop: the unconstrained operators are the same every step - kept on the
            # device and copied (DOLFIN re-assembles them, SolverBase.py:592-602; the copy is a third of the assembly).
            const_ops = F.transient and adv is None and not ip and F.conductivity.kind == "const" and \
                F.capacity.kind == "const" and all(np.ndim(r.h) == 0 for r in F.robin)
            op_key = (V.serial, theta, float(F.conductivity.value), float(F.capacity.value), float(F.dt),
                      tuple((r.marker_id, float(r.h)) for r in F.robin)) if const_ops else None
            kept = self.__dict__.get('_kept_operators')
            if op_key is not None and kept is not None and kept[0] == op_key:
                A.copy_from(kept[1])
            else:
                A.assemble(stiffness=L_(F.conductivity.spec(theta)), mass=mass, advection=adv, advection_scale=adv_scale,
                           supg_pe=pe)
                if ip:          # fully implicit, like the advection term it stabilises (ScalarTransportSolver.py:305-315)
                    A.add_interior_penalty(self.mesh.interior_facet_cells()[0] if loc is None else loc.interior_facet_cells, ip)
                for r in F.robin:
                    tri, _ = self._device_facets(F, r.marker_id)
                    A.add_facet_mass(tri, r.h)
                kept = None
            first = True
            for s in F.sources:
                spec = L_(s.spec())
                backend.assemble_vector(V, b, source=spec, add=not first, supg=(adv, pe) if pe else None)
                first = False
            for fl in F.facet_loads:
                if np.ndim(fl.g) == 2:
                    # a varying flux by its vertex values: int g_h lambda_a ds = |F| / (d (d + 1)) (sum_b g_b + g_a), exact for
                    # the P1 interpolant (FFC: quadrature degree 2 for a degree-1 Expression times the test function)
                    gtri = self._facets_of(fl.marker_id).astype(np.int64)
                    loads = _facet_nodal_loads(self.mesh.coordinates(), gtri, np.asarray(fl.g, dtype=np.float64))
                    tri, loads = self._device_facets(F, fl.marker_id, loads)
                    rows = np.asarray(tri, dtype=np.int64)
                    own_rows = rows < V.n_owned
                    if own_rows.any():
                        b.add_entries(rows[own_rows], loads[own_rows])
                    continue
                tri, g = self._device_facets(F, fl.marker_id, fl.g)
                if len(tri):
                    backend.assemble_facet_vector(V, b, tri, g)
            for r in F.robin:
                if np.ndim(r.ambient) == 2:         # ambient given at the facet vertices: exact load of its P1 interpolant
                    gtri = self._facets_of(r.marker_id).astype(np.int64)
                    loads = _facet_nodal_loads(self.mesh.coordinates(), gtri, r.h * np.asarray(r.ambient, dtype=np.float64))
                    tri, loads = self._device_facets(F, r.marker_id, loads)
                    rows = np.asarray(tri, dtype=np.int64)
                    own_rows = rows < V.n_owned
                    if own_rows.any():
                        b.add_entries(rows[own_rows], loads[own_rows])
                    continue
                tri, amb = self._device_facets(F, r.marker_id, r.ambient if np.ndim(r.ambient) == 1 else None)
                if len(tri):
                    backend.assemble_facet_vector(V, b, tri, r.h * (amb if amb is not None else r.ambient))
            if pe:
                # the reference substitutes q + tau (v . grad q) in the boundary integrals as well (Tq, :296-298)
                def local_facets(marker_id, per_facet):
                    cells_, opp_, _ = self._marked_facet_cells(marker_id)
                    if loc is None:
                        return cells_, opp_, per_facet
                    # several GPUs: the facets whose cell is in this rank's part (rows of other ranks are skipped on the
                    # device); per-facet values follow the facets
                    g2l = self.__dict__.setdefault('_cell_g2l', {}).get(id(loc))
                    if g2l is None:
                        g2l = np.full(self.mesh.num_cells(), -1, dtype=np.int64)
                        g2l[loc.part.cell_gids] = np.arange(len(loc.part.cell_gids))
                        self._cell_g2l[id(loc)] = g2l
                    lc = g2l[cells_]
                    keep = lc >= 0
                    if per_facet is not None and np.ndim(per_facet) >= 1 and np.shape(per_facet)[0] == len(cells_):
                        per_facet = np.asarray(per_facet)[keep]
                    return lc[keep].astype(np.int32), opp_[keep], per_facet
                for fl in F.facet_loads:
                    cells_, opp_, gg = local_facets(fl.marker_id, fl.g if np.ndim(fl.g) < 2 else np.asarray(fl.g).mean(axis=1))
                    if len(cells_):
                        backend.assemble_facet_supg(V, None, b, cells_, opp_, adv, pe, g=gg)
                for r in F.robin:
                    amb = r.ambient if np.ndim(r.ambient) == 0 else (np.asarray(r.ambient).mean(axis=1) if np.ndim(r.ambient) == 2 else np.asarray(r.ambient))
                    cells_, opp_, amb_l = local_facets(r.marker_id, amb if np.ndim(amb) == 1 else None)
                    if len(cells_):
                        backend.assemble_facet_supg(V, A, b, cells_, opp_, adv, pe, g=r.h * (amb_l if amb_l is not None else amb), h=r.h)
            for ps in getattr(F, 'point_sources', []):
                # PointSource.apply(b) (SolverBase.py:597-601): before the Dirichlet rows, which then overwrite
                pd, pw = ps.dofs, ps.weights
                if loc is not None:
                    pd, pw = loc.dofs(pd, pw)
                    keep = pd < V.n_owned
                    pd, pw = pd[keep], pw[keep]
                if len(pd):
                    b.add_entries(pd, pw)
            if F.transient:
                # b += (M/dt - (1-theta) K) T_prev   (Crank-Nicolson old-step terms, :292-293)
                if kept is not None:
                    B = kept[2]
                else:
                    B = backend.DeviceMatrix(V)
                    B.assemble(stiffness=L_(F.conductivity.spec(-(1.0 - theta))), mass=L_(F.capacity.spec(1.0 / F.dt)),
                               advection=adv if pe else None, advection_scale=0.0, supg_pe=pe)    # SUPG mass part only
                    if op_key is not None:
                        Au = backend.DeviceMatrix(V)
                        Au.copy_from(A)              # A is still unconstrained here: the Dirichlet rows come last
                        old_kept = self.__dict__.get('_kept_operators')
                        if old_kept is not None:
                            old_kept[1].close()
                            old_kept[2].close()
                        self._kept_operators = (op_key, Au, B)
                if loc is None or getattr(loc, 'is_identity', False):
                    tp = F.T_prev.vector()._device(V.n_local)          # the previous solve left it in HBM
                else:
                    tp = backend.DeviceVector(V.n_local, solid_steps.to_device_dofs(V, loc, F.T_prev.vector()._values()))
                tmp = backend.DeviceVector(V.n_owned)
                B.spmv(tp, tmp)
                b.axpy(1.0, tmp)
        elif isinstance(F, forms.ElasticityForm):
            aniso = getattr(F, 'anisotropic', None)
            if aniso is not None:
                A.assemble_anisotropic(aniso.material(loc))     # (index and frames in device cell order: a file mesh on one GPU
                #                                                  may be uploaded in locality order, with a one-part localizer)
            else:
                lame = F.lame_spec()
                if F.cellwise() and loc is not None:
                    lame = ('cell', loc.cells(lame[1]))     # per-cell (mu, lambda): this rank's cells, in device cell order
                A.assemble(lame=lame)
            sgn = F.load_sign
            if F.body_force is not None:
                backend.assemble_vector(V, b, vector_value=[sgn * x for x in F.body_force])
            if getattr(F, 'body_force_nodal', None) is not None:
                Mb = backend.DeviceMatrix(V)
                Mb.assemble(lame=(0.0, 0.0), mass=1.0)
                fh = np.ascontiguousarray(F.body_force_nodal, dtype=np.float64).reshape(-1)
                fd = backend.DeviceVector(V.n_local, solid_steps.to_device_dofs(V, loc, fh))
                tmpb = backend.DeviceVector(V.n_owned)
                Mb.spmv(fd, tmpb)
                b.axpy(sgn, tmpb)
            for t in F.tractions:
                if isinstance(t, forms.NodalLoad):          # worked out per node on the host (sign included)
                    nd_, nv_ = np.asarray(t.dofs).ravel(), np.asarray(t.values, dtype=np.float64).ravel()
                    if loc is not None:                     # several GPUs: this rank's rows of the load
                        nd_, nv_ = loc.dofs(nd_, nv_)
                        keep_ = nd_ < V.n_owned
                        nd_, nv_ = nd_[keep_], nv_[keep_]
                    if len(nd_):
                        b.add_entries(nd_, nv_)
                    continue
                tri, g = self._device_facets(F, t.marker_id, t.g)
                if len(tri):
                    backend.assemble_facet_vector(V, b, tri, sgn * np.asarray(g, float))
            if F.thermal is not None:
                coef, T, T_ref = F.thermal
                if np.ndim(coef) > 0:
                    # per-cell E alpha / (1 - 2 nu): a per-cell coefficient, a nodal temperature by its mean at the cell's vertices
                    dT = float(T) - T_ref if np.ndim(T) == 0 else \
                        np.asarray(T, dtype=np.float64)[self.mesh.cells().astype(np.int64)].mean(axis=1) - T_ref
                    backend.assemble_vector(V, b, div_coef=L_(('cell', np.asarray(coef, dtype=np.float64) * dT)), add=True)
                elif np.ndim(T) == 0:
                    backend.assemble_vector(V, b, div_coef=coef * (float(T) - T_ref), add=True)
                else:
                    Tn = np.asarray(T)               # P1 temperature: its vertex values
                    if F.space.degree() == 2:        # nodal array over the P2 nodes; the kernel reads the vertex entries
                        Tn = np.concatenate([Tn, np.full(F.space.num_nodes() - len(Tn), T_ref)])
                    Tn = Tn if loc is None else loc.nodes(Tn)
                    backend.assemble_vector(V, b, div_coef=("nodal", coef * (Tn - T_ref)), add=True)
            if aniso is not None and aniso.thermal is not None:
                # int (C : eps*) : grad v dx with eps* = R alpha R^T (T_cell - T_ref), a nodal T by its mean at the cell's vertices
                backend.assemble_anisotropic_load(V, aniso.material(loc), aniso.eigenstrain(self.mesh.cells(), loc), b, add=True)
            if getattr(F, 'inertia', None) is not None:
                # F -= rho inner(accel, v) dx with the known (explicit) acceleration: rhs += rho M accel
                rho, accel = F.inertia
                Mv = backend.DeviceMatrix(V)
                Mv.assemble(lame=(0.0, 0.0), mass=L_(rho))
                ad = backend.DeviceVector(V.n_local, solid_steps.to_device_dofs(V, loc, accel.vector()._values()))
                tmp = backend.DeviceVector(V.n_owned)
                Mv.spmv(ad, tmp)
                b.axpy(1.0, tmp)
        else:
            raise SolverError('unknown form specification {}'.format(type(F)))
        per = F.space.periodic_pairs() if hasattr(F.space, 'periodic_pairs') else None
        if per is not None and tie:
            if loc is not None and hasattr(loc, 'tied_pairs'):
                per = loc.tied_pairs(per[0], per[1])
            A.tie_nodes(b, per[0], per[1])          # before the Dirichlet rows, as DOLFIN's dofmap has no slave dofs at all
        dofs, vals = self._bc_arrays(bcs)
        if loc is not None and dofs.size:
            dofs, vals = loc.dofs(dofs, vals)       # local dofs, ghosts included (their columns are eliminated too)
        if dofs.size:
            A.apply_dirichlet(b, dofs, vals, symmetric=symmetric)
        return A, b

    def solve_linear_problem(self, F, u, Dirichlet_bcs):
        """LinearVariationalSolver.solve() on the GPU (SolverBase.py:592-613)."""
        if isinstance(F, forms.NavierStokesForm):
            return self._navier_stokes_linear(F, u, Dirichlet_bcs)
        A, b = self.assemble_system(F, Dirichlet_bcs, symmetric=True)
        # advection makes the operator non-symmetric: BiCGStab (PETSc KSPBCGS) instead of CG
        method = "cg" if getattr(F, "symmetric", True) else "bicgstab"
        return self._device_solve(A, b, u, 'solve_linear_problem', method=method)

    def _newton_settings(self):
        """solver_parameters['newton_solver'] with DOLFIN's NewtonSolver defaults, and solver_parameters['monitor_convergence']"""
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        newton = sp.get('newton_solver', {}) if isinstance(sp.get('newton_solver', {}), dict) else {}
        return solid_steps.NewtonSettings(float(newton.get('relative_tolerance', 1e-9)), float(newton.get('absolute_tolerance', 1e-10)),
                                          int(newton.get('maximum_iterations', 50)), float(newton.get('relaxation_parameter', 1.0)),
                                          sp.get('monitor_convergence'))

    def solve_nonlinear_problem(self, F, u_current, Dirichlet_bcs, J):
        """NonlinearVariationalSolver.solve() (SolverBase.py:615-626): Newton iteration with DOLFIN's
        NewtonSolver defaults (relative 1e-9 / absolute 1e-10 on the residual norm, 50 iterations, no
        relaxation).  Every linear step is assembled and solved on the GPU.  The radiation term enters the residual
        exactly (degree-5 facet quadrature of m T_h^4 q) and the Jacobian by its facet-mean linearisation; a temperature-dependent conductivity is
        re-evaluated each iteration and its derivative left out of the Jacobian (quasi-Newton), as the
        reference's own remark at ScalarTransportSolver.py:281-283 does."""
        from . import backend
        if isinstance(F, forms.NavierStokesForm):
            return self._navier_stokes_newton(F, u_current, Dirichlet_bcs)
        if isinstance(F, forms.HyperelasticForm):
            return solid_steps.hyperelastic_newton(self, F, u_current, Dirichlet_bcs)
        if isinstance(F, forms.PlasticForm):
            return solid_steps.plastic_newton(self, F, u_current, Dirichlet_bcs)
        if not isinstance(F, forms.ScalarForm):
            raise SolverError('nonlinear solves are built for scalar transport and Navier-Stokes only')
        per = F.space.periodic_pairs()
        from . import parallel
        rtol, atol, max_it, _, monitor = self._newton_settings()
        V = F.space.device()
        loc = F.space.localizer()          # several GPUs: the iterate stays global on the host, rows are local
        n = V.n_owned
        gdofs, gvals = self._bc_arrays(Dirichlet_bcs)
        T = u_current.vector()._values().copy()
        if gdofs.size:
            T[gdofs] = gvals                                # the first iterate carries the boundary values
        if per is not None:
            T[per[0]] = T[per[1]]                           # ... and is periodic
        # (several GPUs: the iterate above is the global host array; the device works on this rank's pairs)
        per_dev = per if per is None or loc is None or not hasattr(loc, 'tied_pairs') else loc.tied_pairs(per[0], per[1])
        dofs = gdofs if loc is None else loc.dofs(gdofs, gvals)[0]
        own = dofs[dofs < n]
        ext = self.mesh.facets()[self.mesh.exterior_facets()]
        if loc is None:
            ext_dev, ext_mask = ext, slice(None)
        else:
            ext_dev, ext_mask = loc.facets(ext)
        krtol, kmax, pc = self._krylov_options()
        if pc not in ('jacobi', 'none', None):
            # 'amg' / 'petsc_amg' / 'hypre_amg' are accepted by _krylov_options; the Newton steps solve with Jacobi-CG
            self.logger.warning("solve_nonlinear_problem: preconditioner '%s' is not built for the Newton steps; using Jacobi", pc)
            pc = 'jacobi'
        r0 = None
        self.newton_iterations = 0
        for it in range(max_it + 1):
            u_current.vector().set_local(T)
            if hasattr(self, 'refresh_nonlinear_form'):
                self.refresh_nonlinear_form(F, u_current)
            A, b = self.assemble_system(F, [], symmetric=True, tie=False)   # operator and loads at the iterate, no BCs
            if F.radiation is not None:
                m_, T_amb = F.radiation
                Tf = T[ext.astype(np.int64)].mean(axis=1)
                # residual: int m (T_amb^4 - T_h^4) q ds with T_h the P1 iterate, integrated exactly (degree 5) as FFC does
                # for m*(pow(T, 4) - pow(T_amb, 4))*Tq*ds (ScalarTransportSolver.py:186-190); the Jacobian below keeps the
                # facet-mean linearisation - it only steers the iteration
                if F.space.degree() == 2:
                    ftab = F.space.facet_node_table(ext.astype(np.int64))
                    loads = _radiation_loads_p2(self.mesh.coordinates(), ext.astype(np.int64), ftab, T, m_, T_amb)
                    if loc is None:
                        b.add_entries(ftab, loads)
                    else:                                   # several GPUs: this rank's rows of the facet loads
                        rd_, rv_ = loc.dofs(np.asarray(ftab).ravel(), np.asarray(loads, dtype=np.float64).ravel())
                        keep_ = rd_ < n
                        if keep_.any():
                            b.add_entries(rd_[keep_], rv_[keep_])
                    en = T[ftab[:, ext.shape[1]:]]                          # edge-node values: the facet mean of a P2 field
                    Tf = en.mean(axis=1) if ext.shape[1] == 3 else (T[ftab[:, 0]] + 4.0 * en[:, 0] + T[ftab[:, 1]]) / 6.0
                else:
                    loads = _radiation_loads(self.mesh.coordinates(), ext.astype(np.int64), T, m_, T_amb)[ext_mask]
                    rows = np.asarray(ext_dev, dtype=np.int64)
                    own_rows = rows < n
                    b.add_entries(rows[own_rows], loads[own_rows])
            Tdev = backend.DeviceVector(V.n_local, T if loc is None else loc.nodes(T))
            r = backend.DeviceVector(n)
            A.spmv(Tdev, r)
            r.axpy(-1.0, b)                                         # r = A(T) T - b(T)
            if per is not None:
                # periodic constraint: Jacobian and residual are folded onto the masters together (A <- P^T A P + unit
                # slave rows, r <- P^T r with zeros on the slaves), so the Jacobian's boundary term goes in first
                if F.radiation is not None:
                    A.add_facet_mass(ext_dev, (4.0 * m_ * Tf ** 3)[ext_mask])
                A.tie_nodes(r, per_dev[0], per_dev[1])
            if own.size:
                backend.set_dirichlet_values(r, own, 0.0)           # residual of constrained rows is zero
            rn2 = float(r.dot(r))
            if loc is not None and parallel.world()[1] > 1:
                rn2 = float(backend.comm_allreduce_sum([rn2])[0])
            rnorm = float(np.sqrt(rn2))
            if r0 is None:
                r0 = rnorm
            if monitor:
                self.logger.info("Newton iteration %d: r (abs) = %.3e (tol = %.3e) r (rel) = %.3e (tol = %.3e)",
                                 it, rnorm, atol, rnorm / r0 if r0 > 0 else 0.0, rtol)
            if rnorm < atol or (r0 > 0 and rnorm / r0 < rtol):
                break
            if it == max_it:
                raise SolverError('Newton solver did not converge in {} iterations (residual {:.3e})'.format(max_it, rnorm))
            if F.radiation is not None and per is None:
                A.add_facet_mass(ext_dev, (4.0 * m_ * Tf ** 3)[ext_mask])   # d/dT of  + m T^4 q ds
            rhs = backend.DeviceVector(n)
            rhs.axpy(-1.0, r)
            if dofs.size:
                A.apply_dirichlet(rhs, dofs, 0.0, symmetric=True)   # delta = 0 on the Dirichlet boundary
            delta = backend.DeviceVector(V.n_local)
            kmethod = self._krylov_method("cg" if F.symmetric else "bicgstab")
            stats = backend.krylov_solve(A, rhs, delta, rtol=min(krtol, 1e-10), max_iter=kmax, precond=pc, method=kmethod,
                                         norm="preconditioned" if (kmethod == "cg" and pc == "jacobi") else "unpreconditioned")
            self.last_solve_stats = stats
            if stats['converged'] != 1:
                raise SolverError('Newton step {}: Krylov solver did not converge'.format(it))
            if per is not None:
                delta.assign_entries(per_dev[0], per_dev[1])        # the slaves move with their masters
            d = delta.get()[:n]
            if loc is not None:
                d = parallel.gather_owned(d, loc.owned_gids(), loc.n_global, 1)
            T = T + d
            self.newton_iterations = it + 1
        u_current.vector().set_local(T)
        return u_current

    # ---- Taylor-Hood Navier-Stokes (CoupledNavierStokesSolver) -----------------------------------------
    def _navier_stokes_context(self, F, bcs):
        """Device objects shared by the steps of one solve: mixed space, pressure operators, BC lists (local
        numbering of this rank's part on several GPUs)."""
        from . import backend
        W = F.space
        V = W.device()
        loc = W.localizer()
        dofs, vals = self._bc_arrays(bcs)                      # global dofs (a distributed mesh: this rank's host numbering)
        pre = dofs[(dofs % 4) == 3] if dofs.size else dofs
        ctx = getattr(self, '_ns_ctx', None)
        key = (V.serial, pre.size, np.sort(pre).tobytes())
        if ctx is None or ctx['key'] != key:
            from . import parallel
            Qs = W.pressure_space()
            Q = Qs.device()
            qloc = Qs.localizer()
            pinned = (pre // 4).astype(np.int64)
            local_view = getattr(loc, 'is_local_view', False)
            # distributed mesh: the host lists name this rank's vertices only - whether ANY pressure condition exists, and the
            # global vertices it names, are agreed over the ranks (every rank builds the same global pressure hierarchy below)
            gpre = None
            if local_view:
                own = pinned < qloc.n_owned
                gpre = np.concatenate(parallel.allgather_index_lists(np.asarray(qloc.l2g)[pinned[own]])) if parallel.world()[1] > 1 \
                    else np.asarray(qloc.l2g)[pinned[own]]
            n_pre_global = pre.size if gpre is None else gpre.size
            per = W.periodic_pairs()                 # (slave, master) P2 nodes of a periodic_boundary, or None
            qper = Qs.periodic_pairs()
            pin_vertex = 0
            if qper is not None and 0 in set(qper[0].tolist()):
                pin_vertex = int(qper[1][list(qper[0]).index(0)])      # a slave has no equation of its own: pin its master
            pin_local = pin_vertex           # host vertex that carries the pin (None: the pinned vertex is not on this rank)
            if n_pre_global == 0:
                # no pressure condition: the pressure is defined up to a constant (the reference's LU hits a
                # singular matrix here); fix it at vertex 0
                self.logger.warning('no pressure boundary condition: pinning the pressure at vertex %d to 0', pin_vertex)
                if local_view:                # global vertex 0: on the rank(s) whose slab holds it, owned or ghost
                    hit = np.nonzero(np.asarray(qloc.l2g) == pin_vertex)[0]
                    pin_local = int(hit[0]) if hit.size else None
                pinned = np.full(1, pin_local, dtype=np.int64) if pin_local is not None else np.zeros(0, dtype=np.int64)
            if qloc is not None:
                pinned = qloc.dofs(pinned, np.zeros(len(pinned)))[0]
            pinned = np.asarray(pinned, dtype=np.int32)
            Kp = backend.DeviceMatrix(Q)
            Kp.assemble(stiffness=1.0)
            if qper is not None:
                Kp.tie_nodes(None, qper[0], qper[1])
            Kp.apply_dirichlet(None, pinned, np.zeros(len(pinned)), symmetric=True)
            Mp = backend.DeviceMatrix(Q)
            Mp.assemble(mass=1.0)
            if qper is not None:
                Mp.tie_nodes(None, qper[0], qper[1])
            cell_g2l = None
            if loc is not None:
                cell_g2l = np.full(self.mesh.num_cells(), -1, dtype=np.int64)
                cell_g2l[loc.part.cell_gids] = np.arange(len(loc.part.cell_gids))
            # several GPUs: the pressure space is small, so every rank holds the hierarchy of the GLOBAL pressure
            # Laplacian (assembled on the global mesh) and the Schur-complement solve is replicated (sd_precond, fs_saddle_solve.inc)
            if loc is not None:
                if getattr(self.mesh, '_slab', None) is not None:      # distributed box: the device generates the whole box
                    nx_, ny_, nz_, p0_, p1_ = self.mesh._box
                    gm = backend.DeviceMesh.box(nx_, ny_, nz_, p0_, p1_)
                else:
                    gm = backend.DeviceMesh(self.mesh.coordinates(), self.mesh.cells())
                gQ = backend.DeviceSpace(gm, 1, 1)
                gK = backend.DeviceMatrix(gQ)
                gK.assemble(stiffness=1.0)
                if gpre is not None:
                    gpin = np.unique(gpre).astype(np.int32) if gpre.size else np.full(1, pin_vertex, dtype=np.int32)
                else:
                    gpin = (pre // 4).astype(np.int32) if pre.size else np.zeros(1, dtype=np.int32)
                gK.apply_dirichlet(None, gpin, np.zeros(len(gpin)), symmetric=True)
                kp_amg = backend.AMG(gK)
                keep = (gm, gQ, gK)
            else:
                kp_amg, keep = backend.AMG(Kp), None
            ctx = {'key': key, 'Kp': Kp, 'Mp': Mp, 'J': backend.DeviceMatrix(V), 'pinned': pinned,
                   'auto_pin': n_pre_global == 0 and pin_local is not None, 'Kp_amg': kp_amg, 'cell_g2l': cell_g2l, 'global_pressure': keep,
                   'per': per, 'pin_dof': 4 * (pin_local if pin_local is not None else 0) + 3,
                   'slave_dofs': None if per is None else (per[0].astype(np.int64)[:, None] * 4 + np.arange(4)).ravel().astype(np.int32)}
            self._ns_ctx = ctx
        if ctx['auto_pin']:
            dofs = np.concatenate([dofs, np.array([ctx['pin_dof']], dtype=np.int32)]).astype(np.int32)
            vals = np.concatenate([vals, np.zeros(1)])
        if loc is not None:
            dofs, vals = loc.dofs(dofs, vals)
        # "later wins" de-duplication happens on the device; dummy pressure slots stay at zero
        return V, ctx, dofs.astype(np.int32), vals, loc

    @staticmethod
    def _ns_local(loc, w):
        """global dof vector -> this rank's owned + ghost entries"""
        return w if loc is None else loc.nodes(w)

    def _navier_stokes_assemble(self, F, V, ctx, w, newton, loc=None, w_is_local=False, prev=None):
        """(device iterate, right-hand side) with ctx['J'] assembled at w: w a host array (global, or this rank's entries
        with w_is_local) or a DeviceVector that is used as it is; prev: the previous time step already on the device."""
        from . import backend
        if isinstance(w, backend.DeviceVector):
            dw = w
        else:
            dw = backend.DeviceVector(V.n_local, w if w_is_local else self._ns_local(loc, w))
        dp = None
        if F.inv_dt:
            dp = prev if prev is not None else backend.DeviceVector(V.n_local, self._ns_local(loc, F.w_prev.vector()._values()))
        g = backend.DeviceVector(V.n_owned)
        backend.assemble_navier_stokes(ctx['J'], g, dw, dp, nu=F.nu, rho=F.rho, inv_dt=F.inv_dt,
                                       body_force=F.body_force if F.body_force is not None else (0.0, 0.0, 0.0),
                                       convection=True, newton=newton,
                                       mesh_velocity=F.mesh_velocity if F.mesh_velocity is not None else (0.0, 0.0, 0.0),
                                       g2=getattr(F, 'g2', None), viscosity_law=getattr(F, 'viscosity_law', None))
        for marker_id, value in F.pressure_boundaries:
            cells, opp, centroids = self._marked_facet_cells(marker_id)
            if loc is not None:                 # facets whose cell is local; rows of other ranks are skipped on the device
                lc = ctx['cell_g2l'][cells]
                keep = lc >= 0
                cells, opp, centroids = lc[keep].astype(np.int32), opp[keep], centroids[keep]
            fv = None
            if value is not None:
                if is_constant_value(value):
                    fv = DirichletBC._eval(value, centroids, 1).reshape(-1)
                else:
                    # a boundary pressure that varies (e.g. hydrostatic): its values at the facet's vertices, in the cell's local
                    # order with the opposite vertex left out - DOLFIN's P1 interpolant of a degree-1 Expression
                    gcells = self.mesh.cells().astype(np.int64)
                    cg = cells if loc is None else loc.part.cell_gids[cells]
                    nvc = gcells.shape[1]                  # 4 (tetrahedra: facets are triangles) or 3 (triangles: edges)
                    keepv = np.arange(nvc)[None, :] != opp[:, None]
                    fverts = gcells[cg][keepv].reshape(-1, nvc - 1)
                    fv = DirichletBC._eval(value, self.mesh.coordinates()[fverts.ravel()], 1).reshape(-1, nvc - 1)
            backend.assemble_ns_pressure_boundary(ctx['J'], g, cells, opp, F.nu, fv, viscosity_law=getattr(F, 'viscosity_law', None), w0=dw)
        if ctx.get('per') is not None:
            # periodic_boundary: J <- P^T J P + unit slave rows, g <- P^T g (zeros on the slaves), all four unknowns of a node
            ctx['J'].tie_nodes(g, ctx['per'][0], ctx['per'][1])
        return dw, g

    def _marked_facet_cells(self, marker_id):
        """(cell, local opposite vertex, centroid) of the facets carrying a boundary marker."""
        cache = self.__dict__.setdefault('_facet_cell_cache', {})
        if marker_id not in cache:
            sel = self.boundary_facets.where(marker_id)
            cf = self.mesh.cell_facets()
            cells, opp = np.nonzero(np.isin(cf, sel))
            order = np.argsort(cf[cells, opp], kind='stable')       # ascending facet id: the order of _facets_of()
            cells, opp = cells[order], opp[order]
            tri = self.mesh.facets()[cf[cells, opp]].astype(np.int64)
            cache[marker_id] = (cells.astype(np.int32), opp.astype(np.int32), self.mesh.coordinates()[tri].mean(axis=1))
        return cache[marker_id]

    def _navier_stokes_krylov(self, F, ctx, J, b, x, rtol, nonzero_guess):
        from . import backend
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        st = backend.saddle_solve(J, ctx['Kp'] if F.inv_dt else None, ctx['Mp'], b, x, nu=F.nu, rho=F.rho,
                                  inv_dt=F.inv_dt, rtol=rtol, max_iter=int(sp.get('krylov_maximum_iterations', 2000)),
                                  restart=int(sp.get('gmres_restart', 0)),
                                  velocity_sweeps=int(sp.get('velocity_sweeps', 0 if F.inv_dt else 3)),
                                  nonzero_guess=nonzero_guess, Kp_amg=ctx['Kp_amg'] if F.inv_dt else None)
        self.last_solve_stats = st
        if st['converged'] != 1:
            raise SolverError('Navier-Stokes: FGMRES did not converge in {} iterations (||r||/||b|| = {:.3e})'.format(
                st['iterations'], st['rel_residual']))
        return st

    def _navier_stokes_newton(self, F, u_current, bcs):
        """NonlinearVariationalSolver.solve() for the coupled system: DOLFIN NewtonSolver defaults (relative 1e-9 /
        absolute 1e-10 on the residual 2-norm, 50 iterations, relaxation 1); each step solves J dw = -R on the GPU(s).
        On several GPUs every rank keeps the full iterate on the host (as every other path of this back end does),
        assembles and solves its own rows and the update is gathered by global dof."""
        from . import backend, parallel
        V, ctx, dofs, vals, loc = self._navier_stokes_context(F, bcs)
        gdofs, gvals = self._bc_arrays(bcs)
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        rtol, atol, max_it, relax, _ = self._newton_settings()
        lin_rtol = float(sp.get('krylov_relative_tolerance', 1e-6))
        adaptive = 'krylov_relative_tolerance' not in sp     # inexact Newton: see forcing() below
        w = u_current.vector().get_local()
        w[gdofs] = gvals
        if ctx['auto_pin']:
            w[ctx['pin_dof']] = 0.0
        w[F.space.dummy_dofs()] = 0.0
        per = ctx.get('per')
        if per is not None:
            w4 = w.reshape(-1, 4)
            w4[per[0]] = w4[per[1]]                # the iterate is periodic from the start
        own = dofs[dofs < V.n_owned]               # constrained rows of this rank (the list also names ghost dofs)
        if per is not None:
            own = np.unique(np.concatenate([own, ctx['slave_dofs']]))      # slave rows are unit rows: no residual there
        # several GPUs: the iterate lives in this rank's numbering (owned + ghost entries) during the iteration - the
        # update of the ghosts comes with the halo of the Krylov solution - and is gathered once at the end
        # the iterate, the residual and the update stay in HBM for the whole Newton iteration (one upload, one download)
        dw = backend.DeviceVector(V.n_local, self._ns_local(loc, w))
        dprev = backend.DeviceVector(V.n_local, self._ns_local(loc, F.w_prev.vector()._values())) if F.inv_dt else None
        zeros_own = np.zeros(len(own))
        history, krylov = [], 0
        timing = os.environ.get("FS_NS_TIMING") is not None
        tm = {"assemble": 0.0, "residual": 0.0, "dirichlet": 0.0, "krylov": 0.0, "update": 0.0}
        clock = time.perf_counter
        for it in range(max_it + 1):
            t0 = clock()
            dw, g = self._navier_stokes_assemble(F, V, ctx, dw, newton=True, loc=loc, prev=dprev)
            t1 = clock()
            r = backend.DeviceVector(V.n_owned)
            ctx['J'].spmv(dw, r)
            r.axpy(-1.0, g)                                   # R(w) = J w - g
            if len(own):
                backend.set_dirichlet_values(r, own, zeros_own)   # constrained rows carry no residual
            rn2 = float(r.dot(r))
            if loc is not None and parallel.world()[1] > 1:
                rn2 = float(backend.comm_allreduce_sum([rn2])[0])
            rn = float(np.sqrt(rn2))
            t2 = clock()
            tm["assemble"] += t1 - t0
            tm["residual"] += t2 - t1
            history.append(rn)
            self.logger.info("Newton iteration %d: r (abs) = %.3e (tol = %.3e) r (rel) = %.3e (tol = %.3e)", it, rn, atol,
                             rn / max(history[0], 1e-300), rtol)
            if rn <= atol or rn <= rtol * history[0]:
                break
            if it == max_it:
                raise SolverError('Newton solver did not converge in {} iterations: {}'.format(max_it, history))
            t3 = clock()
            rhs = backend.DeviceVector(V.n_owned)
            rhs.fill(0.0)
            rhs.axpy(-1.0, r)
            ctx['J'].apply_dirichlet(rhs, dofs, np.zeros(len(dofs)), symmetric=False)
            t4 = clock()
            x = backend.DeviceVector(V.n_local)
            eta = lin_rtol
            if adaptive:
                # Forcing term of the inexact Newton step (Eisenstat-Walker, choice 2, gamma 0.9 / alpha 2): the linear
                # solve need not be more accurate than the quadratic term of the step it serves; never looser than
                # 1e-3, never tighter than what would finish the iteration from here.  On the cavity of configs[4]
                # the first solve of a time step stops after ~25 instead of ~46 FGMRES iterations, the Newton history
                # is unchanged.
                target = max(atol, rtol * history[0])
                need = 0.3 * target / rn
                eta = 1e-3 if len(history) < 2 else 0.9 * (history[-1] / history[-2]) ** 2
                eta = min(max(eta, need, 1e-10), 1e-3)
            st = self._navier_stokes_krylov(F, ctx, ctx['J'], rhs, x, eta, False)
            krylov += st['iterations']
            t5 = clock()
            if loc is not None and parallel.world()[1] > 1:
                backend.halo_exchange(V, x)                   # ghost entries of the update
            if per is not None:
                x.assign_entries(per[0], per[1], block=4)     # the slaves move with their masters
            dw.axpy(relax, x)
            t6 = clock()
            tm["dirichlet"] += t4 - t3
            tm["krylov"] += t5 - t4
            tm["update"] += t6 - t5
        wl = dw.get()
        if loc is None:
            w = wl[:V.n_owned]
        elif getattr(loc, 'is_local_view', False):
            # distributed mesh: the Function keeps this rank's part - owned values and the ghosts the last halo refreshed - in
            # the host's node order (what a DOLFIN Function holds under MPI); parallel.gather_nodes(u) names the nodes globally
            w = loc.to_host(wl) if not getattr(loc, 'is_identity', True) else wl[:loc.n_local * 4]
        else:
            w = parallel.gather_owned(wl[:V.n_owned], loc.owned_gids(), loc.n_global, 4)
        if timing:
            self.logger.warning("Newton timing [s]: %s", {k: round(v, 4) for k, v in tm.items()})
        self.newton_history = history
        self.newton_krylov_iterations = krylov
        u_current.vector().set_local(w)
        return u_current

    def _navier_stokes_linear(self, F, u, bcs):
        """One Picard step: LinearVariationalSolver on lhs(F) == rhs(F) with the advecting velocity frozen."""
        from . import backend, parallel
        V, ctx, dofs, vals, loc = self._navier_stokes_context(F, bcs)
        gdofs, gvals = self._bc_arrays(bcs)
        sp = self.solver_settings.get('solver_parameters', {}) or {}
        w = F.w_current.vector().get_local()
        dw, g = self._navier_stokes_assemble(F, V, ctx, w, newton=False, loc=loc)
        ctx['J'].apply_dirichlet(g, dofs, vals, symmetric=False)
        w0 = w.copy()
        w0[gdofs] = gvals
        if ctx['auto_pin']:
            w0[ctx['pin_dof']] = 0.0
        per = ctx.get('per')
        if per is not None:
            w04 = w0.reshape(-1, 4)
            w04[per[0]] = 0.0                                  # slave rows are unit rows with a zero right-hand side
        x = backend.DeviceVector(V.n_local, self._ns_local(loc, w0))
        self._navier_stokes_krylov(F, ctx, ctx['J'], g, x, float(sp.get('krylov_relative_tolerance', 1e-8)), True)
        if per is not None:
            x.assign_entries(per[0], per[1], block=4)
        if loc is not None and getattr(loc, 'is_local_view', False):
            if parallel.world()[1] > 1:
                backend.halo_exchange(V, x)
            out = loc.to_host(x.get()) if not getattr(loc, 'is_identity', True) else x.get()[:loc.n_local * 4]
        else:
            out = x.get()[:V.n_owned]
            if loc is not None:
                out = parallel.gather_owned(out, loc.owned_gids(), loc.n_global, 4)
        out[F.space.dummy_dofs()] = 0.0
        u.vector().set_local(out)
        return u

    def solve_amg(self, F, u, bcs):
        """assemble_system + CG preconditioned by smoothed-aggregation AMG with the rigid-body near-null
        space (SolverBase.py:643-672); solver_parameters['preconditioner'] = 'jacobi' selects Jacobi-CG."""
        if isinstance(F, forms.ElasticityForm) and F.body_force is None and getattr(F, 'body_force_nodal', None) is None \
                and not F.tractions and F.thermal is None and getattr(getattr(F, 'anisotropic', None), 'thermal', None) is None \
                and not any(np.any(bc.values != 0) for bc in bcs):
            # empty right-hand side: the reference fails in assemble_system here (Appendix B-Q11)
            self.logger.warning('solve_amg: zero load and homogeneous BCs, the solution is zero')
        A, b = self.assemble_system(F, bcs, symmetric=True)
        key = self._amg_operator_key(F, bcs)
        # near-null space of the elasticity operator: the six rigid-body modes, built on the device from the node
        # coordinates (build_nullspace() below is the host version the reference's API exposes)
        ns = "rigid_body" if isinstance(F, forms.ElasticityForm) and self.dimension == 3 else None
        glob = (lambda: self._undecomposed_elasticity_operator(F, bcs)) if isinstance(F, forms.ElasticityForm) else None
        return self._device_solve(A, b, u, 'solve_amg', amg=True, near_nullspace=ns, operator_key=key, global_operator=glob)

    def _undecomposed_elasticity_operator(self, F, bcs):
        """The Dirichlet-eliminated elasticity operator of the WHOLE mesh on this rank's GPU (several ranks, replicated AMG)."""
        from . import backend, parallel
        W = F.space.root() if hasattr(F.space, 'root') else F.space
        mesh, loc, nc = W.mesh(), W.localizer(), W._ncomp
        if F.cellwise() and getattr(mesh, '_slab', None) is not None:
            raise SolverError("solve_amg: a per-cell material on BoxMesh(distributed=True) under several ranks needs the global "
                              "cell array, which no rank holds - use the replicated BoxMesh (distributed=False), or "
                              "solver_parameters {'preconditioner': 'jacobi'}")
        cache = mesh.__dict__.setdefault('_undecomposed_device', {})
        if 'mesh' not in cache:
            if getattr(mesh, '_slab', None) is not None:          # distributed box: the device generates the whole box
                nx, ny, nz, p0, p1 = mesh._box
                cache['mesh'] = backend.DeviceMesh.box(nx, ny, nz, p0, p1)
            else:
                cache['mesh'] = backend.DeviceMesh(mesh.coordinates(), mesh.cells())
        per = W.periodic_pairs() if hasattr(W, 'periodic_pairs') else None
        skey = ('space', nc, W.degree(), per is not None)
        if skey not in cache:
            # (a periodic space: the hierarchy is the FOLDED operator's - pattern with the master / neighbour-of-slave couplings)
            cache[skey] = backend.DeviceSpace(cache['mesh'], nc, W.degree(), coupled_pairs=None if per is None else W._periodic_couplings())
        Vg = cache[skey]
        Ag = backend.DeviceMatrix(Vg)
        Ag.assemble(lame=F.lame_spec())         # (the host mesh's global cells, which is the order this device mesh holds them in)
        if per is not None:
            Ag.tie_nodes(None, per[0], per[1])
        dofs, vals = self._bc_arrays(bcs)
        if getattr(loc, 'is_local_view', False):
            # the Dirichlet lists of a distributed mesh are local: owned entries -> global dofs, gathered over the ranks
            node, comp = dofs // nc, dofs % nc
            own = node < loc.n_owned
            gd = np.asarray(loc.l2g)[node[own]] * nc + comp[own]
            parts = parallel.allgather_index_lists(gd)
            vparts = parallel.allgather_values(vals[own])
            dofs, vals = np.concatenate(parts), np.concatenate(vparts)
        if dofs.size:
            Ag.apply_dirichlet(backend.DeviceVector(Vg.n_owned), dofs.astype(np.int32), vals, symmetric=True)
        return Ag

    def _amg_operator_key(self, F, bcs):
        """Everything the assembled matrix depends on, or None when that cannot be told cheaply (no hierarchy reuse)."""
        import zlib
        if not isinstance(F, forms.ElasticityForm):
            return None
        dofs = np.concatenate([np.asarray(bc.dofs, dtype=np.int64) for bc in bcs]) if bcs else np.zeros(0, dtype=np.int64)
        if getattr(F, 'anisotropic', None) is not None:     # a digest of table, index and frames
            return ('elasticity', F.space.root().serial(), 'anisotropic', F.anisotropic.digest(), len(dofs),
                    zlib.crc32(np.ascontiguousarray(dofs).tobytes()))
        if F.cellwise():        # per-cell material: a digest of the (mu, lambda) pairs
            pairs = np.ascontiguousarray(F.lame_spec()[1])
            return ('elasticity', F.space.root().serial(), 'cell', pairs.shape[0], zlib.crc32(pairs.tobytes()), len(dofs),
                    zlib.crc32(np.ascontiguousarray(dofs).tobytes()))
        return ('elasticity', F.space.root().serial(), float(F.mu), float(F.lmbda), len(dofs), zlib.crc32(np.ascontiguousarray(dofs).tobytes()))

    def build_nullspace(self, V, x=None):
        """The rigid-body modes of SolverBase.py:674-706 (3 in 2D, 6 in 3D), orthonormalised."""
        co = V.node_coordinates() if hasattr(V, 'node_coordinates') else V.mesh().coordinates()   # P2: edge mid-points too
        n = co.shape[0]
        if self.dimension == 2:
            ns = np.zeros((3, n, 2))
            ns[0, :, 0] = 1.0
            ns[1, :, 1] = 1.0
            ns[2, :, 0], ns[2, :, 1] = -co[:, 1], co[:, 0]
            basis = ns.reshape(3, 2 * n)
        else:
            ns = np.zeros((6, n, 3))
            ns[0, :, 0] = 1.0
            ns[1, :, 1] = 1.0
            ns[2, :, 2] = 1.0
            ns[3, :, 0], ns[3, :, 1] = -co[:, 1], co[:, 0]
            ns[4, :, 0], ns[4, :, 2] = co[:, 2], -co[:, 0]
            ns[5, :, 2], ns[5, :, 1] = co[:, 1], -co[:, 2]
            basis = ns.reshape(6, 3 * n)
        q, _ = np.linalg.qr(basis.T)
        return q.T.copy()


# degree-5 rules: Radon's 7 points on the triangle (barycentric), 3 Gauss points on the segment
_S15 = np.sqrt(15.0)
_TRI7 = np.array([[1 / 3, 1 / 3, 1 / 3]] +
                 [p for a in ((6 - _S15) / 21, (6 + _S15) / 21) for p in ([1 - 2 * a, a, a], [a, 1 - 2 * a, a], [a, a, 1 - 2 * a])])
_TRI7_W = np.array([9 / 40] + [(155 - _S15) / 1200] * 3 + [(155 + _S15) / 1200] * 3)
_SEG3 = np.array([[0.5 - 0.5 * np.sqrt(0.6), 0.5 + 0.5 * np.sqrt(0.6)], [0.5, 0.5], [0.5 + 0.5 * np.sqrt(0.6), 0.5 - 0.5 * np.sqrt(0.6)]])
_SEG3_W = np.array([5 / 18, 8 / 18, 5 / 18])


def _facet_nodal_loads(coords, facets, g):
    """[n_facets, d] vertex loads int_F g_h lambda_a ds for g given at the facet vertices (triangles or edges)."""
    X = coords[facets]
    d = facets.shape[1]
    if d == 3:
        e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        c = np.cross(e1, e2) if X.shape[2] == 3 else (e1[:, 0] * e2[:, 1] - e1[:, 1] * e2[:, 0])[:, None]
        measure = 0.5 * np.linalg.norm(np.atleast_2d(c), axis=1)
    else:
        measure = np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
    return (measure / (d * (d + 1.0)))[:, None] * (g.sum(axis=1, keepdims=True) + g)


def _p2_facet_shape(pts):
    """[nq, n] values of the P2 facet basis (vertices, then edges (0,1), (0,2), (1,2) - or the one mid-point) at barycentric pts."""
    d = pts.shape[1]
    cols = [pts[:, i] * (2.0 * pts[:, i] - 1.0) for i in range(d)]
    for a, b in (((0, 1), (0, 2), (1, 2)) if d == 3 else ((0, 1),)):
        cols.append(4.0 * pts[:, a] * pts[:, b])
    return np.stack(cols, axis=1)


def _radiation_loads_p2(coords, facets, node_table, T, m, T_amb):
    """[n_facets, n] loads int_F m (T_amb^4 - T_h^4) phi_a ds of a P2 field on boundary triangles / edges: degree-10
    integrand (FFC: 4 * 2 + 2), integrated with Gauss-Legendre points (collapsed onto the triangle)."""
    X = coords[facets]
    g, w = np.polynomial.legendre.leggauss(6)
    g, w = 0.5 * (g + 1.0), 0.5 * w
    if facets.shape[1] == 3:
        e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        measure = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
        # Duffy: (u, v) in the unit square -> lambda = (1 - u, u (1 - v), u v), weight u (times 2 for the unit-area normalisation)
        U, Vv = np.meshgrid(g, g, indexing="ij")
        WW = np.outer(w, w) * U * 2.0
        pts = np.stack([1.0 - U.ravel(), (U * (1.0 - Vv)).ravel(), (U * Vv).ravel()], axis=1)
        wq = WW.ravel()
    else:
        measure = np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
        pts, wq = np.stack([1.0 - g, g], axis=1), w
    phi = _p2_facet_shape(pts)                               # [nq, n]
    Tq = T[node_table] @ phi.T                               # [nf, nq]
    return measure[:, None] * ((m * (T_amb ** 4 - Tq ** 4) * wq[None, :]) @ phi)


def _radiation_loads(coords, facets, T, m, T_amb):
    """[n_facets, d] vertex loads  int_F m (T_amb^4 - T_h^4) lambda_a ds  of the P1 field T on boundary triangles (3-D) or
    edges (2-D): quintic integrand, integrated exactly."""
    X = coords[facets]
    if facets.shape[1] == 3:
        e1, e2 = X[:, 1] - X[:, 0], X[:, 2] - X[:, 0]
        measure = 0.5 * np.linalg.norm(np.cross(e1, e2), axis=1)
        pts, w = _TRI7, _TRI7_W
    else:
        measure = np.linalg.norm(X[:, 1] - X[:, 0], axis=1)
        pts, w = _SEG3, _SEG3_W
    Tq = T[facets] @ pts.T                                   # [nf, nq]
    g = m * (T_amb ** 4 - Tq ** 4) * w[None, :]              # [nf, nq]
    return measure[:, None] * (g @ pts)                      # [nf, d]


def write_vtu(path, mesh, function, name, extra=()):
    """ASCII VTK unstructured grid of a nodal function on a tet mesh (vertex values); extra: [(Function, name)]."""
    co, ce = mesh.coordinates(), mesh.cells()
    if co.shape[1] == 2:          # VTK points are 3-D
        co = np.concatenate([co, np.zeros((len(co), 1))], axis=1)
    nvc = ce.shape[1]             # 4: tetra (VTK type 10), 3: triangle (type 5)
    vals = function.vertex_values()
    ncomp = 1 if vals.ndim == 1 else vals.shape[1]
    with open(path, "w") as fh:
        fh.write('<?xml version="1.0"?>\n<VTKFile type="UnstructuredGrid" version="0.1" byte_order="LittleEndian">\n')
        fh.write('<UnstructuredGrid>\n<Piece NumberOfPoints="%d" NumberOfCells="%d">\n' % (len(co), len(ce)))
        fh.write('<Points>\n<DataArray type="Float64" NumberOfComponents="3" format="ascii">\n')
        np.savetxt(fh, co, fmt="%.16e")
        fh.write('</DataArray>\n</Points>\n<Cells>\n<DataArray type="Int32" Name="connectivity" format="ascii">\n')
        np.savetxt(fh, ce, fmt="%d")
        fh.write('</DataArray>\n<DataArray type="Int32" Name="offsets" format="ascii">\n')
        np.savetxt(fh, (np.arange(len(ce)) + 1) * nvc, fmt="%d")
        fh.write('</DataArray>\n<DataArray type="UInt8" Name="types" format="ascii">\n')
        np.savetxt(fh, np.full(len(ce), 10 if nvc == 4 else 5), fmt="%d")
        fh.write('</DataArray>\n</Cells>\n')
        fh.write('<PointData %s="%s">\n' % ("Scalars" if ncomp == 1 else "Vectors", name))
        fh.write('<DataArray type="Float64" Name="%s" NumberOfComponents="%d" format="ascii">\n' % (name, ncomp))
        np.savetxt(fh, vals.reshape(len(co), -1), fmt="%.16e")
        fh.write('</DataArray>\n')
        for f2, n2 in extra:
            v2 = f2.vertex_values()
            fh.write('<DataArray type="Float64" Name="%s" NumberOfComponents="%d" format="ascii">\n' % (
                n2, 1 if v2.ndim == 1 else v2.shape[1]))
            np.savetxt(fh, v2.reshape(len(co), -1), fmt="%.16e")
            fh.write('</DataArray>\n')
        fh.write('</PointData>\n</Piece>\n</UnstructuredGrid>\n</VTKFile>\n')
