"""Results derived from a per-cell stress that a solver class stores itself (PlasticitySolver, ViscoelasticitySolver)."""
from __future__ import annotations

import numpy as np

from .fem import Function
from .SolverBase import SolverError


class StoredStressVonMises:
    """von Mises value of a per-cell stress the solver STORES (``self.stress()``: [n_cells, 6] or, in plane strain, [n_cells, 4]) and
    its CG1 projection - for solver classes whose stress is not C : eps(u) (PlasticitySolver, ViscoelasticitySolver).  Listed before
    LinearElasticitySolver among the bases, so that it replaces the inherited von_Mises()."""

    def von_Mises_cells(self, stress=None):
        """sqrt(3/2) |dev sigma| per cell of ``stress`` (default: the stored stress)"""
        s = self.stress() if stress is None else stress
        m = s[:, :3].mean(axis=1)
        dev2 = ((s[:, :3] - m[:, None]) ** 2).sum(axis=1) + 2.0 * (s[:, 3:] ** 2).sum(axis=1)
        return np.sqrt(1.5 * dev2)

    def von_Mises(self, u=None):
        """The consistent L2 projection onto CG1 of the von Mises value of the RETURNED stress (the inherited method would project
        the elastic stress of u, which is wrong once a cell has yielded): right-hand side int vm phi_a dx with the per-cell value,
        P1 mass matrix, Jacobi-CG to 1e-12 on the device.  ``u`` is accepted for the inherited signature and not used."""
        return self._project_cells(self.von_Mises_cells())

    def _project_cells(self, vm):
        """The consistent L2 projection onto CG1 of one value per cell (host cell order)."""
        from .fem import FunctionSpace
        from . import backend
        P = FunctionSpace(self.mesh, 'P', 1)
        dP = P.device()
        ploc = P.localizer()
        b = backend.DeviceVector(dP.n_owned)
        backend.assemble_vector(dP, b, source=('cell', vm if ploc is None else ploc.cells(vm)))
        M = backend.DeviceMatrix(dP)
        M.assemble(mass=1.0)
        x = backend.DeviceVector(dP.n_local)
        st = backend.krylov_solve(M, b, x, rtol=1e-12, max_iter=2000, precond="jacobi", norm="preconditioned")
        if st['converged'] != 1:
            raise SolverError('von_Mises: the mass-matrix solve did not converge')
        f = Function(P)
        xh = x.get()[:dP.n_owned]
        if ploc is not None:
            from . import parallel
            xh = parallel.gather_owned(xh, ploc.owned_gids(), ploc.n_global, 1)
        f.vector().set_local(xh)
        return f
