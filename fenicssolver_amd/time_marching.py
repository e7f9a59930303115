"""Host pieces the explicit time marchers share (WaveSolver, ElastodynamicsSolver with 'scheme': 'explicit'): the two bounds on the
time step of a central-difference march with the operator K and the lumped mass m, the check of a step against them, and the end of a
batch of device steps."""

from __future__ import annotations

import math

import numpy as np

from .fem import SolverError

POWER_ITERATIONS = 40


def power_iteration(K, m, bc_dofs, who):
    """Rayleigh quotient x^T K x / x^T diag(m) x after POWER_ITERATIONS steps of x <- diag(1/m) K x on the rows that are not Dirichlet: a
    lower bound on the largest eigenvalue of the operator the march sees.  The products run on the device.  who: the solver the
    error names."""
    from . import backend
    n = len(m)
    free = np.ones(n)
    free[np.asarray(bc_dofs, dtype=np.int64)] = 0.0
    x = np.random.default_rng(2024).standard_normal(n) * free
    xd, yd = backend.DeviceVector(n), backend.DeviceVector(n)
    lam = 0.0
    for _ in range(POWER_ITERATIONS):
        x /= math.sqrt(float(x @ (m * x)))
        xd.set(x)
        K.spmv(xd, yd)
        lam = xd.dot(yd)                    # x^T K x with x^T diag(m) x = 1
        x = free * yd.get() / m
    xd.close()
    yd.close()
    if not (lam > 0.0 and np.isfinite(lam)):
        raise SolverError('{}: the power iteration gave lambda_P = {}'.format(who, lam))
    return lam


def step_bounds(solver, K, m, bc_dofs):
    """(2 / sqrt(lambda_G), 2 / sqrt(lambda_P)): the march is stable below the first and certain to blow up above the second.
    lambda_G = max_i sum_j |K_ij| / m_i (Gershgorin, an upper bound on the largest eigenvalue), lambda_P = the solver's
    _power_iteration (a lower bound)."""
    rp, ci, va, _ = K.to_csr()
    lam_g = float(np.max(np.add.reduceat(np.abs(va), rp[:-1].astype(np.int64)) / m))
    lam_p = solver._power_iteration(K, m, bc_dofs)
    return 2.0 / math.sqrt(lam_g), 2.0 / math.sqrt(lam_p)


def check_step(who, dt, bounds, logger, march='the march'):
    """a step above the second bound of step_bounds is refused, one between the two is logged.  who: the solver the messages name;
    march: what the refusal calls the march"""
    if dt > bounds[1]:
        raise SolverError('{}: time_step {:.6g} exceeds 2/sqrt(lambda_P) = {:.6g} (power iteration, a lower bound on the largest '
                          'eigenvalue): {} is certain to blow up; the stable bound 2/sqrt(lambda_G) is {:.6g}'.format(
                              who, dt, bounds[1], march, bounds[0]))
    if dt > bounds[0]:
        logger.warning('%s: time_step %.6g lies between the stable bound 2/sqrt(lambda_G) = %.6g and 2/sqrt(lambda_P) = %.6g', who, dt,
                       bounds[0], bounds[1])


def batch_end(n, N, freqs, batch_steps):
    """the step at which the batch that starts at step n of N ends: the next multiple of each positive frequency, at most batch_steps
    (None: no cap) steps away"""
    end = N
    for freq in freqs:
        if freq and freq > 0:
            end = min(end, (n // int(freq) + 1) * int(freq))
    return end if batch_steps is None else min(end, n + batch_steps)
