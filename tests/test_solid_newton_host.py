"""solid_steps.damped_newton on the host (no GPU, no back end): the loop that decides about convergence, halving and the commit of a
history, driven with numpy callables on r(x) = A x + c x^3 - b (A SPD, three unknowns, the exact Jacobian).  Every case counts the
calls of evaluate and solve_step: one evaluation of the first iterate and one per trial is all the device work a solve may do."""
import numpy as np
import pytest

from fenicssolver_amd.fem import SolverError
from fenicssolver_amd.solid_steps import damped_newton, NewtonSettings, HYPERELASTIC_TEXTS, PLASTIC_TEXTS

A = np.array([[4.0, 1.0, 0.0], [1.0, 3.0, 0.5], [0.0, 0.5, 2.0]])
HYPER_HINT = ('apply the load in steps: transient_settings with boundary values and loads that change from step to step '
              '(a per-step sequence or a callable of time - constant values repeat the full load at every step)')
PLASTIC_HINT = ('apply the load in smaller steps (transient_settings with boundary values and loads that change from step to '
                'step), or give the material a hardening_modulus > 0')
INFO = {'n_inverted': 0, 'first_inverted_cell': -1, 'n_nonfinite': 0, 'n_yielded': 5}
BAD = {'n_inverted': 2, 'first_inverted_cell': 7, 'n_nonfinite': 1, 'n_yielded': 0}


class Log:
    def __init__(self):
        self.lines = []

    def info(self, fmt, *args):
        self.lines.append(fmt % args)


class Problem:
    """r(x) = A x + c x^3 - b.  Like the device side, it keeps the residual and the Jacobian of the LAST state evaluated, and
    solve_step solves with those.  accept(x) False: the state is rejected with the info ``bad``."""

    def __init__(self, c=0.5, b=(1.0, 2.0, 3.0), accept=lambda x: True, bad=BAD, correction=None):
        self.c, self.b, self.accept, self.bad, self.correction = c, np.asarray(b, dtype=float), accept, bad, correction
        self.evaluations, self.solves, self.commits, self.states = 0, 0, 0, []

    def evaluate(self, x):
        self.evaluations += 1
        self.states.append(x.copy())
        if not self.accept(x):
            return dict(self.bad), None
        self.r = A @ x + self.c * x ** 3 - self.b
        self.J = A + np.diag(3.0 * self.c * x ** 2)
        return dict(INFO), float(np.linalg.norm(self.r))

    def solve_step(self, it):
        self.solves += 1
        d = np.linalg.solve(self.J, -self.r) if self.correction is None else self.correction
        return d, {'krylov_iterations': 3 + it}

    def commit(self, info):
        self.commits += 1
        self.committed = info

    def run(self, settings=NewtonSettings(1e-9, 1e-10, 50, 1.0, False), texts=HYPERELASTIC_TEXTS, log=None, x0=np.zeros(3)):
        self.log = Log() if log is None else log
        return damped_newton(x0, self.evaluate, self.solve_step, settings, texts, self.log, self.commit)


def test_smooth_problem_converges_with_one_evaluation_per_iteration():
    p = Problem()
    run = p.run()
    assert 2 <= run.iterations <= 10
    assert len(run.history) == run.iterations + 1 and len(run.steps) == run.iterations
    assert run.steps == [1.0] * run.iterations
    assert [s['krylov_iterations'] for s in run.stats] == [3 + it for it in range(run.iterations)]
    assert p.evaluations == 1 + run.iterations and p.solves == run.iterations
    assert run.history[-1] / run.history[0] < 1e-9 <= run.history[-2] / run.history[0]
    assert np.linalg.norm(A @ run.x + 0.5 * run.x ** 3 - p.b) == run.history[-1]
    assert np.array_equal(run.x, p.states[-1]) and run.info == INFO        # the last evaluation was at the iterate returned
    assert p.commits == 1 and p.log.lines == []


def test_rejected_trials_halve_the_step():
    """c = 10, b = 10: the solution has |x| ~ 1.4, the full first step from 0 is A^-1 b, |.| ~ 5.5.  States outside |x| <= 3 are
    rejected, so the first step is cut."""
    radius = 3.0
    p = Problem(c=10.0, b=(10.0, 10.0, 10.0), accept=lambda x: np.linalg.norm(x) <= radius)
    assert np.linalg.norm(np.linalg.solve(A, p.b)) > radius
    run = p.run()
    assert min(run.steps) < 1.0 and run.steps[0] == 0.5
    trials = [1 + int(round(np.log2(1.0 / s))) for s in run.steps]
    assert p.evaluations == 1 + sum(trials) and p.solves == run.iterations == len(run.steps)
    assert np.linalg.norm(run.x) <= radius and len(run.history) == run.iterations + 1
    assert np.linalg.norm(A @ run.x + 10.0 * run.x ** 3 - p.b) < 1e-9 * run.history[0]
    assert p.log.lines == ['hyperelastic Newton: step of iteration 0 cut to 0.5 (inverted cells at the full step)']
    assert p.commits == 1


@pytest.mark.parametrize("texts,bad,message", [
    (HYPERELASTIC_TEXTS, BAD, 'hyperelastic Newton: at iteration 0 the step, halved 10 times, still inverts 2 cell(s), first cell 7: '
     + HYPER_HINT),
    (HYPERELASTIC_TEXTS, dict(BAD, n_inverted=0), 'hyperelastic Newton: at iteration 0 the step, halved 10 times, still gives a '
     'non-finite residual: ' + HYPER_HINT),
    (PLASTIC_TEXTS, BAD, 'plastic Newton: at iteration 0 the step, halved 10 times, still gives a non-finite residual: ' + PLASTIC_HINT)])
def test_eleven_rejections_in_a_row_raise(texts, bad, message):
    p = Problem(accept=lambda x: not x.any(), bad=bad)            # only the first iterate is accepted
    with pytest.raises(SolverError) as err:
        p.run(texts=texts)
    assert str(err.value) == message and 'halved 10 times' in message
    assert p.solves == 1 and p.evaluations == 12 and p.commits == 0
    d = np.linalg.solve(A, p.b)
    assert all(np.array_equal(x, 0.5 ** k * d) for k, x in enumerate(p.states[1:]))       # steps 1, 1/2, ..., 2^-10


@pytest.mark.parametrize("texts,tail", [(HYPERELASTIC_TEXTS, ''), (PLASTIC_TEXTS, ': ' + PLASTIC_HINT)])
def test_maximum_iterations(texts, tail):
    p = Problem()
    with pytest.raises(SolverError) as err:
        p.run(NewtonSettings(1e-9, 1e-10, 1, 1.0, False), texts)
    r1 = np.linalg.norm(A @ p.states[1] + 0.5 * p.states[1] ** 3 - p.b)
    assert str(err.value) == 'Newton solver did not converge in 1 iterations (residual {:.3e})'.format(r1) + tail
    assert p.solves == 1 and p.evaluations == 2 and p.commits == 0


def test_converged_first_iterate_solves_nothing():
    p = Problem()
    x0 = Problem().run().x
    run = p.run(NewtonSettings(1e-9, 1e-6, 50, 1.0, False), x0=x0)
    assert run.iterations == 0 and p.solves == 0 and p.evaluations == 1 and p.commits == 1
    assert len(run.history) == 1 and run.history[0] < 1e-6 and run.steps == [] and run.stats == []
    assert run.x is x0


def test_relaxation_parameter_is_the_step():
    p = Problem()
    run = p.run(NewtonSettings(1e-9, 1e-10, 50, 0.5, False))
    assert run.iterations > Problem().run().iterations and run.steps == [0.5] * run.iterations
    assert p.evaluations == 1 + run.iterations and p.log.lines == []           # a relaxed step is not a cut one


def test_the_record_of_a_failed_solve_tells_how_far_it_got():
    from fenicssolver_amd.solid_steps import NewtonRun
    p, rec = Problem(), NewtonRun()
    with pytest.raises(SolverError, match='did not converge in 2 iterations'):
        damped_newton(np.zeros(3), p.evaluate, p.solve_step, NewtonSettings(1e-9, 1e-10, 2, 1.0, False), PLASTIC_TEXTS, Log(), p.commit, rec)
    assert rec.iterations == 2 and len(rec.history) == 3 and rec.steps == [1.0, 1.0] and len(rec.stats) == 2 and rec.x is None


def test_every_other_message_is_the_one_the_solvers_have_always_given():
    # a rejected first iterate
    for texts, bad, message in [
            (HYPERELASTIC_TEXTS, BAD, 'hyperelastic Newton: the initial iterate (previous solution with the boundary values imposed) inverts '
             '2 cell(s), first cell 7: ' + HYPER_HINT),
            (HYPERELASTIC_TEXTS, dict(BAD, n_inverted=0), 'hyperelastic Newton: the residual of the initial iterate is not finite'),
            (PLASTIC_TEXTS, BAD, 'plastic Newton: the residual of the initial iterate is not finite')]:
        p = Problem(accept=lambda x: False, bad=bad)
        with pytest.raises(SolverError) as err:
            p.run(texts=texts)
        assert str(err.value) == message
        assert p.evaluations == 1 and p.solves == 0 and p.commits == 0
    # a correction that is not finite
    for texts, message in [(HYPERELASTIC_TEXTS, 'hyperelastic Newton: the correction of iteration 0 is not finite'),
                           (PLASTIC_TEXTS, 'plastic Newton: the correction of iteration 0 is not finite: ' + PLASTIC_HINT)]:
        p = Problem(correction=np.array([0.0, np.nan, 0.0]))
        with pytest.raises(SolverError) as err:
            p.run(texts=texts)
        assert str(err.value) == message
        assert p.evaluations == 1 and p.solves == 1 and p.commits == 0
    # the monitor line and the line of a cut step
    for texts, tail, cut in [(HYPERELASTIC_TEXTS, '', 'hyperelastic Newton: step of iteration 0 cut to 0.25 (inverted cells at the full step)'),
                             (PLASTIC_TEXTS, ', 5 cells yielding', 'plastic Newton: step of iteration 0 cut to 0.25 (non-finite residual at the full step)')]:
        p = Problem(accept=lambda x: p.evaluations not in (2, 3))          # the first two trials of iteration 0 are rejected
        run = p.run(NewtonSettings(1e-9, 1e-10, 50, 1.0, True), texts)
        assert run.steps[0] == 0.25 and p.log.lines[1] == cut
        r0, r1 = run.history[:2]
        assert p.log.lines[0] == "Newton iteration 0: r (abs) = %.3e (tol = %.3e) r (rel) = %.3e (tol = %.3e)" % (r0, 1e-10, 1.0, 1e-9) + tail
        assert p.log.lines[2] == "Newton iteration 1: r (abs) = %.3e (tol = %.3e) r (rel) = %.3e (tol = %.3e)" % (r1, 1e-10, r1 / r0, 1e-9) + tail
        assert len(p.log.lines) == 1 + run.iterations + sum(s != 1.0 for s in run.steps)
    # what the callers make of the record: the CG breakdown and the label of the linear solve
    assert HYPERELASTIC_TEXTS.breakdown.format(4, HYPERELASTIC_TEXTS.hint) == (
        'hyperelastic Newton: CG broke down at iteration 4 - the tangent is not positive definite there '
        '(a material instability, or a load step too large: ' + HYPER_HINT + ')')
    assert PLASTIC_TEXTS.breakdown.format(4, PLASTIC_TEXTS.hint) == (
        'plastic Newton: CG broke down at iteration 4 - the consistent tangent is singular there (a limit '
        'load with hardening_modulus = 0): ' + PLASTIC_HINT)
    assert HYPERELASTIC_TEXTS.name + ' Newton step' == 'hyperelastic Newton step' and PLASTIC_TEXTS.name + ' Newton step' == 'plastic Newton step'
    assert (HYPERELASTIC_TEXTS.hint, PLASTIC_TEXTS.hint) == (HYPER_HINT, PLASTIC_HINT)


def test_the_driver_needs_no_back_end():
    """solid_steps binds no back end at module level (its device functions import it when they are called), and the driver's globals
    are numpy, the error class and the records"""
    from fenicssolver_amd import solid_steps
    assert not {'backend', 'parallel', '_lib'} & set(vars(solid_steps))
    assert {n for n in damped_newton.__code__.co_names if n in vars(solid_steps)} == {'NewtonRun', 'SolverError', 'np'}
