"""Host-side checks of the shared fit driver (tensor_regression_amd._fit), no GPU.

lbfgs_fit runs a scripted `log_loss` and a do-nothing closure over one dummy parameter (a zero gradient:
torch.optim.LBFGS returns after one closure evaluation, so closure calls count optimizer steps).  The
expected (convergence_reached, optimizer steps, len(loss_running)) are the reference's two loop bodies
run on the same sequences: the "index" rule of the standard and multinomial modules and the "length"
rule (with its NaN check) of the spectral and convolutional ones.
"""
import itertools
import types

import pytest
import torch

from tensor_regression_amd import _fit, _many

HALVING = lambda: (2.0 ** -k for k in itertools.count())  # noqa: E731
ONE_THEN_NAN = lambda: itertools.chain([1.0], itertools.repeat(float("nan")))  # noqa: E731
CONSTANT = lambda: itertools.repeat(1.0)  # noqa: E731

#        losses        tol   patience interval max_iter  index rule        length rule
CASES = [
    (HALVING,      1e-3, 3,  1, 100, (True, 13, 14),    (True, 10, 11)),
    (HALVING,      1e-3, 3,  4, 100, (True, 4, 2),      (True, 40, 11)),   # index: the one-entry slice
    (HALVING,      0.0,  3,  4, 100, (False, 100, 25),  (False, 100, 25)),
    (HALVING,      1e-3, 10, 1, 6,   (False, 6, 6),     (False, 6, 6)),
    (ONE_THEN_NAN, 1e-3, 3,  1, 100, (False, 100, 100), (False, 1, 2)),
    (CONSTANT,     1e-3, 1,  1, 100, (True, 2, 3),      (True, 1, 2)),
]


def _run(losses, stop, tol, patience, interval, max_iter, verbose=False, line=None, **kw):
    p = torch.zeros(1, requires_grad=True)
    seq, steps, loss_running = losses(), [], []

    def closure_loss():
        steps.append(1)
        p.grad = torch.zeros_like(p)
        return torch.zeros(())

    def log_loss(ii):
        return next(seq), (None if line is None else line(ii))

    conv = _fit.lbfgs_fit([p], {'lr': 1.0}, closure_loss, log_loss, stop=stop, max_iter=max_iter, tol=tol,
                          patience=patience, running_loss_logging_interval=interval, verbose=verbose,
                          loss_running=loss_running, **kw)
    return bool(conv), len(steps), len(loss_running)


@pytest.mark.parametrize("case", range(len(CASES)))
@pytest.mark.parametrize("stop", ["index", "length"])
def test_stop_rules_on_scripted_losses(case, stop, capsys):
    losses, tol, patience, interval, max_iter, want_index, want_length = CASES[case]
    got = _run(losses, stop, tol, patience, interval, max_iter)
    assert got == (want_index if stop == "index" else want_length)
    nan_stop = losses is ONE_THEN_NAN and stop == "length"  # the index rule never looks for NaN
    assert capsys.readouterr().out == ("Loss is NaN. Stopping.\n" if nan_stop else "")


def test_stop_rule_functions():
    assert not _fit.stop_index([1.0, 1.0, 1.0], 3, 3, 1e-3)          # ii == patience: not yet
    assert _fit.stop_index([1.0, 0.5], 4, 3, 1e-3)                   # one entry left: an empty diff sums to 0
    assert not _fit.stop_index([1.0, 0.5, 0.25, 0.125, 0.0625], 4, 3, 1e-3)
    assert _fit.stop_length([1.0, 1.0], 0, 3, 1e-3) is None          # too short: the caller looks for NaN
    assert _fit.stop_length([9.0, 1.0, 1.0, 1.0], 0, 3, 1e-3)        # the last patience - 1 values
    assert not _fit.stop_length([1.0, 1.0, 1.0, 2.0], 0, 3, 1e-3)


def test_lbfgs_kwargs_none_is_the_reference_error():
    want = r"torch\.optim\.lbfgs\.LBFGS\(\) argument after \*\* must be a mapping, not NoneType"
    with pytest.raises(TypeError, match=want):
        _fit.lbfgs_fit([torch.zeros(1, requires_grad=True)], None, None, None, stop="index", max_iter=1, tol=0.0,
                       patience=1, running_loss_logging_interval=1, verbose=False, loss_running=[])
    with pytest.raises(TypeError, match=want):
        _fit.require_lbfgs_kwargs(None)


@pytest.mark.parametrize("verbose", [False, True, 1, 2])
@pytest.mark.parametrize("converges", [True, False])
def test_convergence_line_and_hooks(verbose, converges, capsys):
    seen = []
    got = _run(CONSTANT, "index", 1e-3, 1, 1, 100 if converges else 2, verbose=verbose,
               line=lambda ii: f"logged {ii}", after=lambda: seen.append("after"),
               on_optimizer=lambda o: seen.append(type(o)))
    assert got[0] is converges
    assert seen == [torch.optim.LBFGS, "after"]
    last = "Convergence reached" if converges else "Reached maximum number of iterations without convergence"
    lines = [f"logged {ii}" for ii in range(got[2])] + ([] if verbose is False else [last])
    assert capsys.readouterr().out == "".join(s + "\n" for s in lines)


def test_finish_fit(capsys):
    assert _fit.finish_fit(True, False) is True
    assert capsys.readouterr().out == ""
    assert _fit.finish_fit(True, 1) is True
    assert capsys.readouterr().out == "Convergence reached\n"
    assert _fit.finish_fit(False, True) is False
    assert capsys.readouterr().out == "Reached maximum number of iterations without convergence\n"
    assert _fit.finish_fit(False, False, nan_stopped=True) is False  # the NaN notice does not ask `verbose`
    assert capsys.readouterr().out == "Loss is NaN. Stopping.\n"
    assert _fit.finish_fit(False, 3, nan_stopped=True) is False
    assert capsys.readouterr().out == ("Loss is NaN. Stopping.\n"
                                       "Reached maximum number of iterations without convergence\n")
    _many.finish_many([True, False], True, None)  # the many-model routes word it the same
    assert capsys.readouterr().out == ("model 0: Convergence reached\n"
                                       "model 1: Reached maximum number of iterations without convergence\n")


def test_non_negative_flags_and_softplus_default():
    assert _fit.non_negative_flags(True, 3) == [True, True, True]
    assert _fit.non_negative_flags(False, 2) == [False, False]
    own = [True, False, True]
    assert _fit.non_negative_flags(own, 5) is own  # a list is kept, whatever its length
    assert _fit.softplus_or_default(None) == {'beta': 50, 'threshold': 1}
    assert _fit.softplus_or_default(None) is not _fit.softplus_or_default(None)  # a dict of the model's own
    kw = {'beta': 2, 'threshold': 20}
    assert _fit.softplus_or_default(kw) is kw


def test_set_factor_grads_slices_by_plan_offsets():
    plan = types.SimpleNamespace(offsets=[0, 6, 10, 16])
    gtot = torch.arange(18, dtype=torch.float32)
    A, B, C = torch.zeros(3, 2), torch.zeros(2, 2), torch.zeros(3, 2, 1)
    bias = torch.zeros(2)
    _fit.set_factor_grads(plan, gtot, [A, B, C], bias)
    assert torch.equal(A.grad, gtot[0:6].view(3, 2)) and torch.equal(B.grad, gtot[6:10].view(2, 2))
    assert torch.equal(C.grad, gtot[10:16].view(3, 2, 1)) and torch.equal(bias.grad, gtot[16:18])
    gtot += 1  # the leaves own their gradients
    assert A.grad[0, 0] == 0 and bias.grad[0] == 16
    D = torch.zeros(3, 2)
    _fit.set_factor_grads(types.SimpleNamespace(offsets=[0, 6, 10]), gtot, [D, B])  # no bias: the tail is unread
    assert torch.equal(D.grad, gtot[0:6].view(3, 2)) and torch.equal(B.grad, gtot[6:10].view(2, 2))


def test_start_adam_without_a_process_group():
    calls = []

    def prepare():
        calls.append(1)
        return ("X", "plan")

    def no_plan(o):
        raise AssertionError("the arena size is only compared under a process group")

    assert _fit.start_adam(None, prepare, lambda o: 7.0, no_plan) == (("X", "plan"), 7.0)
    assert calls == [1]


def test_verbose_printer(capsys):
    vp = _fit.VerbosePrinter(_fit.line_plain)  # the multinomial form: no y_hat
    vp.before_step(None)
    vp.after_step(3, 0.5)
    y = torch.tensor([0.0, 2.0])
    vp = _fit.VerbosePrinter(_fit.line_with_ratio, y, lambda arena: arena * 2)
    vp.before_step(y)
    vp.after_step(4, 0.25)
    assert capsys.readouterr().out == ("Iteration: 3, Loss: 0.5\n"
                                       "Iteration: 4, Loss: 0.25  ;  Variance ratio (y_hat / y_true): 4.0\n")
