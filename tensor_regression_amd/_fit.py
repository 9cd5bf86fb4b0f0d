"""What the single-model fits of the model modules share: the LBFGS loop with the reference's two stop
rules, the start and the end of fit_Adam, its per-iteration printer, the gradient hand-back to the torch
leaves, and the constructor / predict / plot pieces the modules spelled out alike.  Plain functions that
take callables: what differs between models (which value is logged, what a line says, which stop rule)
is an argument.  Nothing here draws from an RNG.  The engine is reached as `_engine.<name>` at call time
(see _many.py)."""
import numpy as np
import torch

from . import _engine

DEFAULT_SOFTPLUS = {'beta': 50, 'threshold': 1}
CONVERGED = 'Convergence reached'
NOT_CONVERGED = 'Reached maximum number of iterations without convergence'
NAN_NOTICE = 'Loss is NaN. Stopping.'


# ---- constructor and post-hoc pieces ---------------------------------------------------------

def softplus_or_default(softplus_kwargs):
    return dict(DEFAULT_SOFTPLUS) if softplus_kwargs is None else softplus_kwargs


def non_negative_flags(non_negative, n):
    """True / False repeated for n factors; a list is the caller's own and kept as it is."""
    if non_negative is True:
        return [True] * n
    if non_negative is False:
        return [False] * n
    return non_negative


def coerce_predict_inputs(X, Bcp, own_Bcp, device):
    """predict's X and Bcp as tensors on `device`, cast to fp32 when they are not tensors (quirk Q12);
    a Bcp list given by the caller is converted in place, as in the reference."""
    if isinstance(X, torch.Tensor) is False:
        X = torch.tensor(X, dtype=torch.float32, requires_grad=False).to(device)
    elif X.device != torch.device(device):
        X = X.to(device)
    if Bcp is None:
        Bcp = own_Bcp
    elif isinstance(Bcp[0], torch.Tensor) is False:
        for ii in range(len(Bcp)):
            Bcp[ii] = torch.tensor(Bcp[ii], dtype=torch.float32, requires_grad=False).to(device)
    elif Bcp[0].device != torch.device(device):
        for ii in range(len(Bcp)):
            Bcp[ii] = Bcp[ii].to(device)
    return X, Bcp


def plot_loss(loss_running):
    """The "loss" figure every plot_outputs starts with; returns pyplot for the figures that follow."""
    import matplotlib.pyplot as plt
    plt.figure()
    plt.plot(loss_running)
    plt.xlabel('logged iteration')
    plt.ylabel('loss')
    plt.title('loss')
    return plt


# ---- what both fits use ----------------------------------------------------------------------

def line_plain(ii, loss, ratio=None):
    return f'Iteration: {ii}, Loss: {loss}'


def line_with_ratio(ii, loss, ratio):
    return f'Iteration: {ii}, Loss: {loss}  ;  Variance ratio (y_hat / y_true): {ratio}'


def convergence_line(convergence_reached):
    return CONVERGED if convergence_reached else NOT_CONVERGED


def finish_fit(convergence_reached, verbose, nan_stopped=False):
    """The end of a fit: the NaN notice (whatever `verbose` says), the convergence line for verbose >= 1;
    returns convergence_reached."""
    if nan_stopped:
        print(NAN_NOTICE)
    if (verbose is True) or (verbose >= 1):
        print(convergence_line(convergence_reached))
    return convergence_reached


# ---- LBFGS -----------------------------------------------------------------------------------

def require_lbfgs_kwargs(LBFGS_kwargs):
    """The reference's error for the default LBFGS_kwargs=None, raised before any device work."""
    if LBFGS_kwargs is None:
        raise TypeError("torch.optim.lbfgs.LBFGS() argument after ** must be a mapping, not NoneType")


def lbfgs_buffers(plan, dev, dtype=torch.float32):
    """(grad, gtot, loss_out) of plan.loss_grad / plan.finalize_grad on cuda:dev."""
    opts = dict(dtype=dtype, device=f"cuda:{dev}")
    return torch.zeros(plan.num_grads, **opts), torch.zeros(plan.num_params, **opts), torch.zeros(1, **opts)


def set_factor_grads(plan, gtot, tensors, bias=None):
    """Hand the arena gradient `gtot` back to the torch leaves: `tensors` in arena order by
    plan.offsets, `bias` (where the model has one) the rest of the arena after them."""
    o = plan.offsets
    for f, A in enumerate(tensors):
        A.grad = gtot[o[f]:o[f + 1]].to(A.device).clone().view(A.shape)
    if bias is not None:
        bias.grad = gtot[o[len(tensors)]:].to(bias.device).clone().view(bias.shape)


def stop_index(loss_running, ii, patience, tol):
    """The standard and multinomial modules' rule: indexed by the loop counter, so with a logging
    interval above 1 the slice may hold one entry, whose empty diff sums to 0 < tol."""
    return ii > patience and np.sum(np.abs(np.diff(loss_running[ii - patience:]))) < tol


def stop_length(loss_running, ii, patience, tol):
    """The spectral and convolutional modules' rule: over the last patience - 1 logged values.  None
    (not False) while the log is no longer than `patience`: only then does the reference look for NaN."""
    if len(loss_running) > patience:
        return np.sum(np.abs(np.diff(loss_running[-patience + 1:]))) < tol
    return None


def lbfgs_fit(params, LBFGS_kwargs, closure_loss, log_loss, *, stop, max_iter, tol, patience,
              running_loss_logging_interval, verbose, loss_running, after=None, on_optimizer=None):
    """The LBFGS loop of every model.  torch.optim.LBFGS drives `params`; `closure_loss()` computes the
    loss on the device and sets every .grad.  Every `running_loss_logging_interval` iterations
    `log_loss(ii)` returns (the value to append to loss_running, the line to print or None).
    stop: "index" (stop_index) or "length" (stop_length, then the NaN check that prints and stops).
    `on_optimizer(optimizer)` is called once before the loop, `after()` once after it.  Prints the
    convergence line for verbose >= 1 and returns convergence_reached."""
    require_lbfgs_kwargs(LBFGS_kwargs)
    stop_rule = {"index": stop_index, "length": stop_length}[stop]
    optimizer = torch.optim.LBFGS(params, **LBFGS_kwargs)
    if on_optimizer is not None:
        on_optimizer(optimizer)

    def closure():
        optimizer.zero_grad()
        return closure_loss()

    convergence_reached = False
    for ii in range(max_iter):
        if ii % running_loss_logging_interval == 0:
            value, line = log_loss(ii)
            loss_running.append(value)
            if line is not None:
                print(line)
        verdict = stop_rule(loss_running, ii, patience, tol)
        if verdict:
            convergence_reached = True
            break
        if verdict is None and np.isnan(loss_running[-1]):
            print(NAN_NOTICE)
            break
        optimizer.step(closure)
    if after is not None:
        after()
    return finish_fit(convergence_reached, verbose)


# ---- Adam ------------------------------------------------------------------------------------

def start_adam(process_group, prepare, local_norm, plan_of):
    """(prepare()'s result, the loss normaliser).  Under a process group one collective settles the start
    (_engine.fit_start): a rank-local failure of `prepare` raises on every rank, the arena sizes of
    `plan_of(prepared)` agree, and the normaliser is the sum of every rank's `local_norm(prepared)`."""
    if process_group is None:
        prepared = prepare()
        return prepared, local_norm(prepared)
    return _engine.fit_start(process_group, prepare, local_norm, lambda o: plan_of(o).num_params)


def yhat_from_loss_grad(plan, X, target, norm, weights):
    """arena -> the fit model's y_hat, from plan.loss_grad(..., yhat=) into buffers made once."""
    grad = torch.zeros(plan.num_grads, dtype=torch.float32, device=X.device)
    yhat = torch.empty_like(target)

    def yhat_of(arena):
        plan.loss_grad(X, target, None, norm, arena, weights, grad, yhat=yhat)
        return yhat
    return yhat_of


class VerbosePrinter:
    """The per-iteration print of fit_Adam (run_adam_fit's verbose_cb): `line(ii, loss, ratio)` with
    ratio = var(y_hat) / var(y), y_hat = `yhat_of(arena)` before the step.  Without `yhat_of` (the
    multinomial modules) no y_hat is computed and ratio is None."""

    def __init__(self, line, y=None, yhat_of=None):
        self.line, self.yhat_of, self.yhat = line, yhat_of, None
        self.var_y = None if yhat_of is None else torch.var(y).item()

    def before_step(self, arena):
        if self.yhat_of is not None:
            self.yhat = self.yhat_of(arena)

    def after_step(self, ii, loss):
        print(self.line(ii, loss, None if self.yhat_of is None else torch.var(self.yhat).item() / self.var_y))
