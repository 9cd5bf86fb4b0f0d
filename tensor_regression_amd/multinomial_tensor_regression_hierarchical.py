"""CP multinomial logistic tensor regression with one optimizer param group per factor on MI355X —
drop-in for the reference's `multinomial_tensor_regression_hierarchical.py` (kimerein/tensor_regression).

The model, the double softmax and the L2 term are the multinomial module's; what differs is the
optimizer of `fit_Adam` (hierarchical…py:436-440): `Bcp[0]`, `Bcp[1]` and `Bcp[2]` each sit in a
param group of their own, so that their learning rates can be set separately and changed during the
fit (the commented-out `optimizer.param_groups[2]['lr'] = …` of :450-452).  Consequences kept here:

  * a factor past the third (X with four or more dimensions) is in no group: it gets a gradient and
    counts in the L2 term of the recorded loss, but is never stepped and has no Adam state;
  * `fit_Adam` on a 2-D X raises IndexError, `Adam_kwargs` without 'lr' KeyError;
  * the loss is the unweighted CrossEntropyLoss; `fit` / `fit_Adam` take no `weights` (the
    constructor's `weights` are the CP component weights);
  * `get_params` / `display_params` read a `self.bias` that does not exist (AttributeError),
    `plot_outputs` unpacks four values from `predict`'s two (ValueError).

The one extension is `fit_Adam(..., group_lr=None)`, the learning-rate schedule of the three groups.
The fit runs the multinomial plan (class weights of ones, normaliser N) with the grouped update step
`tr_adam_step_groups`; with `group_lr=None` on a 3-D X it is bitwise the multinomial module's
`fit_Adam(weights=np.ones(C))`.
"""
import bisect
import functools
import math
import numbers
import types

import numpy as np
import torch

from . import _engine, _fit, _many
from ._engine import adam_hparams, run_adam_fit_groups
from . import multinomial_tensor_regression as _mnl
from .multinomial_tensor_regression import (squeeze_integers, confusion_matrix, idx_to_oneHot,  # noqa: F401
                                            make_BcpInit, non_neg_fn, model, L2_penalty,
                                            predict_many, score_many)

__all__ = ["squeeze_integers", "confusion_matrix", "idx_to_oneHot", "make_BcpInit", "non_neg_fn", "model",
           "L2_penalty", "CP_logistic_regression", "fit_Adam_many", "predict_many", "score_many"]

N_GROUPS = 3  # hierarchical…py:436-440: Bcp[0], Bcp[1], Bcp[2]


def _is_number(x):
    return isinstance(x, numbers.Real) and not isinstance(x, bool)


def _check_lr(lr, where):
    if not _is_number(lr) or not math.isfinite(float(lr)) or float(lr) < 0.0:
        raise ValueError(f"group_lr{where}: a learning rate must be a finite number >= 0, got {lr!r}")
    return float(lr)


def resolve_group_lr(group_lr, lr):
    """The schedule of the three param groups as [(starts, lrs)] * 3, `starts` increasing from 0.

    None: every group at `lr` for the whole fit (the reference).  Otherwise a sequence of exactly
    three entries, each a number or a list of (first_iteration, lr) pairs whose first pair starts at
    0 and whose starts strictly increase; anything else raises ValueError."""
    if group_lr is None:
        return [([0], [float(lr)]) for _ in range(N_GROUPS)]
    if isinstance(group_lr, (str, bytes, dict)) or not hasattr(group_lr, "__len__"):
        raise ValueError(f"group_lr must be None or a sequence of {N_GROUPS} entries, got {group_lr!r}")
    if len(group_lr) != N_GROUPS:
        raise ValueError(f"group_lr must have exactly {N_GROUPS} entries (Bcp[0], Bcp[1], Bcp[2]), "
                         f"got {len(group_lr)}")
    out = []
    for g, entry in enumerate(group_lr):
        if _is_number(entry):
            out.append(([0], [_check_lr(entry, f"[{g}]")]))
            continue
        if isinstance(entry, (str, bytes, dict)) or not hasattr(entry, "__len__") or len(entry) == 0:
            raise ValueError(f"group_lr[{g}] must be a number or a non-empty list of (first_iteration, lr) "
                             f"pairs, got {entry!r}")
        starts, lrs = [], []
        for k, pair in enumerate(entry):
            if isinstance(pair, (str, bytes, dict)) or not hasattr(pair, "__len__") or len(pair) != 2:
                raise ValueError(f"group_lr[{g}][{k}] must be a (first_iteration, lr) pair, got {pair!r}")
            s = pair[0]
            if not isinstance(s, numbers.Integral) or isinstance(s, bool):
                raise ValueError(f"group_lr[{g}][{k}]: first_iteration must be an integer, got {s!r}")
            if k == 0 and int(s) != 0:
                raise ValueError(f"group_lr[{g}]: the first pair must start at iteration 0, got {s}")
            if k > 0 and int(s) <= starts[-1]:
                raise ValueError(f"group_lr[{g}]: first_iteration must strictly increase, got {s} after "
                                 f"{starts[-1]}")
            starts.append(int(s))
            lrs.append(_check_lr(pair[1], f"[{g}][{k}]"))
        out.append((starts, lrs))
    return out


def lr_in_force(schedule, ii):
    """The three learning rates at loop index ii: for each group the lr of the last pair with
    first_iteration <= ii (`optimizer.param_groups[g]['lr'] = lr` run at the top of that iteration)."""
    return [lrs[bisect.bisect_right(starts, ii) - 1] for starts, lrs in schedule]


def _seq(x):
    return hasattr(x, "__len__") and not isinstance(x, (str, bytes, dict))


def _one_schedule(value):
    """Whether `value` reads as ONE group_lr (three entries, each a number or a list of (first_iteration,
    lr) pairs) rather than a list of one group_lr per model (entries None or themselves three-entry
    sequences, whose elements are numbers or lists of pairs — never pairs)."""
    return _seq(value) and len(value) == N_GROUPS and all(
        _is_number(e) or (_seq(e) and len(e) > 0 and all(_seq(x) and len(x) > 0 and _is_number(x[0]) for x in e))
        for e in value)


def _per_member(name, value, M):
    """One value for all M models, or a list of M values (ValueError on another length)."""
    return _many.per_member(name, value, M, _one_schedule if name == "group_lr" else None)


def fit_Adam_many(models, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False, Adam_kwargs=None,
                  group_lr=None, report=None):
    """fit_Adam of many independent models at once — the outer loop of a hyperparameter grid
    (demo_tensorRegression_forKim.ipynb: one freshly built model per grid point) as one launch per 64
    iterations, one workgroup per model.

    models: CP_logistic_regression objects of this module, each with its own X, y, rank, non_negative
    and initial factors.  lambda_L2, max_iter, tol, patience, Adam_kwargs and group_lr are each one
    value for all models or a list of len(models) values.  Afterwards every model is in exactly the
    state its own `model.fit_Adam(...)` with its own arguments would have left it (Bcp bitwise,
    loss_running extended); the returned list holds each model's convergence_reached.

    A model inside the resident envelope (3-D X, n_classes and rank <= 16, the problem within one
    CU's LDS; TR_MNL_RESIDENT not 0) is fitted in the batch; every other model by its own fit_Adam,
    one after another.  report (a dict) receives {'batched': indices, 'alone': indices, 'launches': n}.
    verbose=2 (a line per iteration) is not offered: it would force one launch per iteration."""
    models = list(models)
    M = len(models)
    _many.check_models(models, CP_logistic_regression, verbose, ", which forces one launch per iteration per model")
    given = dict(lambda_L2=lambda_L2, max_iter=max_iter, tol=tol, patience=patience, Adam_kwargs=Adam_kwargs,
                 group_lr=group_lr)
    args = {k: _per_member(k, v, M) for k, v in given.items()}
    _many.start_report(report, batched=[], alone=[], launches=0)
    if M == 0:
        return []
    # every member's own argument errors, in fit_Adam's order, before anything is launched
    hps, schedules = [], []
    for j, m in enumerate(models):
        ak = args["Adam_kwargs"][j]
        if ak is None:
            raise TypeError("'NoneType' object is not subscriptable")
        m.Bcp[0]
        lr0 = ak['lr']  # KeyError without 'lr'
        m.Bcp[1]
        m.Bcp[2]  # IndexError on a 2-D X
        hps.append(adam_hparams(ak))
        schedules.append(resolve_group_lr(args["group_lr"][j], lr0))
        _check_lr(lr0, " (Adam_kwargs['lr'])")
    devs = {_engine.compute_device(m.X, m.device) for m in models}
    if len(devs) != 1:
        raise ValueError(f"fit_Adam_many: the models are on different devices ({sorted(devs)})")
    dev = devs.pop()
    on = _engine.resident_enabled()
    batched, alone = [], []
    for j, m in enumerate(models):
        inside = (on and len(m.Bcp) == N_GROUPS and getattr(m.X, "ndim", 0) == 3 and int(m.X.shape[0]) <= _engine.resident_max_rows(
            m.Bcp[0].shape[0], m.Bcp[1].shape[0], m.Bcp[2].shape[0], m.Bcp[0].shape[1]))
        (batched if inside else alone).append(j)
    results, launches = [False] * M, 0
    if batched:
        members, params = [], []
        for j in batched:
            m = models[j]
            _, Xd, yd = m._device_data()
            dims = [int(A.shape[0]) for A in m.Bcp]
            if list(Xd.shape[1:]) != dims[:2]:
                raise ValueError(f"Incorrect shapes for inner product along 2 common modes. "
                                 f"tensor_1.shape={list(Xd.shape)}, factors={[tuple(A.shape) for A in m.Bcp]}")
            R = int(m.Bcp[0].shape[1])
            nn, beta, thr = _engine.nonlin_key(m.non_negative, m.softplus_kwargs, N_GROUPS)
            mb = types.SimpleNamespace(
                X=Xd, y=yd, n_classes=dims[2], rank=R, nonneg=nn, beta=beta, thr=thr, lambda_L2=args["lambda_L2"][j],
                hp=hps[j], lr_at=functools.partial(lr_in_force, schedules[j]),
                breaks=sorted({s for starts, _ in schedules[j] for s in starts[1:]}), max_iter=args["max_iter"][j],
                tol=args["tol"][j], patience=args["patience"][j], loss_running=m.loss_running,
                w=m.weights.to(f"cuda:{dev}", torch.float32).contiguous())
            factors = [torch.as_tensor(A) for A in m.Bcp]
            for f, A in enumerate(factors):
                if tuple(A.shape) != (dims[f], R):
                    raise ValueError(f"factor {f} has shape {tuple(A.shape)}, expected {(dims[f], R)}")
            members.append(mb)
            params.append(factors)
        arena, offsets, slices = _many.pack_members(params, f"cuda:{dev}")
        for mb, own in zip(members, slices):
            mb.arena = own
        stops, launches = _engine.run_resident_many(dev, members)
        _many.unpack_members(arena, offsets, [models[j].Bcp for j in batched])
        for j, s in zip(batched, stops):
            results[j] = s > 0
    for j in alone:  # outside the envelope (or the route switched off): the model's own fit, one after another
        results[j] = models[j].fit_Adam(verbose=False, **{k: v[j] for k, v in args.items()})
    return _many.finish_many(results, verbose, report, batched=batched, alone=alone, launches=launches)


class CP_logistic_regression(_mnl.CP_logistic_regression):
    _takes_host_stream = False

    def __init__(self, X, y, rank=5, non_negative=False, weights=None, Bcp_init=None, Bcp_init_scale=1,
                 device='cpu', softplus_kwargs=None):
        """(hierarchical…py:215-290; same arguments, attributes and RNG draws): the multinomial
        constructor, without a HostStream X and with a class factor that a fit never resizes."""
        super().__init__(X, y, rank=rank, non_negative=non_negative, weights=weights, Bcp_init=Bcp_init,
                         Bcp_init_scale=Bcp_init_scale, device=device, softplus_kwargs=softplus_kwargs)
        self._class_factor_auto = False

    def _ones(self):
        """The unweighted CrossEntropyLoss as the multinomial plan's class weights."""
        return np.ones(int(self.Bcp[-1].shape[0]), dtype=np.float32)

    # ---- fitting -------------------------------------------------------------------------------
    def fit(self, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
            running_loss_logging_interval=10, LBFGS_kwargs=None):
        """LBFGS fit over every factor (hierarchical…py:292-381); closures evaluated on gfx950."""
        return super().fit(lambda_L2=lambda_L2, max_iter=max_iter, tol=tol, patience=patience,
                           weights=self._ones(), verbose=verbose,
                           running_loss_logging_interval=running_loss_logging_interval, LBFGS_kwargs=LBFGS_kwargs)

    def fit_Adam(self, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False, Adam_kwargs=None,
                 group_lr=None):
        """Adam fit with a param group per factor (hierarchical…py:383-470), device resident on gfx950.

        group_lr: None (the reference: every group at Adam_kwargs['lr']), or three entries for
        Bcp[0], Bcp[1], Bcp[2], each a learning rate or a list of (first_iteration, lr) pairs —
        `optimizer.param_groups[g]['lr'] = lr` executed at the top of iteration first_iteration."""
        # the reference builds its param groups before anything else (:436-440)
        if Adam_kwargs is None:
            raise TypeError("'NoneType' object is not subscriptable")
        self.Bcp[0]
        lr0 = Adam_kwargs['lr']  # KeyError without 'lr'
        self.Bcp[1]
        self.Bcp[2]  # IndexError on a 2-D X
        hp = adam_hparams(Adam_kwargs)
        schedule = resolve_group_lr(group_lr, lr0)
        _check_lr(lr0, " (Adam_kwargs['lr'])")
        dev, Xd, yd = self._device_data()
        plan = self._get_plan(Xd, Xd.shape[0])
        cw, W = self._class_weights(self._ones(), dev, yd)
        arena = plan.pack(self.Bcp)
        w = self.weights.to(f"cuda:{dev}", torch.float32).contiguous()
        frozen = [0.0] * (plan.n_factors - N_GROUPS)
        vcb = _fit.VerbosePrinter(_fit.line_plain) if verbose == 2 else None
        # the resident route (one workgroup, whole iterations per launch) wherever the plan's envelope
        # admits the problem; plan.describe names the route taken
        resident = plan.set_resident(True)
        breaks = sorted({s for starts, _ in schedule for s in starts[1:]})
        convergence_reached, _ = run_adam_fit_groups(
            plan, Xd, yd, cw, W, arena, w, lambda_L2, max_iter, tol, patience, hp, self.loss_running,
            lambda ii: lr_in_force(schedule, ii) + frozen, range(N_GROUPS), verbose_cb=vcb, resident=resident,
            breaks=breaks)
        plan.unpack_into(arena, self.Bcp)
        return _fit.finish_fit(convergence_reached, verbose)

    def predict(self, X=None, y_true=None, Bcp=None, device=None, plot_pref=False):
        """(probabilities, argmax) as numpy (hierarchical…py:473-549; y_true and plot_pref are
        accepted and unused there too)."""
        return super().predict(X=X, y_true=y_true, Bcp=Bcp, device=device)

    def get_params(self):
        """(hierarchical…py:618-632): reads self.bias, which this model does not have."""
        return {'X': self.X.detach().cpu().numpy(),
                'y': self.y.detach().cpu().numpy(),
                'weights': self.weights.detach().cpu().numpy(),
                'Bcp': self.detach_Bcp(),
                'bias': self.bias.detach().cpu().numpy(),
                'non_negative': self.non_negative,
                'softplus_kwargs': self.softplus_kwargs,
                'rank': self.rank,
                'device': self.device,
                'loss_running': self.loss_running}

    def set_params(self, params):
        """(hierarchical…py:634-652)"""
        self.X = params['X']
        self.y = params['y']
        self.weights = params['weights']
        self.Bcp = params['Bcp']
        self.bias = params['bias']
        self.non_negative = params['non_negative']
        self.softplus_kwargs = params['softplus_kwargs']
        self.rank = params['rank']
        self.device = params['device']
        self.loss_running = params['loss_running']
        self._plan = None
        self._dev_cache = None
        self._cw_cache = None

    def display_params(self):
        """(hierarchical…py:654-668)"""
        print('X:', self.X.shape)
        print('y:', self.y.shape)
        print('weights:', self.weights)
        print('Bcp:', self.Bcp)
        print('bias', self.bias)
        print('non_negative:', self.non_negative)
        print('softplus_kwargs:', self.softplus_kwargs)
        print('rank:', self.rank)
        print('device:', self.device)
        print('loss_running:', self.loss_running)

    def plot_outputs(self):
        """(hierarchical…py:670-700): unpacks four values from predict's two."""
        plt = _fit.plot_loss(self.loss_running)
        prob, pred, cm, acc = self.predict()
        fig, axs = plt.subplots(2)
        axs[0].imshow(idx_to_oneHot(pred, self.n_classes), aspect='auto', interpolation='none')
        axs[1].imshow(idx_to_oneHot(self.y.detach().cpu().numpy(), self.n_classes), aspect='auto',
                      interpolation='none')
        axs[1].set_xlabel('class')
        fig.suptitle('predictions')
        cm, acc = self.make_confusion_matrix(prob_or_pred='pred')
        fig = plt.figure()
        plt.imshow(cm)
        plt.ylabel('true class')
        plt.xlabel('predicted class')
        plt.title('confusion matrix (predictions)')
        Bcp_final = self.return_Bcp_final()
        fig, axs = plt.subplots(len(Bcp_final))
        for ii, val in enumerate(Bcp_final):
            axs[ii].set_title(f'factor {ii}')
            axs[ii].plot(val)
        fig.suptitle('components')
