"""CP linear tensor regression on MI355X — drop-in for the reference's
`standard_tensor_regression.py` (kimerein/tensor_regression).

Same module functions and `CP_linear_regression` class, same argument names, defaults,
Kruskal-factor list layout and `loss_running` semantics.  What changes is underneath:
the hot path — softplus + cp_to_tensor + inner(X, B) + MSELoss + backward + Adam
(standard_tensor_regression.py:458-470) — runs as gfx950 HIP kernels through the C ABI
(`include/tensor_regression_hip.h`), X is streamed from HBM once per iteration, and there is
no torch.autograd on that path.

Differences from the reference (all deliberate):
  * tensors must live on a HIP device (`device='cuda'`); the kernels compute in the model's
    dtype, float32 or float64 (dtype=torch.float64: a float64 two-pass path, csrc/tr_fp64.hip);
  * `lin_model` returns a non-differentiable tensor (the fit loops compute gradients in HIP);
  * a 2-D `y` is rejected (the reference silently broadcasts (N,) - (N,1) to (N,N), quirk Q11);
  * `fit_Adam` takes an optional `process_group` to fit sample shards over torch.distributed.
"""
import types

import numpy as np
import torch

from . import _engine, _fit, _lib, _many
from ._engine import Plan, as_device_f32, adam_hparams, run_adam_fit

__all__ = ["make_BcpInit", "non_neg_fn", "lin_model", "stepwise_model", "L2_penalty",
           "CP_linear_regression", "fit_Adam_many", "predict_many", "score_many"]


####################################
######## Helper functions ##########
####################################

def make_BcpInit(B_dims, rank, non_negative, scale=1, device='cpu', dtype=torch.float32):
    """Initial Kruskal factors (standard_tensor_regression.py:18-51).

    Orthogonal init with gain `scale`, drawn on the CPU generator exactly like the reference
    (so the same torch seed gives the same factors), then non-negative factors shifted by two
    standard deviations and halved — only when the first factor has more than one row
    (reference quirk Q6).
    """
    Bcp_init = [torch.nn.init.orthogonal_(torch.empty(B_dims[ii], rank, dtype=dtype), gain=scale).to(device)
                for ii in range(len(B_dims))]
    if Bcp_init[0].shape[0] > 1:
        Bcp_init = [(Bcp_init[ii] + torch.std(Bcp_init[ii]) * 2 * non_negative[ii]) / (non_negative[ii] + 1)
                    for ii in range(len(Bcp_init))]
    return Bcp_init


def non_neg_fn(B_cp, non_negative, softplus_kwargs=None):
    """Yield softplus(A_k) for flagged factors, A_k otherwise (standard…py:53-85)."""
    if softplus_kwargs is None:
        softplus_kwargs = {'beta': 50, 'threshold': 1}
    for ii in range(len(B_cp)):
        if non_negative[ii]:
            yield torch.nn.functional.softplus(B_cp[ii], **softplus_kwargs)
        else:
            yield B_cp[ii]


_plan_cache = {}


def _plan_for(model, feature_dims, n_classes, rank, rows, non_negative, softplus_kwargs, device,
              dtype=torch.float32):
    nf = len(feature_dims) + (1 if model == _lib.TR_MODEL_MULTINOMIAL else 0)
    beta, thr = _engine.softplus_params(softplus_kwargs)
    key = (model, tuple(int(d) for d in feature_dims), int(n_classes), int(rank),
           tuple(bool(non_negative[f]) for f in range(nf)), beta, thr, _engine.device_index(device), dtype)
    p = _plan_cache.get(key)
    if p is None or p.max_rows < rows:
        p = Plan(model, feature_dims, n_classes, rank, rows, non_negative, softplus_kwargs, device, dtype=dtype)
        _plan_cache[key] = p
    return p


def lin_model(X, Bcp, weights, non_negative, bias, softplus_kwargs=None):
    """y_hat = inner(X, cp_to_tensor((weights, non_neg_fn(Bcp)))[..., None], n_modes=len(Bcp)) + bias

    (standard_tensor_regression.py:87-130), computed by the gfx950 forward kernel.
    X: (N, I_1..I_K) on a HIP device; returns (N,) fp32 (no autograd graph).
    """
    if not isinstance(X, torch.Tensor) or X.device.type != "cuda":
        raise ValueError("lin_model: X must be a torch tensor on a HIP device (device='cuda')")
    K = len(Bcp)
    if list(X.shape[1:]) != [int(A.shape[0]) for A in Bcp] or X.ndim != K + 1:
        raise ValueError(f"Incorrect shapes for inner product along {K} common modes. "
                         f"tensor_1.shape={list(X.shape)}, factors={[tuple(A.shape) for A in Bcp]}")
    rank = int(Bcp[0].shape[1])
    dev = X.device
    dtype = X.dtype
    for A in Bcp:  # inner(X, B) is one matmul in the reference: operands of one dtype
        if torch.as_tensor(A).dtype != dtype:
            raise RuntimeError(f"expected m1 and m2 to have the same dtype, but got: {dtype} != "
                               f"{torch.as_tensor(A).dtype}")
    Xd = _engine.as_device_rows(X, dev.index, dtype)
    plan = _plan_for(_lib.TR_MODEL_LINEAR, X.shape[1:], 1, rank, 1, non_negative, softplus_kwargs, dev, dtype)
    arena = plan.pack([torch.as_tensor(A).to(dev) for A in Bcp], torch.as_tensor(bias).to(dev))
    w = torch.as_tensor(weights, dtype=dtype).to(dev).contiguous()
    return plan.forward(Xd, arena, w)


def stepwise_model(X, Bcp, weights, non_negative, bias, softplus_kwargs=None):
    """einsum form of lin_model for 3-D X (standard…py:133-177): the reference ignores
    `weights` here, i.e. it is lin_model with unit weights."""
    if Bcp[0].shape[1] == 0:
        return torch.zeros(1).to(X.device)
    rank = int(Bcp[0].shape[1])
    return lin_model(X, Bcp, torch.ones(rank, device=X.device), non_negative, bias, softplus_kwargs)


def L2_penalty(B_cp):
    """sum_k ||A_k||_F of the raw factors, not squared (standard…py:180-196)."""
    ii = 0
    for comp in B_cp:
        ii += torch.sqrt(torch.sum(comp ** 2))
    return ii


####################################
########### Main class #############
####################################

class CP_linear_regression():
    def __init__(self,
                 X_shape,
                 dtype=torch.float32,
                 rank=5,
                 non_negative=False,
                 weights=None,
                 Bcp_init=None,
                 Bcp_init_scale=1,
                 bias_init=0,
                 device='cpu',
                 softplus_kwargs=None):
        """CP linear regression y = <X, [[weights; softplus?(Bcp)]]> + bias
        (standard_tensor_regression.py:204-303; same arguments and attributes)."""
        self.dtype = dtype
        if weights is None:
            self.weights = torch.ones((rank), dtype=self.dtype, requires_grad=False, device=device)
        else:
            self.weights = torch.tensor(weights, dtype=self.dtype, requires_grad=False, device=device)
        self.softplus_kwargs = _fit.softplus_or_default(softplus_kwargs)
        self.rank = rank
        self.device = device
        self.non_negative = _fit.non_negative_flags(non_negative, len(X_shape))
        self.bias = torch.tensor([bias_init], dtype=self.dtype, requires_grad=True, device=device)
        B_dims = list(X_shape[1:])
        if Bcp_init is None:
            self.Bcp = make_BcpInit(B_dims, self.rank, self.non_negative, scale=Bcp_init_scale,
                                    device=self.device, dtype=self.dtype)
            for ii in range(len(B_dims)):
                self.Bcp[ii].requires_grad = True
        else:
            self.Bcp = Bcp_init
        self.loss_running = []
        self._plan = None

    # ---- plumbing --------------------------------------------------------------------------
    def _check_dtype(self):
        if self.dtype not in (torch.float32, torch.float64):
            raise NotImplementedError(f"the gfx950 kernels compute in float32 or float64; this model was built "
                                      f"with dtype={self.dtype}")

    def _get_plan(self, X, rows):
        from .util import HostStream
        if isinstance(X, HostStream):
            rows = min(rows, X.chunk_rows)
        dims = [int(A.shape[0]) for A in self.Bcp]
        if list(X.shape[1:]) != dims:
            raise ValueError(f"Incorrect shapes for inner product along {len(dims)} common modes. "
                             f"tensor_1.shape={list(X.shape)}, factors={[tuple(A.shape) for A in self.Bcp]}")
        p = self._plan
        dev = _engine.device_index(X.device if isinstance(X, torch.Tensor) else f"cuda:{X.dev_index}")
        if (p is None or p.max_rows < rows or p.feature_dims != dims or p.rank != int(self.Bcp[0].shape[1])
                or p.dev != dev or p.dtype != self.dtype
                or p.nonlin != _engine.nonlin_key(self.non_negative, self.softplus_kwargs, len(dims))):
            p = Plan(_lib.TR_MODEL_LINEAR, dims, 1, int(self.Bcp[0].shape[1]), rows, self.non_negative,
                     self.softplus_kwargs, f"cuda:{dev}", dtype=self.dtype)
            self._plan = p
        return p

    def _inputs(self, X, y):
        self._check_dtype()
        from .util import HostStream
        if isinstance(X, HostStream):  # out-of-core: X streams from host memory every iteration
            if self.dtype != torch.float32:
                raise NotImplementedError("HostStream streams float32 samples; this model is float64")
            dev = X.dev_index
            y = torch.as_tensor(y)
            if y.ndim != 1 or y.shape[0] != len(X):
                raise ValueError(f"y must be 1-D with len(y) == len(X); got y.shape={tuple(y.shape)}")
            return X, as_device_f32(y, dev), dev
        dev = _engine.compute_device(X, self.device)
        X = _engine.as_device_rows(X, dev, self.dtype)
        y = torch.as_tensor(y)
        if y.ndim != 1 or y.shape[0] != X.shape[0]:
            raise ValueError(f"y must be 1-D with len(y) == X.shape[0]; got y.shape={tuple(y.shape)}, "
                             f"X.shape[0]={X.shape[0]}")
        y = as_device_f32(y, dev, self.dtype)
        return X, y, dev

    # ---- fitting -----------------------------------------------------------------------------
    def fit(self, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
            running_loss_logging_interval=10, LBFGS_kwargs=None):
        """LBFGS fit (standard_tensor_regression.py:305-398).  torch.optim.LBFGS drives the
        parameters; every closure evaluation is one gfx950 loss+gradient pass."""
        _fit.require_lbfgs_kwargs(LBFGS_kwargs)
        X, y, dev = self._inputs(X, y)
        from .util import HostStream
        if isinstance(X, HostStream):
            raise NotImplementedError("the LBFGS fit needs X resident on the device (use fit_Adam for a HostStream)")
        N = X.shape[0]
        plan = self._get_plan(X, N)
        w = self.weights.to(f"cuda:{dev}", self.dtype).contiguous()
        grad, gtot, loss_out = _fit.lbfgs_buffers(plan, dev, self.dtype)
        var_y = torch.var(y).item() if verbose == 2 else None

        def closure_loss():
            arena = plan.pack(self.Bcp, self.bias)
            plan.loss_grad_checked(X, y, None, float(N), arena, w, grad)
            plan.finalize_grad(arena, grad, lambda_L2, gtot, loss_out)
            _fit.set_factor_grads(plan, gtot, self.Bcp, self.bias)
            return loss_out[0].clone()

        def log_loss(ii):  # the data loss of the forward kernel, without the L2 term
            y_hat = plan.forward(X, plan.pack(self.Bcp, self.bias), w)
            loss = torch.mean((y_hat - y) ** 2).item()
            return loss, (_fit.line_with_ratio(ii, loss, torch.var(y_hat).item() / var_y) if verbose == 2 else None)

        return _fit.lbfgs_fit(self.Bcp + [self.bias], LBFGS_kwargs, closure_loss, log_loss, stop="index",
                              max_iter=max_iter, tol=tol, patience=patience,
                              running_loss_logging_interval=running_loss_logging_interval, verbose=verbose,
                              loss_running=self.loss_running, after=plan.check_status)

    def fit_Adam(self, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
                 Adam_kwargs=None, process_group=None):
        """Adam fit (standard_tensor_regression.py:400-476), device resident on gfx950.

        X: a device tensor (samples may be a strided / windowed view, util.windowed_view) or a
        util.HostStream (host-resident X streamed through HBM in chunks every iteration).
        process_group: optional torch.distributed group; X / y are then this rank's sample
        shard and the per-iteration gradient arena is summed with one all-reduce.
        """
        hp = adam_hparams(Adam_kwargs)
        from .util import HostStream

        def prepare():
            Xd, yd, dev = self._inputs(X, y)
            if verbose == 2 and isinstance(Xd, HostStream):
                raise NotImplementedError("verbose=2 (per-iteration y_hat variance) is not offered for a HostStream X")
            return Xd, yd, dev, self._get_plan(Xd, Xd.shape[0])
        (X, y, dev, plan), n_global = _fit.start_adam(process_group, prepare, lambda o: float(o[0].shape[0]),
                                                      lambda o: o[3])
        arena = plan.pack(self.Bcp, self.bias)
        w = self.weights.to(f"cuda:{dev}", self.dtype).contiguous()
        vcb = _fit.VerbosePrinter(_fit.line_with_ratio, y, lambda a: plan.forward(X, a, w)) if verbose == 2 else None
        convergence_reached, _ = run_adam_fit(plan, X, y, None, n_global, arena, w, lambda_L2, max_iter, tol,
                                              patience, hp, self.loss_running, verbose_cb=vcb,
                                              process_group=process_group, arena_checked=True)
        plan.unpack_into(arena, self.Bcp, self.bias)
        return _fit.finish_fit(convergence_reached, verbose)

    ####################################
    ############ POST-HOC ##############
    ####################################

    def predict(self, X, Bcp=None, device=None, plot_pref=False):
        """y_hat as numpy (standard_tensor_regression.py:628-687); inputs are cast to fp32
        like the reference (quirk Q12)."""
        if device is None:
            device = self.device
        X, Bcp = _fit.coerce_predict_inputs(X, Bcp, self.Bcp, device)
        y_hat = lin_model(X, Bcp, self.weights, self.non_negative, self.bias,
                          softplus_kwargs=self.softplus_kwargs).detach().cpu().numpy()
        return y_hat

    def return_Bcp_final(self):
        """softplus-applied factors as numpy (standard…py:690-703)."""
        Bcp = list(non_neg_fn(self.Bcp, self.non_negative, softplus_kwargs=self.softplus_kwargs))
        return [Bcp[ii].detach().cpu().numpy() for ii in range(len(Bcp))]

    def detach_Bcp(self):
        return [Bcp.detach().cpu().numpy() for Bcp in self.Bcp]

    def get_params(self):
        return {
            'weights': self.weights.detach().cpu().numpy(),
            'Bcp': self.detach_Bcp(),
            'non_negative': self.non_negative,
            'softplus_kwargs': self.softplus_kwargs,
            'rank': self.rank,
            'device': self.device,
            'loss_running': self.loss_running}

    def set_params(self, params):
        self.weights = params['weights']
        self.Bcp = params['Bcp']
        self.non_negative = params['non_negative']
        self.softplus_kwargs = params['softplus_kwargs']
        self.rank = params['rank']
        self.device = params['device']
        self.loss_running = params['loss_running']
        self._plan = None

    def display_params(self):
        print('weights:', self.weights)
        print('Bcp:', self.Bcp)
        print('non_negative:', self.non_negative)
        print('softplus_kwargs:', self.softplus_kwargs)
        print('rank:', self.rank)
        print('device:', self.device)
        print('loss_running:', self.loss_running)

    def plot_outputs(self):
        plt = _fit.plot_loss(self.loss_running)
        Bcp_final = self.return_Bcp_final()
        fig, axs = plt.subplots(len(Bcp_final))
        for ii, val in enumerate(Bcp_final):
            axs[ii].set_title(f'factor {ii}')
            axs[ii].plot(val)
        fig.suptitle('components')


####################################
####### Many models, one X #########
####################################

# Groups of fewer models go to the models' own fit_Adam: the single-pass kernel reads X once per
# iteration and a group reads it twice, so a small group cannot win.  Measured (tools/
# linear_many_shapes.py, DESIGN.md "Shared-X linear sweep"): a group of 2 loses (0.86x the loop), 4 is
# the smallest measured size that wins at both shapes (1.66x and 1.68x).
LINEAR_MANY_MIN_BATCH = 4


_per_member = _many.per_member


def _targets(y, M):
    """y as M targets: one (N,) target for all models, or a list of M of them."""
    if isinstance(y, (list, tuple)) and len(y) > 0 and all(hasattr(e, "__len__") for e in y):
        if len(y) != M:
            raise ValueError(f"y: a list must hold one target per model ({M}), got {len(y)}")
        return list(y), False
    return [y] * M, True


def fit_Adam_many(models, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
                  Adam_kwargs=None, min_batch=None, report=None):
    """fit_Adam of many CP_linear_regression models over ONE X: the outer loop of a hyperparameter grid
    (demo_TensorRegression.ipynb: a fresh model per value of lambda_L2, every fit on the same X and y)
    with X streamed twice per iteration for a whole group of models instead of once per model.

    models: CP_linear_regression objects of this module, each with its own rank, non_negative,
    softplus_kwargs, weights, initial Bcp and bias; the feature dims of each must equal X.shape[1:].
    X: one device tensor for all models (a strided or util.windowed_view X is allowed).  y: one (N,)
    target for all models or a list of len(models) targets.  lambda_L2, max_iter, tol, patience and
    Adam_kwargs are each one value for all models or a list of len(models) values.  Afterwards every
    model is in the state its own `model.fit_Adam(X, y, ...)` would have left it, up to fp32 summation
    order (Bcp, bias, loss_running extended, plateau stops included); `model._plan` is untouched.  The
    returned list holds each model's convergence_reached.

    A model inside the envelope is fitted in a group: float32, two feature modes (3-D X), rank <= 32,
    P = I * J and X's row stride multiples of 4 floats (a stride below P, a windowed view, included),
    any N >= 1.  Groups hold up to 16 models in list order and run one after another; a group of fewer
    than `min_batch` models (None: LINEAR_MANY_MIN_BATCH) and every model outside the envelope go to
    their own fit_Adam, as does every model when X is a util.HostStream, the dtype is float64 or
    TR_LINEAR_MANY=0.  report (a dict) receives {'batched': indices, 'alone': indices, 'groups': n,
    'x_passes': n} (x_passes: passes over X made by the groups).  verbose=2 (a line per iteration) is
    not offered, and neither is process_group."""
    from .util import HostStream
    models = list(models)
    M = len(models)
    _many.check_models(models, CP_linear_regression, verbose, " of every model")
    given = dict(lambda_L2=lambda_L2, max_iter=max_iter, tol=tol, patience=patience, Adam_kwargs=Adam_kwargs)
    args = {k: _per_member(k, v, M) for k, v in given.items()}
    ys, shared_y = _targets(y, M)
    if min_batch is None:
        min_batch = LINEAR_MANY_MIN_BATCH
    if int(min_batch) < 1:
        raise ValueError(f"min_batch must be >= 1, got {min_batch}")
    _many.start_report(report, batched=[], alone=[], groups=0, x_passes=0)
    if M == 0:
        return []
    hps = [adam_hparams(ak) for ak in args["Adam_kwargs"]]  # TypeError on None, as fit_Adam
    if not isinstance(X, (torch.Tensor, HostStream)):
        raise TypeError(f"fit_Adam_many: X must be a torch tensor or a util.HostStream, got {type(X).__name__}")
    N = len(X) if isinstance(X, HostStream) else int(X.shape[0])
    for j, m in enumerate(models):
        m._check_dtype()
        dims = [int(A.shape[0]) for A in m.Bcp]
        if list(X.shape[1:]) != dims:
            raise ValueError(f"model {j}: Incorrect shapes for inner product along {len(dims)} common modes. "
                             f"tensor_1.shape={list(X.shape)}, factors={[tuple(A.shape) for A in m.Bcp]}")
    for j, yj in enumerate(ys[:1] if shared_y else ys):
        shp = tuple(torch.as_tensor(yj).shape) if not isinstance(yj, torch.Tensor) else tuple(yj.shape)
        if len(shp) != 1 or shp[0] != N:
            raise ValueError(f"y{'' if shared_y else f'[{j}]'} must be 1-D with len(y) == X.shape[0]; got "
                             f"y.shape={shp}, X.shape[0]={N}")
    # ---- routing ----
    inside = []
    grouped = (_engine.linear_many_enabled() and isinstance(X, torch.Tensor) and X.dtype == torch.float32
               and X.ndim == 3)
    if grouped:
        dev = _engine.compute_device(X, models[0].device)
        X = _engine.as_device_rows(X, dev, torch.float32)
        I0, I1 = int(X.shape[1]), int(X.shape[2])
        xld = int(X.stride(0)) if N > 1 else I0 * I1
        inside = [j for j, m in enumerate(models)
                  if m.dtype == torch.float32 and len(m.Bcp) == 2
                  and _engine.linear_many_envelope(I0, I1, xld, int(m.Bcp[0].shape[1]))]
    groups = [inside[k:k + _engine.LINEAR_MANY_MAX] for k in range(0, len(inside), _engine.LINEAR_MANY_MAX)]
    groups = [g for g in groups if len(g) >= int(min_batch)]
    batched = [j for g in groups for j in g]
    alone = [j for j in range(M) if j not in set(batched)]
    results, passes, y_dev = [False] * M, 0, {}

    def target(j):  # a shared y is uploaded once
        key = 0 if shared_y else j
        if key not in y_dev:
            y_dev[key] = as_device_f32(torch.as_tensor(ys[j]), dev, torch.float32)
        return y_dev[key]

    for g in groups:
        members, params = [], []
        for j in g:
            m = models[j]
            R = int(m.Bcp[0].shape[1])
            nn, beta, thr = _engine.nonlin_key(m.non_negative, m.softplus_kwargs, 2)
            factors = [torch.as_tensor(A) for A in m.Bcp]
            for f, A in enumerate(factors):
                if tuple(A.shape) != ((I0, I1)[f], R):
                    raise ValueError(f"model {j}: factor {f} has shape {tuple(A.shape)}, expected {((I0, I1)[f], R)}")
            params.append(factors + [torch.as_tensor(m.bias).detach().reshape(-1)[:1]])
            w = torch.as_tensor(m.weights).to(f"cuda:{dev}", torch.float32).contiguous()
            if w.numel() != R:
                raise ValueError(f"model {j}: weights holds {w.numel()} values, the rank is {R}")
            members.append(types.SimpleNamespace(
                y=target(j), w=w, rank=R, nonneg=nn, beta=beta, thr=thr, lambda_L2=args["lambda_L2"][j], hp=hps[j],
                max_iter=args["max_iter"][j], tol=args["tol"][j], patience=args["patience"][j],
                loss_running=m.loss_running))
        arena, offsets, slices = _many.pack_members(params, f"cuda:{dev}")
        for mb, own in zip(members, slices):
            mb.arena = own
        stops, n_pass = _engine.run_linear_many(dev, X, members)
        passes += n_pass
        _many.unpack_members(arena, offsets, [(*models[j].Bcp, models[j].bias) for j in g])
        for j, s in zip(g, stops):
            results[j] = s > 0
    for j in alone:  # outside the envelope, a small group or the route switched off: the model's own fit
        results[j] = models[j].fit_Adam(X, ys[j], verbose=False, **{k: v[j] for k, v in args.items()})
    return _many.finish_many(results, verbose, report, batched=batched, alone=alone, groups=len(groups),
                             x_passes=passes)


####################################
###### Scoring many models #########
####################################

# Groups of fewer models go to the models' own predict.  Measured (tools/linear_score_shapes.py,
# profiles/linear_score_shapes.txt, DESIGN.md "Scoring the linear sweep"): a group of 1 loses to predict
# plus host metrics at the notebook's shape (0.88x: the same one stream of X, more host work); 2 is the
# smallest measured size that wins at both shapes (1.69x and 2.11x).
LINEAR_SCORE_MIN_BATCH = 2


def _np64(t):
    """A target or prediction as a float64 numpy vector on the host."""
    if isinstance(t, torch.Tensor):
        t = t.detach().cpu().numpy()
    return np.asarray(t, dtype=np.float64).reshape(-1)


def _host_metrics(y_hat, y):
    """{'loss', 'var_ratio', 'r2'} of one prediction in float64 numpy.  N = 1 divides 0 by 0: nan, as the
    same formulas give in numpy, with no warning."""
    y_hat, y = _np64(y_hat), _np64(y)
    n = np.float64(y.shape[0])
    with np.errstate(all="ignore"):
        e = y_hat - y
        dh, dy = y_hat - y_hat.mean(), y - y.mean()
        sse, syy = np.float64(e @ e), np.float64(dy @ dy)
        return {"loss": float(sse / n), "var_ratio": float((np.float64(dh @ dh) / (n - 1)) / (syy / (n - 1))),
                "r2": float(1.0 - sse / syy)}


def _metrics_from_sums(s, N):
    """The same three numbers from tr_linear_many_score's five shifted fp64 sums."""
    s = np.asarray(s, dtype=np.float64)
    n = np.float64(N)
    with np.errstate(all="ignore"):
        shh = s[2] - s[1] * s[1] / n
        syy = s[4] - s[3] * s[3] / n
        return {"loss": float(s[0] / n), "var_ratio": float((shh / (n - 1)) / (syy / (n - 1))),
                "r2": float(1.0 - s[0] / syy)}


def _score_prelude(name, models, X, Bcp, ys, shared_y, min_batch, report):
    """The argument checks of predict_many and score_many, all before any device work; returns
    (the Bcp entry per model, min_batch, N)."""
    M = len(models)
    for m in models:
        if not isinstance(m, CP_linear_regression):
            raise TypeError(f"{name} takes this module's CP_linear_regression objects, got {type(m).__name__}")
    if Bcp is None:
        Bcp = [None] * M
    elif not isinstance(Bcp, (list, tuple)) or len(Bcp) != M:
        raise ValueError(f"Bcp: a list must hold one value per model ({M}), got "
                         f"{len(Bcp) if isinstance(Bcp, (list, tuple)) else type(Bcp).__name__}")
    if min_batch is None:
        min_batch = LINEAR_SCORE_MIN_BATCH
    if int(min_batch) < 1:
        raise ValueError(f"min_batch must be >= 1, got {min_batch}")
    _many.start_report(report, batched=[], alone=[], groups=0, x_passes=0)
    if M == 0:
        return [], int(min_batch), 0
    if not hasattr(X, "shape"):
        X = np.asarray(X)
    N = int(X.shape[0])
    for j, m in enumerate(models):
        m._check_dtype()
        factors = m.Bcp if Bcp[j] is None else Bcp[j]
        dims = [int(np.shape(A)[0]) for A in factors]
        if list(X.shape[1:]) != dims:
            raise ValueError(f"model {j}: Incorrect shapes for inner product along {len(dims)} common modes. "
                             f"tensor_1.shape={list(X.shape)}, factors={[tuple(np.shape(A)) for A in factors]}")
        R = int(np.shape(factors[0])[1])
        if any(tuple(np.shape(A)) != (d, R) for A, d in zip(factors, dims)):
            raise ValueError(f"model {j}: the factors {[tuple(np.shape(A)) for A in factors]} do not share one rank")
        nw = int(np.size(m.weights)) if not isinstance(m.weights, torch.Tensor) else int(m.weights.numel())
        if nw != R:
            raise ValueError(f"model {j}: weights holds {nw} values, the rank is {R}")
    if ys is not None:
        for j, yj in enumerate(ys[:1] if shared_y else ys):
            shp = tuple(torch.as_tensor(yj).shape) if not isinstance(yj, torch.Tensor) else tuple(yj.shape)
            if len(shp) != 1 or shp[0] != N:
                raise ValueError(f"y{'' if shared_y else f'[{j}]'} must be 1-D with len(y) == X.shape[0]; got "
                                 f"y.shape={shp}, X.shape[0]={N}")
    return list(Bcp), int(min_batch), N


def _score_many(name, models, X, ys, shared_y, Bcp, min_batch, report):
    """What predict_many (ys None) and score_many share: the prelude, the routing, the grouped call and
    the models that go alone."""
    models = list(models)
    M = len(models)
    Bcp, min_batch, N = _score_prelude(name, models, X, Bcp, ys, shared_y, min_batch, report)
    if M == 0:
        return []
    # ---- routing ----
    inside = []
    grouped = (_engine.linear_many_enabled() and isinstance(X, torch.Tensor) and X.dtype == torch.float32
               and X.ndim in (3, 4))
    if grouped:
        dev = _engine.compute_device(X, models[0].device)
        X = _engine.as_device_rows(X, dev, torch.float32)
        dims = [int(d) for d in X.shape[1:]]
        P = 1
        for d in dims:
            P *= d
        xld = int(X.stride(0)) if N > 1 else P
        for j, m in enumerate(models):
            factors = m.Bcp if Bcp[j] is None else Bcp[j]
            f32 = all(not isinstance(A, torch.Tensor) or A.dtype == torch.float32 for A in factors)
            if (m.dtype == torch.float32 and f32
                    and _engine.linear_score_envelope(dims, xld, int(np.shape(factors[0])[1]))):
                inside.append(j)
    groups = [inside[k:k + _engine.LINEAR_MANY_MAX] for k in range(0, len(inside), _engine.LINEAR_MANY_MAX)]
    groups = [g for g in groups if len(g) >= min_batch]
    batched = [j for g in groups for j in g]
    alone = [j for j in range(M) if j not in set(batched)]
    results = [None] * M
    if batched:
        y_dev, packed, params, w_dev = {}, {}, [], {}
        members = []
        for j in batched:
            m = models[j]
            _, factors = _fit.coerce_predict_inputs(X, Bcp[j], m.Bcp, m.device)  # the caller's list as predict's
            key = (id(m), id(factors))
            if key not in packed:  # every distinct factor list is packed once
                packed[key] = len(params)
                params.append([torch.as_tensor(A) for A in factors] + [torch.as_tensor(m.bias).detach().reshape(-1)[:1]])
            if id(m) not in w_dev:
                w_dev[id(m)] = torch.as_tensor(m.weights).to(f"cuda:{dev}", torch.float32).contiguous()
            nn, beta, thr = _engine.nonlin_key(m.non_negative, m.softplus_kwargs, len(dims))
            mb = types.SimpleNamespace(slot=packed[key], w=w_dev[id(m)], rank=int(factors[0].shape[1]), nonneg=nn,
                                       beta=beta, thr=thr, y=None)
            if ys is not None:
                ykey = 0 if shared_y else j  # a shared y is uploaded once
                if ykey not in y_dev:
                    y_dev[ykey] = as_device_f32(torch.as_tensor(ys[j]), dev, torch.float32)
                mb.y = y_dev[ykey]
            members.append(mb)
        arena, offsets, _ = _many.pack_members(params, f"cuda:{dev}")
        first = [0]
        for p in params[:-1]:
            first.append(first[-1] + len(p))
        for mb in members:
            mb.arena, mb.arena_at = arena, offsets[first[mb.slot]]
        out = _engine.run_linear_score(dev, X, members, "predict" if ys is None else "score")
        for j, o in zip(batched, out):
            results[j] = o if ys is None else _metrics_from_sums(o, N)
    for j in alone:  # outside the envelope, a small group or the route switched off: the model's own predict
        y_hat = models[j].predict(X, Bcp=Bcp[j])
        results[j] = y_hat if ys is None else _host_metrics(y_hat, ys[j])
    if report is not None:
        report.update(batched=batched, alone=alone, groups=len(groups), x_passes=len(groups))
    return results


def predict_many(models, X, Bcp=None, report=None, min_batch=None):
    """predict of many CP_linear_regression models over ONE X: [ (N,) float32 ndarray ], entry j equal to
    `models[j].predict(X, Bcp=Bcp[j])` up to fp32 summation order, with X streamed once per group of up
    to 16 models instead of once per model.

    models: CP_linear_regression objects of this module; the same object may appear more than once.  X:
    one device tensor for all of them (a row-contiguous view such as X[n_train:], a strided view or a
    util.windowed_view included).  Bcp: None, or a list with one entry per model, each None or a factor
    list handled as predict's Bcp.  The routing, `report` and `min_batch` are score_many's."""
    return _score_many("predict_many", models, X, None, True, Bcp, min_batch, report)


def score_many(models, X, y, report=None, min_batch=None):
    """Score many CP_linear_regression models over ONE X: [ {'loss', 'var_ratio', 'r2'} ] with
    loss = mean((y_hat - y)^2), the data loss fit_Adam records; var_ratio = var(y_hat) / var(y) with the
    unbiased variance, the number verbose=2 prints; r2 = 1 - sum (y_hat - y)^2 / sum (y - mean(y))^2.
    N = 1 gives what the same numpy formulas give (nan), with no warning.

    y: one (N,) target for all models or a list of len(models) targets.  A model inside the envelope is
    scored in a group: X a float32 device tensor with row-contiguous samples and two or three feature
    modes (3-D or 4-D), P and the row stride multiples of 4 floats, the model float32 with rank <= 32.
    Groups hold up to 16 models in list order and share one X stream each; only five fp64 sums per model
    (40 bytes) come back, all groups' in one copy, and no y_hat.  A group of fewer than `min_batch` models
    (None: LINEAR_SCORE_MIN_BATCH) and everything outside the envelope (float64, a numpy X, a
    util.HostStream, an unaligned P, rank above 32, TR_LINEAR_MANY=0) go to the model's own predict with
    the metrics formed on the host in float64.  report (a dict) receives {'batched': indices, 'alone':
    indices, 'groups': n, 'x_passes': n} (x_passes: passes over X made by the groups).  Arguments are
    checked before any device work."""
    models = list(models)
    ys, shared_y = _targets(y, len(models)) if len(models) else ([], True)
    return _score_many("score_many", models, X, ys, shared_y, None, min_batch, report)
