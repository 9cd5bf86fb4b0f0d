"""What the three convolutional models share (convolutional_spectral_, phase_constrained_spectral_
convolutional_ and convolutional_fourier_tensor_regression): the helper functions all of them use,
the plan cache, and two base classes.

  ConvModelBase     constructor body, plan / input plumbing, both fits (their loop, printer and end
                    are _fit's, shared with the other modules), predict and the post-hoc methods
                    every model has.
  SmoothConvModel   what the phase and Fourier models add to it alike: the smoothness arguments of
                    both fits, `self.optimizer`, `y_spectrum`, get_params / set_params / detach_Bcp.

The reference's three modules differ from one another in points that are kept for parity (which
softplus parameters fit_Adam and predict use, how lambda_L2 is read, what verbose prints, what the
constructor refuses).  Each of them is one class attribute or one small overridable method here,
set in the public module of the model it belongs to.
"""
import numpy as np
import torch

from . import _engine, _fit
from ._engine import adam_hparams, as_device_f32, run_adam_fit

_OWN = object()  # _plan_for: the model's own softplus_kwargs


####################################
######## Helper functions ##########
####################################

def make_BcpInit(B_dims, rank, non_negative, complex_dims=None, scale=1, device='cpu', dtype=torch.float32):
    """Initial Kruskal factors (…py:19-65): an orthogonal draw per factor with unit-norm columns;
    non-negative factors are shifted by two standard deviations and normalised again; a complex
    dim of 1 is squeezed away.  Draws come from torch's global generator of `device`, in list order."""
    if complex_dims is None:
        complex_dims = [1] * len(B_dims)
    out = []
    for n_rows, cdim, nn in zip(B_dims, complex_dims, non_negative):
        A = torch.nn.init.orthogonal_(torch.empty(n_rows, rank, cdim, dtype=dtype, device=device))
        A = A / torch.norm(A, dim=0)[None, ...]
        if nn:
            A = A + torch.std(A) * 2
            A = A / torch.norm(A, dim=0)[None, ...]
        if cdim == 1:
            A = A.squeeze(-1)
        out.append(A * scale)
    return out


def non_neg_fn(B_cp, non_negative, softplus_kwargs=None):
    """Yield softplus(A_k) for flagged factors, A_k otherwise (…py:67-93; None = beta 50 / threshold 1
    here, where the reference would fail on `**None`)."""
    if softplus_kwargs is None:
        softplus_kwargs = _fit.DEFAULT_SOFTPLUS
    for A, nn in zip(B_cp, non_negative):
        yield torch.nn.functional.softplus(A, **softplus_kwargs) if nn else A


def gaussian(x, mu, sig, plot_pref=False):
    """Normalised gaussian of x and its parameters (…py:101-131)."""
    gaus = 1 / (np.sqrt(2 * np.pi) * sig) * np.exp(-np.power((x - mu) / sig, 2) / 2)
    if plot_pref:
        import matplotlib.pyplot as plt
        plt.figure()
        plt.plot(x, gaus)
        plt.xlabel('x')
    return gaus, {"x": x, "mu": mu, "sig": sig}


def _lambda3(lambda_L2, n_factors):
    """lambda_L2 as the phase and Fourier references read it (…py:1245-1249, 1385-1389): a scalar or a
    length-1 list is repeated for (w, d, out); anything else is indexed [0], [1], [2]."""
    if isinstance(lambda_L2, (int, float)):
        return [float(lambda_L2)] * (1 + n_factors)
    if isinstance(lambda_L2, list) and len(lambda_L2) == 1:
        return [float(lambda_L2[0])] * (1 + n_factors)
    return [float(lambda_L2[0]), float(lambda_L2[1]), float(lambda_L2[2])]


def _series(X, dev=None):
    """X as an fp32 (T, D) device tensor with contiguous rows."""
    if isinstance(X, torch.Tensor) and X.dtype == torch.float64:
        raise NotImplementedError("the gfx950 conv kernel computes in fp32; got a float64 X")
    if type(X).__name__ == "HostStream":
        raise NotImplementedError("HostStream is not offered for the convolutional model")
    if not isinstance(X, torch.Tensor):
        X = torch.as_tensor(np.asarray(X), dtype=torch.float32)
    if dev is None:
        if X.device.type != "cuda":
            raise ValueError("X must be a torch tensor on a HIP device (device='cuda')")
        dev = X.device.index
    if X.ndim != 2:
        raise ValueError(f"X must be the untiled (T, D) series; got {tuple(X.shape)}")
    X = _engine.as_device_rows(X, dev)
    return X, dev


_plan_cache = {}


def _cached_plan(plan_cls, shape, rows, non_negative, softplus_kwargs, dev):
    """The plan of `plan_cls` for `shape` (its leading constructor arguments), rebuilt when the cached
    one was created for fewer series rows."""
    beta, thr = _engine.softplus_params(softplus_kwargs)
    key = (plan_cls,) + tuple(shape) + (tuple(bool(non_negative[f]) for f in range(3)), beta, thr, dev)
    p = _plan_cache.get(key)
    if p is None or p.max_rows < rows:
        p = plan_cls(*shape, rows, non_negative, softplus_kwargs, f"cuda:{dev}")
        _plan_cache[key] = p
    return p


####################################
########## Base classes ############
####################################

class ConvModelBase:
    _plan_cls = None             # the _engine plan class of the model
    _verbose_levels = (2, 3)     # values of `verbose` that print every logged iteration
    _keeps_optimizer = False     # both fits leave `self.optimizer` behind
    _default_softplus_in_adam = False  # fit_Adam and predict run beta 50 / threshold 1, not self.softplus_kwargs

    @staticmethod
    def _check_ctor(y_shape, dtype, temporal_window):
        if int(temporal_window) % 2 == 0 or int(temporal_window) < 1:
            raise ValueError(f"temporal_window must be odd and >= 1 (got {temporal_window}): with an even window "
                             "the reference's y_hat (T - W + 1 rows) and y[idx_conv] (T - W rows) never match")
        if len(y_shape) < 2:
            raise ValueError("y must be 2-D (T, n_out); the reference's model breaks at the first fit on a 1-D y")
        if dtype == torch.float64:
            raise NotImplementedError("the gfx950 conv kernel computes in fp32; fp64 is not offered")

    def _init_model(self, X_shape, y_shape, dtype, rank_normal, temporal_window, rank_spectral, non_negative,
                    weights, Bcp_init, Bcp_init_scale, spectral_complex_dims, device, softplus_kwargs):
        """The constructor body the three models share.  RNG draws in the reference's order: Bcp_w normal
        ranks, Bcp_w spectral ranks (`spectral_complex_dims` is their make_BcpInit complex_dims), Bcp_n."""
        self.dtype = dtype
        if weights is None:
            self.weights = torch.ones((rank_normal + rank_spectral), dtype=self.dtype, requires_grad=False,
                                      device=device)
        else:
            self.weights = torch.tensor(weights, dtype=self.dtype, requires_grad=False, device=device)
        self.softplus_kwargs = _fit.softplus_or_default(softplus_kwargs)
        self.rank_normal = rank_normal
        self.temporal_window = temporal_window
        self.idx_conv = self.get_idxConv(X_shape[0]).to(device)
        self.rank_spectral = rank_spectral
        self.rank = rank_normal + rank_spectral
        self.device = device
        self.non_negative = _fit.non_negative_flags(non_negative, len(X_shape) + len(y_shape[1:]))
        self.bias = torch.zeros(y_shape[1:], dtype=self.dtype, requires_grad=True, device=device)
        self.y_shape = y_shape
        B_dims = list(X_shape[1:]) + list(y_shape[1:])
        Bw_dims = [temporal_window]
        if Bcp_init is None:
            nn_w = [self.non_negative[0]]
            self.Bcp_w = make_BcpInit(Bw_dims, self.rank_normal, nn_w, complex_dims=None, scale=Bcp_init_scale,
                                      device=self.device, dtype=self.dtype) + \
                make_BcpInit(Bw_dims, self.rank_spectral, nn_w, complex_dims=spectral_complex_dims,
                             scale=Bcp_init_scale, device=self.device, dtype=self.dtype)
            self.Bcp_n = make_BcpInit(B_dims, self.rank, self.non_negative[1:], complex_dims=[1] * len(B_dims),
                                      scale=Bcp_init_scale, device=self.device, dtype=self.dtype)
            for A in self.Bcp_n + self.Bcp_w:
                A.requires_grad = True
        else:
            self.Bcp_n = Bcp_init[1]
            self.Bcp_w = Bcp_init[0]
        self.loss_running = []

    # ---- what a model may override ---------------------------------------------------------
    def _shape(self):
        """The plan constructor's leading arguments (W, D, N, Rn, Rs, C)."""
        Kn, Ks = self.Bcp_w
        C = int(Ks.shape[2]) if Ks.ndim == 3 else 1
        return (int(Kn.shape[0]), int(self.Bcp_n[0].shape[0]), int(self.Bcp_n[1].shape[0]), int(Kn.shape[1]),
                int(Ks.shape[1]), C)

    def _check_offered(self, X, verbose, process_group=None):
        if process_group is not None:
            raise NotImplementedError("process_group is not offered for the convolutional model")

    def _lambda_fit(self, lambda_L2):
        return _lambda3(lambda_L2, len(self.Bcp_n))

    def _lambda_adam(self, lambda_L2):
        return _lambda3(lambda_L2, len(self.Bcp_n))

    @staticmethod
    def _verbose_line(ii, loss, ratio):
        return f'Iter: {ii}, loss: {loss:.5}, var_ratio (y_hat/y_true): {ratio:.5}'

    # ---- plumbing --------------------------------------------------------------------------
    def _plan_for(self, X, dev, softplus_kwargs=_OWN):
        shape = self._shape()
        if int(X.shape[1]) != shape[1]:
            raise ValueError(f"X must be (T, {shape[1]}) for these factors; got {tuple(X.shape)}")
        if int(X.shape[0]) < shape[0]:
            raise ValueError(f"X has {X.shape[0]} rows, fewer than temporal_window = {shape[0]}")
        if softplus_kwargs is _OWN:
            softplus_kwargs = self.softplus_kwargs
        return _cached_plan(self._plan_cls, shape, int(X.shape[0]), self.non_negative, softplus_kwargs, dev)

    def _adam_plan_for(self, X, dev):
        return self._plan_for(X, dev, None) if self._default_softplus_in_adam else self._plan_for(X, dev)

    def _inputs(self, X, y):
        if self.dtype != torch.float32:
            raise NotImplementedError(f"the gfx950 kernels compute in fp32; this model has dtype={self.dtype}")
        dev = None if isinstance(X, torch.Tensor) and X.device.type == "cuda" else \
            _engine.device_index(self.device)
        X, dev = _series(X, dev)
        y = torch.as_tensor(y)
        N = int(self.Bcp_n[1].shape[0])
        if y.ndim != 2 or y.shape[0] != X.shape[0] or y.shape[1] != N:
            raise ValueError(f"y must be (T, n_out) = ({X.shape[0]}, {N}); got {tuple(y.shape)}")
        y = as_device_f32(y, dev)
        W = int(self.Bcp_w[0].shape[0])
        target = y[W // 2: y.shape[0] - W // 2]  # y[idx_conv]: a contiguous block of rows
        return X, y, target, dev

    def _parameters(self):
        """The torch leaves in arena order, the bias last."""
        return list(self.Bcp_n) + list(self.Bcp_w) + [self.bias]

    # ---- fitting -----------------------------------------------------------------------------
    def _fit_lbfgs(self, X, y, lambda_L2, max_iter, tol, patience, verbose, running_loss_logging_interval,
                   LBFGS_kwargs, penalties=None):
        """The LBFGS fit: torch.optim.LBFGS drives the parameters, every closure evaluation is one device
        pass with self.softplus_kwargs; logs the total loss.  `penalties`: _set_penalties' arguments
        after (plan, target), for the models that have it."""
        self._check_offered(X, verbose)
        _fit.require_lbfgs_kwargs(LBFGS_kwargs)
        lam = self._lambda_fit(lambda_L2)
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev)
        if penalties is not None:
            self._set_penalties(plan, target, *penalties)
        grad, gtot, loss_out = _fit.lbfgs_buffers(plan, dev)
        yhat = torch.empty_like(target)
        norm = float(target.numel())
        chatty = verbose in self._verbose_levels
        var_y = torch.var(y).item() if chatty else None
        params = self._parameters()

        def total_loss(with_grads=True):
            arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
            plan.loss_grad(X, target, None, norm, arena, None, grad, yhat=yhat)
            plan.finalize_grad(arena, grad, lam, gtot, loss_out)
            if with_grads:
                _fit.set_factor_grads(plan, gtot, params[:-1], self.bias)
            return loss_out[0].clone()

        def log_loss(ii):
            loss = total_loss(False).item()
            return loss, (self._verbose_line(ii, loss, torch.var(yhat).item() / var_y) if chatty else None)

        keep = (lambda optimizer: setattr(self, "optimizer", optimizer)) if self._keeps_optimizer else None
        return _fit.lbfgs_fit(params, LBFGS_kwargs, total_loss, log_loss, stop="length", max_iter=max_iter, tol=tol,
                              patience=patience, running_loss_logging_interval=running_loss_logging_interval,
                              verbose=verbose, loss_running=self.loss_running, on_optimizer=keep)

    def _fit_adam(self, X, y, lambda_L2, max_iter, tol, patience, verbose, Adam_kwargs, process_group,
                  penalties=None):
        """The Adam fit, device resident on gfx950 (`penalties` as in _fit_lbfgs)."""
        self._check_offered(X, verbose, process_group)
        hp = adam_hparams(Adam_kwargs)
        lam = self._lambda_adam(lambda_L2)
        X, y, target, dev = self._inputs(X, y)
        plan = self._adam_plan_for(X, dev)
        if penalties is not None:
            self._set_penalties(plan, target, *penalties)
        if self._keeps_optimizer:  # kept for inspection: the step itself runs on the device
            self.optimizer = torch.optim.Adam(self._parameters(), **Adam_kwargs)
        norm = float(target.numel())
        arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
        vcb = _fit.VerbosePrinter(self._verbose_line, y, _fit.yhat_from_loss_grad(plan, X, target, norm, None)) \
            if verbose in self._verbose_levels else None
        convergence_reached, _ = run_adam_fit(plan, X, target, None, norm, arena, None, lam, max_iter, tol, patience,
                                              hp, self.loss_running, verbose_cb=vcb)
        plan.unpack_into(arena, self.Bcp_w, self.Bcp_n, self.bias)
        return _fit.finish_fit(convergence_reached, verbose, nan_stopped=plan.last_stop < 0)

    ####################################
    ############ POST-HOC ##############
    ####################################

    def predict(self, X, Bcp=None, device=None, plot_pref=False):
        """y_hat of the model's own factors (the Bcp argument is ignored, as in the reference) with the
        softplus parameters fit_Adam uses, as a detached CPU tensor (T - W + 1, n_out)."""
        if device is None:
            device = self.device
        dev = None if isinstance(X, torch.Tensor) and X.device.type == "cuda" else _engine.device_index(device)
        Xd, dev = _series(X, dev)
        plan = self._adam_plan_for(Xd, dev)
        arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
        return plan.forward(Xd, arena).cpu().detach()

    def get_idxConv(self, input_length):
        return torch.arange(self.temporal_window // 2, input_length - self.temporal_window // 2)

    def return_Bcp_final(self):
        """softplus-applied (Bcp_n, Bcp_w) as numpy lists, with self.softplus_kwargs."""
        Bcp_n = list(non_neg_fn(self.Bcp_n, self.non_negative[1:], softplus_kwargs=self.softplus_kwargs))
        Bcp_w = list(non_neg_fn(self.Bcp_w, [self.non_negative[0]] * 2, softplus_kwargs=self.softplus_kwargs))
        return [A.detach().cpu().numpy() for A in Bcp_n], [A.detach().cpu().numpy() for A in Bcp_w]

    def display_params(self):
        print('weights:', self.weights)
        print('Bcp:', getattr(self, 'Bcp', None))
        print('non_negative:', self.non_negative)
        print('softplus_kwargs:', self.softplus_kwargs)
        print('rank:', self.rank)
        print('device:', self.device)
        print('loss_running:', self.loss_running)

    def plot_outputs(self):
        plt = _fit.plot_loss(self.loss_running)
        Bcp_n_final, Bcp_w_final = self.return_Bcp_final()
        fig, axs = plt.subplots(len(Bcp_n_final) + len(Bcp_w_final))
        for ii, val in enumerate(Bcp_n_final + Bcp_w_final):
            axs[ii].plot(val.reshape(val.shape[0], -1))
        fig.suptitle('Bcp_n and Bcp_w components')


class SmoothConvModel(ConvModelBase):
    """The phase and Fourier models: smoothness arguments in both fits, self.softplus_kwargs everywhere,
    a scalar lambda_L2 accepted by both fits, `self.optimizer`, `y_spectrum`, get_params / set_params."""
    _keeps_optimizer = True

    def _init_spectrum(self, X_shape, do_spectralPenalty, spectrum_smoothing_factor):
        self.X_shape = X_shape
        self.do_spectralPenalty = do_spectralPenalty
        half = spectrum_smoothing_factor // 2
        self.spectral_smoothing_kernel = torch.tensor(
            gaussian(np.arange(-half, half + 1), 0, spectrum_smoothing_factor / 7)[0],
            dtype=self.dtype, requires_grad=False, device=self.device)

    def _set_penalties(self, plan, target, lambda_spectralPenalty, lambda_smooth, smooth_diff_order):
        plan.set_smoothness(lambda_smooth, smooth_diff_order)
        self.y_spectrum = None

    def fit(self, X, y, lambda_L2=0.01, lambda_spectralPenalty=0.01, lambda_smooth=0.01, smooth_diff_order=2,
            max_iter=1000, tol=1e-5, patience=10, verbose=False, running_loss_logging_interval=10,
            LBFGS_kwargs=None):
        """LBFGS fit: torch.optim.LBFGS (kept as self.optimizer) drives the parameters, every closure
        evaluation is one device pass; logs the total loss."""
        return self._fit_lbfgs(X, y, lambda_L2, max_iter, tol, patience, verbose, running_loss_logging_interval,
                               LBFGS_kwargs, (lambda_spectralPenalty, lambda_smooth, smooth_diff_order))

    def fit_Adam(self, X, y, lambda_L2=0.01, lambda_spectralPenalty=0.01, lambda_smooth=0.01, smooth_diff_order=2,
                 max_iter=1000, tol=1e-5, patience=10, verbose=False, plotting_interval=100, Adam_kwargs=None,
                 process_group=None):
        """Adam fit, device resident on gfx950, with self.softplus_kwargs; a scalar lambda_L2 is accepted."""
        return self._fit_adam(X, y, lambda_L2, max_iter, tol, patience, verbose, Adam_kwargs, process_group,
                              (lambda_spectralPenalty, lambda_smooth, smooth_diff_order))

    def predict(self, X, Bcp=None, device=None, plot_pref=False):
        """forward_model with the model's own factors (the Bcp argument is ignored, as in the reference)
        and self.softplus_kwargs, as a detached CPU tensor (T - W + 1, n_out)."""
        if type(X).__name__ == "HostStream":
            raise NotImplementedError("HostStream is not offered for the convolutional model")
        return super().predict(X, Bcp, device, plot_pref)

    def detach_Bcp(self):
        """The raw (Bcp_n, Bcp_w) as numpy lists."""
        return ([A.detach().cpu().numpy() for A in self.Bcp_n], [A.detach().cpu().numpy() for A in self.Bcp_w])

    def get_params(self):
        """The model's state as a dict."""
        return {
            'X_shape': self.X_shape,
            'y_shape': self.y_shape,
            'dtype': self.dtype,
            'device': self.device,
            'weights': self.weights.detach().cpu().numpy(),
            'Bcp_n': [A.detach().cpu().numpy() for A in self.Bcp_n],
            'Bcp_w': [A.detach().cpu().numpy() for A in self.Bcp_w],
            'bias': self.bias.detach().cpu().numpy(),
            'non_negative': self.non_negative,
            'softplus_kwargs': self.softplus_kwargs,
            'rank': self.rank,
            'rank_normal': self.rank_normal,
            'rank_spectral': self.rank_spectral,
            'idxConv': self.idx_conv.detach().cpu().numpy(),
            'spectral_smoothing_kernel': self.spectral_smoothing_kernel.detach().cpu().numpy(),
            'temporal_window': self.temporal_window,
            'do_spectralPenalty': self.do_spectralPenalty,
            'loss_running': self.loss_running,
        }

    def set_params(self, params):
        """Restore get_params' dict (idx_conv comes back in self.dtype, as in the reference)."""
        self.X_shape = params['X_shape']
        self.y_shape = params['y_shape']
        self.dtype = params['dtype']
        self.device = params['device']
        self.weights = torch.as_tensor(params['weights'], dtype=self.dtype).to(self.device)
        self.Bcp_n = [torch.as_tensor(A, dtype=self.dtype).to(self.device) for A in params['Bcp_n']]
        self.Bcp_w = [torch.as_tensor(A, dtype=self.dtype).to(self.device) for A in params['Bcp_w']]
        self.bias = torch.as_tensor(params['bias'], dtype=self.dtype).to(self.device)
        self.non_negative = params['non_negative']
        self.softplus_kwargs = params['softplus_kwargs']
        self.rank = params['rank']
        self.rank_normal = params['rank_normal']
        self.rank_spectral = params['rank_spectral']
        self.idx_conv = torch.as_tensor(params['idxConv'], dtype=self.dtype).to(self.device)
        self.spectral_smoothing_kernel = torch.as_tensor(params['spectral_smoothing_kernel'],
                                                         dtype=self.dtype).to(self.device)
        self.temporal_window = params['temporal_window']
        self.do_spectralPenalty = params['do_spectralPenalty']
        self.loss_running = params['loss_running']
