"""Convolutional Fourier CP regression on MI355X — drop-in for the reference's
`convolutional_fourier_tensor_regression.py` (kimerein/tensor_regression).

The convolutional model of `convolutional_spectral_tensor_regression` (unconstrained spectral kernels
Ks (W, Rs, C), magnitude over the C = n_complex_dim + 1 components) with two penalties:

  * the smoothness penalty lambda_smooth * mean((Delta^q F)^2) on the raw temporal kernels Kn and Ks
    (for Ks the mean runs over all (W + q) Rs C entries);
  * with do_spectralPenalty=True, the output-spectrum penalty

        Y = rfft(y_hat, n = T) (y_hat zero-padded from T - W + 1 rows),  A = |Y|,
        M = A smoothed along frequency with the gaussian `spectral_smoothing_kernel` (valid, no flip),
        pen = lambda_spectralPenalty * mean(((M - M_y) / (M_y + 1e-8))^2),   M_y the same of y[idx_conv]

    T being the constructor's y_shape[0].

    loss = MSE + l0 (||Kn|| + ||Ks||) + l1 ||Bd|| + l2 ||Bo|| + pen + smoothness(Kn) + smoothness(Ks)

Same module functions and `CP_linear_regression` class as the reference (arguments, RNG draws and
their order, Bcp_w = [Kn (W, Rn), Ks (W, Rs, C)], Bcp_n = [Bd (D, R), Bo (N, R)], `loss_running`,
`y_spectrum`), with fit / fit_Adam / predict on the gfx950 kernels: csrc/tr_conv.hip for the X pass,
csrc/tr_conv_spectrum.hip for the spectrum path (a direct real DFT of any length with exact integer
angle indices, its adjoint, and the terms between them) and for the update step.  Envelope: the conv
module's (W odd <= 257, D <= 65536, n_out <= 64, Rn + Rs <= 32, C <= 4, Rn + Rs C <= 64), a
smoothing kernel of at most 4097 taps, T <= 2^22; outside it the plan raises ValueError.

Deliberate differences from the reference:
  * an even temporal_window or a 1-D y raises ValueError at construction (the reference fails later,
    inside the first fit);
  * dtype=float64, `HostStream`, `process_group` and verbose == 3 (live plots) raise NotImplementedError;
  * rank_normal == 1 with rank_spectral > 0, and n_complex_dim == 0 with rank_spectral > 0, raise
    ValueError at construction: the reference's own forward_model fails there in torch.cat (it
    squeezes a single normal rank away; a Ks without a component axis gives a block of another
    rank of dimensions, and without normal ranks a norm over the spectral ranks);
  * a smoothing kernel longer than the T // 2 + 1 bins raises ValueError from fit / fit_Adam before any
    device work (the reference fails in conv1d), and so does an X with more than T + W - 1 rows (the
    reference's rfft would truncate y_hat to T rows).
"""
import numpy as np
import torch

from . import _engine
from ._engine import ConvFourierPlan, adam_hparams, as_device_f32, run_adam_fit
from .convolutional_spectral_tensor_regression import (L2_penalty, _series, complex_magnitude, make_BcpInit,
                                                       non_neg_fn, stepwise_linear_model_multirank)
from .phase_constrained_spectral_convolutional_tensor_regression import (_lambda3, conv, diff_highOrder, gaussian,
                                                                         smoothness_penalty)

__all__ = ["make_BcpInit", "non_neg_fn", "gaussian", "conv", "complex_magnitude", "stepwise_linear_model_multirank",
           "forward_model", "spectral_penalty", "L2_penalty", "diff_highOrder", "smoothness_penalty",
           "CP_linear_regression"]


####################################
######## Helper functions ##########
####################################

def forward_model(X, kernel, Bcp, weights, non_negative, bias, softplus_kwargs=None):
    """y_hat (T - W + 1, n_out) of the Fourier model (…py:694-725) as a torch expression in the dtype
    and on the device of its inputs: the host-side restatement (the fits and predict run the gfx950
    kernels).  kernel = [Kn (W, Rn), Ks (W, Rs, C)], Bcp = [Bd, Bo] (raw factors); `weights` is unused,
    as in the reference."""
    kernel_nn = list(non_neg_fn(kernel, [non_negative[0]] * 2, softplus_kwargs))
    Bcp_nn = list(non_neg_fn(Bcp, non_negative[1:], softplus_kwargs))
    parts = []
    if kernel_nn[0].ndim > 1 and kernel_nn[0].shape[1] > 0:
        parts.append(conv(X, kernel_nn[0]))
    if kernel_nn[1].ndim > 1 and kernel_nn[1].shape[1] > 0:
        Ks = kernel_nn[1] if kernel_nn[1].ndim == 3 else kernel_nn[1][..., None]
        parts.append(complex_magnitude(conv(X, Ks)))
    return stepwise_linear_model_multirank(torch.cat(parts, dim=-1), Bcp_nn, weights, bias)


def spectral_penalty(y_pred, y_true=None, y_true_fft=None, n_fft=None, smoothing_kernel=None, passthrough=False,
                     lam=0, plot_pref=False):
    """lam * mean(((M - M_y) / (M_y + 1e-8))^2) with M = conv(|rfft(y_pred, n=n_fft, dim=0)|,
    smoothing_kernel) (…py:727-812) as a torch expression; M_y = y_true_fft, or |rfft(y_true)| when
    y_true is given (unsmoothed, as in the reference).  The fits compute this on the device."""
    if passthrough:
        return torch.tensor(0.)
    if y_true is not None:
        y_true_fft = torch.abs(torch.fft.rfft(y_true, dim=0))
    assert y_true_fft is not None, "y_true_fft is None"
    y_pred_fft = conv(torch.abs(torch.fft.rfft(y_pred, dim=0, n=n_fft)), smoothing_kernel)
    mse = torch.mean(((y_pred_fft - y_true_fft) / (y_true_fft + 1e-8)) ** 2)
    if plot_pref:
        import matplotlib.pyplot as plt
        plt.figure()
        plt.plot(y_true_fft[:, 0].cpu().detach().numpy(), label='true')
        plt.plot(y_pred_fft[:, 0].cpu().detach().numpy(), label='pred')
        plt.xlabel('smooth')
    return mse * lam


_plan_cache = {}


def _cached_plan(W, D, N, Rn, Rs, C, rows, non_negative, softplus_kwargs, dev):
    beta, thr = _engine.softplus_params(softplus_kwargs)
    key = (W, D, N, Rn, Rs, C, tuple(bool(non_negative[f]) for f in range(3)), beta, thr, dev)
    p = _plan_cache.get(key)
    if p is None or p.max_rows < rows:
        p = ConvFourierPlan(W, D, N, Rn, Rs, C, rows, non_negative, softplus_kwargs, f"cuda:{dev}")
        _plan_cache[key] = p
    return p


class _VerbosePrinter:
    """verbose == 2 per-iteration print (…py:1287-1308; the total and the variance ratio)."""

    def __init__(self, plan, X, target, y, norm):
        self.plan, self.X, self.t, self.norm = plan, X, target, norm
        self.var_y = torch.var(y).item()
        self.grad = torch.zeros(plan.num_grads, dtype=torch.float32, device=X.device)
        self.yhat = torch.empty_like(target)

    def before_step(self, arena):
        self.plan.loss_grad(self.X, self.t, None, self.norm, arena, None, self.grad, yhat=self.yhat)

    def after_step(self, ii, loss):
        ratio = torch.var(self.yhat).item() / self.var_y
        print(f'Iter: {ii}, loss: {loss:.5}, var_ratio (y_hat/y_true): {ratio:.5}')


####################################
########### Main class #############
####################################

class CP_linear_regression():
    def __init__(self,
                 X_shape,
                 y_shape,
                 dtype=torch.float32,
                 rank_normal=1,
                 temporal_window=5,
                 rank_spectral=1,
                 non_negative=False,
                 weights=None,
                 Bcp_init=None,
                 Bcp_init_scale=1,
                 n_complex_dim=0,
                 bias_init=0,
                 device='cpu',
                 do_spectralPenalty=False,
                 spectrum_smoothing_factor=100,
                 softplus_kwargs=None):
        """Convolutional Fourier CP regression (…py:909-1050; same arguments and attributes;
        `bias_init` is accepted and unused, as in the reference).  RNG draws in the reference's order:
        Bcp_w normal ranks, Bcp_w spectral ranks, then Bcp_n."""
        if int(temporal_window) % 2 == 0 or int(temporal_window) < 1:
            raise ValueError(f"temporal_window must be odd and >= 1 (got {temporal_window}): with an even window "
                             "the reference's y_hat (T - W + 1 rows) and y[idx_conv] (T - W rows) never match")
        if len(y_shape) < 2:
            raise ValueError("y must be 2-D (T, n_out); the reference's model breaks at the first fit on a 1-D y")
        if dtype == torch.float64:
            raise NotImplementedError("the gfx950 conv kernel computes in fp32; fp64 is not offered")
        if Bcp_init is None and rank_spectral > 0 and rank_normal == 1:
            raise ValueError("rank_normal == 1 with rank_spectral > 0: the reference's own forward_model fails there "
                             "(it squeezes the single normal rank away before torch.cat)")
        if Bcp_init is None and rank_spectral > 0 and n_complex_dim == 0:
            raise ValueError("n_complex_dim == 0 with rank_spectral > 0: the reference's own forward_model fails "
                             "there (torch.cat of a 3-D and a 2-D block; a norm over the ranks without normal ranks)")
        self.dtype = dtype
        if weights is None:
            self.weights = torch.ones((rank_normal + rank_spectral), dtype=self.dtype, requires_grad=False,
                                      device=device)
        else:
            self.weights = torch.tensor(weights, dtype=self.dtype, requires_grad=False, device=device)
        self.softplus_kwargs = {'beta': 50, 'threshold': 1} if softplus_kwargs is None else softplus_kwargs
        self.X_shape = X_shape
        self.y_shape = y_shape
        self.rank_normal = rank_normal
        self.temporal_window = temporal_window
        self.idx_conv = self.get_idxConv(X_shape[0]).to(device)
        self.rank_spectral = rank_spectral
        self.rank = rank_normal + rank_spectral
        self.device = device
        n_flags = len(X_shape) + len(y_shape[1:])
        if non_negative is True:
            self.non_negative = [True] * n_flags
        elif non_negative is False:
            self.non_negative = [False] * n_flags
        else:
            self.non_negative = non_negative
        self.bias = torch.zeros(y_shape[1:], dtype=self.dtype, requires_grad=True, device=device)
        B_dims = list(X_shape[1:]) + list(y_shape[1:])
        Bw_dims = [temporal_window]
        if Bcp_init is None:
            nn_w = [self.non_negative[0]]
            self.Bcp_w = make_BcpInit(Bw_dims, self.rank_normal, nn_w, complex_dims=None, scale=Bcp_init_scale,
                                      device=self.device, dtype=self.dtype) + \
                make_BcpInit(Bw_dims, self.rank_spectral, nn_w, complex_dims=[n_complex_dim + 1],
                             scale=Bcp_init_scale, device=self.device, dtype=self.dtype)
            self.Bcp_n = make_BcpInit(B_dims, self.rank, self.non_negative[1:], complex_dims=[1] * len(B_dims),
                                      scale=Bcp_init_scale, device=self.device, dtype=self.dtype)
            for A in self.Bcp_n + self.Bcp_w:
                A.requires_grad = True
        else:
            self.Bcp_n = Bcp_init[1]
            self.Bcp_w = Bcp_init[0]
        self.do_spectralPenalty = do_spectralPenalty
        half = spectrum_smoothing_factor // 2
        self.spectral_smoothing_kernel = torch.tensor(
            gaussian(np.arange(-half, half + 1), 0, spectrum_smoothing_factor / 7)[0],
            dtype=self.dtype, requires_grad=False, device=self.device)
        self.loss_running = []

    # ---- plumbing --------------------------------------------------------------------------
    def _shape(self):
        Kn, Ks = self.Bcp_w
        C = int(Ks.shape[2]) if Ks.ndim == 3 else 1
        return (int(Kn.shape[0]), int(self.Bcp_n[0].shape[0]), int(self.Bcp_n[1].shape[0]), int(Kn.shape[1]),
                int(Ks.shape[1]), C)

    def _plan_for(self, X, dev):
        W, D, N, Rn, Rs, C = self._shape()
        if int(X.shape[1]) != D:
            raise ValueError(f"X must be (T, {D}) for these factors; got {tuple(X.shape)}")
        if int(X.shape[0]) < W:
            raise ValueError(f"X has {X.shape[0]} rows, fewer than temporal_window = {W}")
        return _cached_plan(W, D, N, Rn, Rs, C, int(X.shape[0]), self.non_negative, self.softplus_kwargs, dev)

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

    def _check_offered(self, X, verbose, process_group=None):
        if type(X).__name__ == "HostStream":
            raise NotImplementedError("HostStream is not offered for the convolutional model")
        if process_group is not None:
            raise NotImplementedError("process_group is not offered for the convolutional model")
        if verbose == 3:
            raise NotImplementedError("verbose == 3 (live plots) is not offered")
        if self.do_spectralPenalty:
            n_fft, S = int(self.y_shape[0]), int(self.spectral_smoothing_kernel.numel())
            if n_fft // 2 + 1 < S:
                raise ValueError(f"the spectrum of n = {n_fft} has {n_fft // 2 + 1} bins, fewer than the "
                                 f"{S} taps of spectral_smoothing_kernel")
            W = int(self.Bcp_w[0].shape[0])
            if hasattr(X, "shape") and int(X.shape[0]) - W + 1 > n_fft:
                raise ValueError(f"X has {X.shape[0]} rows: y_hat would be longer than n_fft = y_shape[0] = {n_fft}")

    def _set_penalties(self, plan, target, lambda_spectralPenalty, lambda_smooth, smooth_diff_order):
        plan.set_smoothness(lambda_smooth, smooth_diff_order)
        if self.do_spectralPenalty:
            plan.set_spectrum_penalty(lambda_spectralPenalty, self.spectral_smoothing_kernel.detach().cpu().numpy(),
                                      int(self.y_shape[0]), target)
            self.y_spectrum = plan.conv_spectrum(target)
        else:
            plan.set_spectrum_penalty(0.0, None, 0, None)
            self.y_spectrum = None

    def _set_grads(self, plan, gtot):
        o = plan.offsets
        for f, A in enumerate(list(self.Bcp_n) + list(self.Bcp_w)):
            A.grad = gtot[o[f]:o[f + 1]].to(A.device).clone().view(A.shape)
        self.bias.grad = gtot[o[4]:].to(self.bias.device).clone().view(self.bias.shape)

    # ---- fitting -----------------------------------------------------------------------------
    def fit(self, X, y, lambda_L2=0.01, lambda_spectralPenalty=0.01, lambda_smooth=0.01, smooth_diff_order=2,
            max_iter=1000, tol=1e-5, patience=10, verbose=False, running_loss_logging_interval=10,
            LBFGS_kwargs=None):
        """LBFGS fit (…py:1052-1194): torch.optim.LBFGS (kept as self.optimizer) drives the parameters,
        every closure evaluation is one device pass; logs the total loss."""
        self._check_offered(X, verbose)
        if LBFGS_kwargs is None:
            raise TypeError("torch.optim.lbfgs.LBFGS() argument after ** must be a mapping, not NoneType")
        lam = _lambda3(lambda_L2, len(self.Bcp_n))
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev)
        self._set_penalties(plan, target, lambda_spectralPenalty, lambda_smooth, smooth_diff_order)
        self.optimizer = torch.optim.LBFGS(list(self.Bcp_n) + list(self.Bcp_w) + [self.bias], **LBFGS_kwargs)
        opts = dict(dtype=torch.float32, device=f"cuda:{dev}")
        grad = torch.zeros(plan.num_grads, **opts)
        gtot = torch.zeros(plan.num_params, **opts)
        loss_out = torch.zeros(1, **opts)
        yhat = torch.empty_like(target)
        norm = float(target.numel())
        var_y = torch.var(y).item() if verbose == 2 else None

        def total_loss(with_grads):
            arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
            plan.loss_grad(X, target, None, norm, arena, None, grad, yhat=yhat)
            plan.finalize_grad(arena, grad, lam, gtot, loss_out)
            if with_grads:
                self._set_grads(plan, gtot)
            return loss_out[0].clone()

        def closure():
            self.optimizer.zero_grad()
            return total_loss(True)

        convergence_reached = False
        for ii in range(max_iter):
            if ii % running_loss_logging_interval == 0:
                self.loss_running.append(total_loss(False).item())
                if verbose == 2:
                    print(f'Iter: {ii}, loss: {self.loss_running[-1]:.5}, var_ratio (y_hat/y_true): '
                          f'{torch.var(yhat).item() / var_y:.5}')
            if len(self.loss_running) > patience:
                if np.sum(np.abs(np.diff(self.loss_running[-patience + 1:]))) < tol:
                    convergence_reached = True
                    break
            elif np.isnan(self.loss_running[-1]):
                convergence_reached = False
                print('Loss is NaN. Stopping.')
                break
            self.optimizer.step(closure)
        if (verbose is True) or (verbose >= 1):
            print('Convergence reached' if convergence_reached else
                  'Reached maximum number of iterations without convergence')
        return convergence_reached

    def fit_Adam(self, X, y, lambda_L2=0.01, lambda_spectralPenalty=0.01, lambda_smooth=0.01, smooth_diff_order=2,
                 max_iter=1000, tol=1e-5, patience=10, verbose=False, plotting_interval=100, Adam_kwargs=None,
                 process_group=None):
        """Adam fit (…py:1197-1327), device resident on gfx950."""
        self._check_offered(X, verbose, process_group)
        hp = adam_hparams(Adam_kwargs)
        lam = _lambda3(lambda_L2, len(self.Bcp_n))
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev)
        self._set_penalties(plan, target, lambda_spectralPenalty, lambda_smooth, smooth_diff_order)
        self.optimizer = torch.optim.Adam(list(self.Bcp_n) + list(self.Bcp_w) + [self.bias], **Adam_kwargs)
        norm = float(target.numel())
        arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
        vcb = _VerbosePrinter(plan, X, target, y, norm) if verbose == 2 else None
        convergence_reached, _ = run_adam_fit(plan, X, target, None, norm, arena, None, lam, max_iter, tol, patience,
                                              hp, self.loss_running, verbose_cb=vcb)
        plan.unpack_into(arena, self.Bcp_w, self.Bcp_n, self.bias)
        if plan.last_stop < 0:
            print('Loss is NaN. Stopping.')
        if (verbose is True) or (verbose >= 1):
            print('Convergence reached' if convergence_reached else
                  'Reached maximum number of iterations without convergence')
        return convergence_reached

    ####################################
    ############ POST-HOC ##############
    ####################################

    def predict(self, X, Bcp=None, device=None, plot_pref=False):
        """forward_model with the model's own factors (the Bcp argument is ignored, …py:1543) and
        self.softplus_kwargs, as a detached CPU tensor (T - W + 1, n_out)."""
        if device is None:
            device = self.device
        if type(X).__name__ == "HostStream":
            raise NotImplementedError("HostStream is not offered for the convolutional model")
        dev = None if isinstance(X, torch.Tensor) and X.device.type == "cuda" else _engine.device_index(device)
        Xd, dev = _series(X, dev)
        plan = self._plan_for(Xd, dev)
        arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
        return plan.forward(Xd, arena).cpu().detach()

    def get_idxConv(self, input_length):
        return torch.arange(self.temporal_window // 2, input_length - self.temporal_window // 2)

    def return_Bcp_final(self):
        """softplus-applied (Bcp_n, Bcp_w) as numpy lists, with self.softplus_kwargs (…py:1636-1651)."""
        Bcp_n = list(non_neg_fn(self.Bcp_n, self.non_negative[1:], softplus_kwargs=self.softplus_kwargs))
        Bcp_w = list(non_neg_fn(self.Bcp_w, [self.non_negative[0]] * 2, softplus_kwargs=self.softplus_kwargs))
        return [A.detach().cpu().numpy() for A in Bcp_n], [A.detach().cpu().numpy() for A in Bcp_w]

    def detach_Bcp(self):
        """The raw (Bcp_n, Bcp_w) as numpy lists (…py:1653-1664)."""
        return ([A.detach().cpu().numpy() for A in self.Bcp_n], [A.detach().cpu().numpy() for A in self.Bcp_w])

    def get_params(self):
        """The model's state as a dict (…py:1666-1690)."""
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
        """Restore get_params' dict (…py:1692-1714; idx_conv comes back in self.dtype, as there)."""
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

    def display_params(self):
        print('weights:', self.weights)
        print('Bcp:', getattr(self, 'Bcp', None))
        print('non_negative:', self.non_negative)
        print('softplus_kwargs:', self.softplus_kwargs)
        print('rank:', self.rank)
        print('device:', self.device)
        print('loss_running:', self.loss_running)

    def plot_outputs(self):
        import matplotlib.pyplot as plt
        plt.figure()
        plt.plot(self.loss_running)
        plt.xlabel('logged iteration')
        plt.ylabel('loss')
        plt.title('loss')
        Bcp_n_final, Bcp_w_final = self.return_Bcp_final()
        fig, axs = plt.subplots(len(Bcp_n_final) + len(Bcp_w_final))
        for ii, val in enumerate(Bcp_n_final + Bcp_w_final):
            axs[ii].plot(val.reshape(val.shape[0], -1))
        fig.suptitle('Bcp_n and Bcp_w components')
