"""Phase-constrained spectral convolutional CP regression on MI355X — drop-in for the reference's
`phase_constrained_spectral_convolutional_tensor_regression.py` (kimerein/tensor_regression).

The convolutional model of `convolutional_spectral_tensor_regression` with two additions:

  * a spectral rank carries ONE temporal kernel k (W taps); its second component is derived, k with
    every frequency shifted by 90 degrees (`phase_shifter`), so ||(X*k, X*Hk)|| is an envelope
    detector by construction;
  * a smoothness penalty lambda_smooth * mean((Delta^q F)^2) on the raw temporal kernels.

    z_n[t,d,r] = sum_w X[t+w,d] phi(Kn)[w,r]                                  (normal ranks, signed)
    z0 = X * phi(Ks),  z1 = X * H phi(Ks),  u_s = sqrt(z0^2 + z1^2)           (spectral ranks)
    y_hat      = (sum_d u * phi(Bd)) . phi(Bo)^T + bias      compared with y[idx_conv]
    loss       = MSE + l0 (||Kn|| + ||Ks||) + l1 ||Bd|| + l2 ||Bo|| + smoothness(Kn) + smoothness(Ks)

`phase_shifter` is computed as the fixed real linear map it is: circular convolution with
h[d] = (2 / W) sum_{j=1..ceil(W/2)-1} sin(2 pi j d / W) (H^T = -H), times sin(angle), plus cos(angle)
times the signal.  The reference's fp32 mask shifts by fp32(pi/2), whose cosine is -4.4e-8; here
the angle is exact.

Same module functions and `CP_linear_regression` class as the reference (arguments, RNG draws and
their order, Bcp_w = [Kn (W, Rn), Ks (W, Rs)], Bcp_n = [Bd (D, R), Bo (N, R)], `loss_running`), with
fit / fit_Adam / predict on the gfx950 kernels (csrc/tr_conv.hip for the X pass, csrc/tr_conv_phase.hip
for the constraint, its adjoint and the smoothness term).  Envelope: W odd <= 257, D <= 65536,
n_out <= 64, 1 <= Rn + Rs <= 32; outside it the plan raises ValueError.

What this reference file does, unlike the conv module's: fit, fit_Adam and predict all use
self.softplus_kwargs; a scalar (or length-1 list) lambda_L2 is accepted by both fits; both fits keep
`self.optimizer` (fit_Adam's is a torch.optim.Adam over the parameters, kept for inspection: the
step itself runs on the device).

Choices mirrored from the conv module: an even temporal_window, a 1-D y and dtype=float64 raise at
construction (the reference fails later, inside the first fit); tensors run on a HIP device in
fp32; `process_group` and `HostStream` raise NotImplementedError.

Out of scope: `do_spectralPenalty=True` is stored and round-trips through get_params / set_params,
and fit / fit_Adam then raise NotImplementedError before touching the device (the output-spectrum
penalty needs |rfft(y_hat, n=T)| of arbitrary length and a forward / backward split of the X pass);
the verbose == 3 live plots are not offered (verbose 3 prints like verbose 2).
"""
import numpy as np
import torch

from . import _engine
from ._engine import ConvPhasePlan, adam_hparams, as_device_f32, run_adam_fit
from .convolutional_spectral_tensor_regression import (L2_penalty, _series, make_BcpInit, non_neg_fn,
                                                       stepwise_linear_model_multirank)
from .convolutional_spectral_tensor_regression import conv as _conv_unfold

__all__ = ["make_BcpInit", "non_neg_fn", "gaussian", "conv", "stepwise_linear_model_multirank", "forward_model",
           "L2_penalty", "diff_highOrder", "smoothness_penalty", "phase_shifter", "CP_linear_regression"]


####################################
######## Helper functions ##########
####################################

def gaussian(x, mu, sig, plot_pref=False):
    """Normalised gaussian of x and its parameters (…py:101-131)."""
    gaus = 1 / (np.sqrt(2 * np.pi) * sig) * np.exp(-np.power((x - mu) / sig, 2) / 2)
    if plot_pref:
        import matplotlib.pyplot as plt
        plt.figure()
        plt.plot(x, gaus)
        plt.xlabel('x')
    return gaus, {"x": x, "mu": mu, "sig": sig}


def conv(X, kernels, **conv1d_kwargs):
    """Valid cross-correlation along dim 0 (…py:291-334): X (T, D), kernels (W,) / (W, R) / (W, R, C) ->
    (T - W + 1, D) + kernels.shape[1:].  A torch expression on X's device: the reference's inspection
    helper (the fit path fuses it into the kernel); conv1d keyword arguments are not offered."""
    if conv1d_kwargs:
        raise NotImplementedError("conv1d keyword arguments (padding, stride) are not offered")
    k3 = kernels.reshape(kernels.shape[0], -1, 1)
    out = _conv_unfold(X, k3)[..., 0]  # (T', D, prod(kernels.shape[1:]))
    return out.reshape(tuple(out.shape[:2]) + tuple(kernels.shape[1:]))


def diff_highOrder(traces, order):
    """`order` rounds of a first difference along dim 0, one zero row prepended and appended each
    round (…py:933-937): (W, ...) -> (W + order, ...)."""
    buffer = torch.zeros(traces.shape[1:], device=traces.device, dtype=traces.dtype).unsqueeze(0)
    for _ in range(order):
        traces = torch.diff(traces, dim=0, prepend=buffer, append=buffer)
    return traces


def smoothness_penalty(Bcp_w, derivative_order=2, lambda_smooth=1):
    """sum over the non-empty factors of mean(diff_highOrder(F)^2) * lambda_smooth (…py:938-956)."""
    penalty = 0
    for comp in Bcp_w:
        if comp.numel() > 0:
            penalty += torch.mean(diff_highOrder(comp, order=derivative_order) ** 2) * lambda_smooth
    return penalty


def quadrature_filter(signal_len, dtype=torch.float64):
    """h of the module docstring, (signal_len,), computed in fp64."""
    W = int(signal_len)
    d = torch.arange(W, dtype=torch.float64)
    j = torch.arange(1, (W + 1) // 2, dtype=torch.float64)
    h = (2.0 / W) * torch.sin(2.0 * np.pi * j[None, :] * d[:, None] / W).sum(dim=1)
    return h.to(dtype)


def quadrature_matrix(signal_len, dtype=torch.float64):
    """H (W, W) with H[n, m] = h[(n - m) mod W]: the 90-degree shift of every frequency."""
    W = int(signal_len)
    h = quadrature_filter(W)
    n = torch.arange(W)
    return h[(n[:, None] - n[None, :]) % W].to(dtype)


class phase_shifter():
    def __init__(self, signal_len, discard_imaginary_component=True, device='cpu', dtype=torch.float32,
                 pin_memory=False):
        """Shifts every frequency of a signal by an angle (…py:959-1027; same constructor and
        attributes).  The call computes real(ifft(fft(x) * exp(i * angle_mask * angle))) as the linear
        map cos(angle) * x + sin(angle) * H x."""
        self.signal_len = signal_len
        n = int(signal_len)
        self.angle_mask = torch.cat([-torch.ones((n + 1) // 2, dtype=dtype, device=device, pin_memory=pin_memory),
                                     torch.ones(n // 2, dtype=dtype, device=device, pin_memory=pin_memory)])
        self.discard_imaginary_component = discard_imaginary_component
        self._H = quadrature_matrix(n)

    def __call__(self, signal, shift_angle=90, deg_or_rad='deg', dim=0):
        if shift_angle == 0:
            return signal
        if not self.discard_imaginary_component:
            raise NotImplementedError("the complex-valued shift (discard_imaginary_component=False) is not offered")
        angle = np.deg2rad(shift_angle) if deg_or_rad == 'deg' else shift_angle
        c = 0.0 if shift_angle == 90 and deg_or_rad == 'deg' else float(np.cos(angle))
        s = 1.0 if shift_angle == 90 and deg_or_rad == 'deg' else float(np.sin(angle))
        H = self._H.to(device=signal.device, dtype=signal.dtype)
        x = signal.movedim(dim, 0)
        out = s * torch.tensordot(H, x, dims=([1], [0]))
        if c != 0.0:
            out = out + c * x
        return out.movedim(0, dim)


def forward_model(X, kernel, shifter, Bcp, weights, non_negative, bias, softplus_kwargs=None):
    """y_hat (T - W + 1, n_out) of the phase-constrained model (…py:696-744) as a torch expression in
    the dtype and on the device of its inputs: the host-side restatement (the fits and predict run the
    gfx950 kernels).  kernel = [Kn, Ks], Bcp = [Bd, Bo] (raw factors); `weights` is unused, as in the
    reference."""
    kernel_nn = list(non_neg_fn(kernel, [non_negative[0]] * 2, softplus_kwargs))
    Bcp_nn = list(non_neg_fn(Bcp, non_negative[1:], softplus_kwargs))
    parts = []
    if kernel_nn[0].ndim > 1 and kernel_nn[0].shape[1] > 0:
        parts.append(conv(X, kernel_nn[0]))
    if kernel_nn[1].ndim > 1 and kernel_nn[1].shape[1] > 0:
        z = torch.stack([conv(X, shifter(kernel_nn[1], shift_angle=a, deg_or_rad='deg', dim=0)) for a in (0, 90)],
                        dim=-1)
        parts.append(torch.norm(z, dim=-1))
    return stepwise_linear_model_multirank(torch.cat(parts, dim=-1), Bcp_nn, weights, bias)


_plan_cache = {}


def _cached_plan(W, D, N, Rn, Rs, rows, non_negative, softplus_kwargs, dev):
    beta, thr = _engine.softplus_params(softplus_kwargs)
    key = (W, D, N, Rn, Rs, tuple(bool(non_negative[f]) for f in range(3)), beta, thr, dev)
    p = _plan_cache.get(key)
    if p is None or p.max_rows < rows:
        p = ConvPhasePlan(W, D, N, Rn, Rs, rows, non_negative, softplus_kwargs, f"cuda:{dev}")
        _plan_cache[key] = p
    return p


def _lambda3(lambda_L2, n_factors):
    """lambda_L2 as the reference reads it (…py:1245-1249, 1385-1389): a scalar or a length-1 list is
    repeated for (w, d, out); anything else is indexed [0], [1], [2]."""
    if isinstance(lambda_L2, (int, float)):
        return [float(lambda_L2)] * (1 + n_factors)
    if isinstance(lambda_L2, list) and len(lambda_L2) == 1:
        return [float(lambda_L2[0])] * (1 + n_factors)
    return [float(lambda_L2[0]), float(lambda_L2[1]), float(lambda_L2[2])]


class _VerbosePrinter:
    """verbose == 2 / 3 per-iteration print (…py:1418-1444; the total and the variance ratio)."""

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
                 bias_init=0,
                 device='cpu',
                 do_spectralPenalty=False,
                 spectrum_smoothing_factor=100,
                 softplus_kwargs=None):
        """Phase-constrained spectral convolutional CP regression (…py:1034-1181; same arguments and
        attributes; `bias_init` is accepted and unused, as in the reference).  RNG draws in the
        reference's order: Bcp_w normal ranks, Bcp_w spectral ranks, then Bcp_n."""
        if int(temporal_window) % 2 == 0 or int(temporal_window) < 1:
            raise ValueError(f"temporal_window must be odd and >= 1 (got {temporal_window}): with an even window "
                             "the reference's y_hat (T - W + 1 rows) and y[idx_conv] (T - W rows) never match")
        if len(y_shape) < 2:
            raise ValueError("y must be 2-D (T, n_out); the reference's model breaks at the first fit on a 1-D y")
        if dtype == torch.float64:
            raise NotImplementedError("the gfx950 conv kernel computes in fp32; fp64 is not offered")
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
        self.shifter = phase_shifter(signal_len=temporal_window, discard_imaginary_component=True,
                                     device=self.device, dtype=self.dtype, pin_memory=False)
        if Bcp_init is None:
            nn_w = [self.non_negative[0]]
            self.Bcp_w = make_BcpInit(Bw_dims, self.rank_normal, nn_w, complex_dims=None, scale=Bcp_init_scale,
                                      device=self.device, dtype=self.dtype) + \
                make_BcpInit(Bw_dims, self.rank_spectral, nn_w, complex_dims=None, scale=Bcp_init_scale,
                             device=self.device, dtype=self.dtype)
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
        return (int(Kn.shape[0]), int(self.Bcp_n[0].shape[0]), int(self.Bcp_n[1].shape[0]), int(Kn.shape[1]),
                int(Ks.shape[1]))

    def _plan_for(self, X, dev):
        W, D, N, Rn, Rs = self._shape()
        if int(X.shape[1]) != D:
            raise ValueError(f"X must be (T, {D}) for these factors; got {tuple(X.shape)}")
        if int(X.shape[0]) < W:
            raise ValueError(f"X has {X.shape[0]} rows, fewer than temporal_window = {W}")
        return _cached_plan(W, D, N, Rn, Rs, int(X.shape[0]), self.non_negative, self.softplus_kwargs, dev)

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

    def _check_offered(self, X):
        if self.do_spectralPenalty:
            raise NotImplementedError("do_spectralPenalty=True (the output-spectrum penalty) is not offered")
        if type(X).__name__ == "HostStream":
            raise NotImplementedError("HostStream is not offered for the convolutional model")

    def _set_grads(self, plan, gtot):
        o = plan.offsets
        for f, A in enumerate(list(self.Bcp_n) + list(self.Bcp_w)):
            A.grad = gtot[o[f]:o[f + 1]].to(A.device).clone().view(A.shape)
        self.bias.grad = gtot[o[4]:].to(self.bias.device).clone().view(self.bias.shape)

    # ---- fitting -----------------------------------------------------------------------------
    def fit(self, X, y, lambda_L2=0.01, lambda_spectralPenalty=0.01, lambda_smooth=0.01, smooth_diff_order=2,
            max_iter=1000, tol=1e-5, patience=10, verbose=False, running_loss_logging_interval=10,
            LBFGS_kwargs=None):
        """LBFGS fit (…py:1183-1325): torch.optim.LBFGS (kept as self.optimizer) drives the parameters,
        every closure evaluation is one device pass; logs the total loss."""
        self._check_offered(X)
        if LBFGS_kwargs is None:
            raise TypeError("torch.optim.lbfgs.LBFGS() argument after ** must be a mapping, not NoneType")
        lam = _lambda3(lambda_L2, len(self.Bcp_n))
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev)
        plan.set_smoothness(lambda_smooth, smooth_diff_order)
        self.y_spectrum = None
        self.optimizer = torch.optim.LBFGS(list(self.Bcp_n) + list(self.Bcp_w) + [self.bias], **LBFGS_kwargs)
        opts = dict(dtype=torch.float32, device=f"cuda:{dev}")
        grad = torch.zeros(plan.num_grads, **opts)
        gtot = torch.zeros(plan.num_params, **opts)
        loss_out = torch.zeros(1, **opts)
        yhat = torch.empty_like(target)
        norm = float(target.numel())
        var_y = torch.var(y).item() if verbose in (2, 3) else None

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
                if verbose in (2, 3):
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
        """Adam fit (…py:1328-1459), device resident on gfx950, with self.softplus_kwargs (:1432); a
        scalar lambda_L2 is accepted (:1385)."""
        self._check_offered(X)
        if process_group is not None:
            raise NotImplementedError("process_group is not offered for the convolutional model")
        hp = adam_hparams(Adam_kwargs)
        lam = _lambda3(lambda_L2, len(self.Bcp_n))
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev)
        plan.set_smoothness(lambda_smooth, smooth_diff_order)
        self.y_spectrum = None
        self.optimizer = torch.optim.Adam(list(self.Bcp_n) + list(self.Bcp_w) + [self.bias], **Adam_kwargs)
        norm = float(target.numel())
        arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
        vcb = _VerbosePrinter(plan, X, target, y, norm) if verbose in (2, 3) else None
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
        """forward_model with the model's own factors (the Bcp argument is ignored, …py:1675) and
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
        """softplus-applied (Bcp_n, Bcp_w) as numpy lists, with self.softplus_kwargs (…py:1768-1783)."""
        Bcp_n = list(non_neg_fn(self.Bcp_n, self.non_negative[1:], softplus_kwargs=self.softplus_kwargs))
        Bcp_w = list(non_neg_fn(self.Bcp_w, [self.non_negative[0]] * 2, softplus_kwargs=self.softplus_kwargs))
        return [A.detach().cpu().numpy() for A in Bcp_n], [A.detach().cpu().numpy() for A in Bcp_w]

    def detach_Bcp(self):
        """The raw (Bcp_n, Bcp_w) as numpy lists (…py:1785-1796)."""
        return ([A.detach().cpu().numpy() for A in self.Bcp_n], [A.detach().cpu().numpy() for A in self.Bcp_w])

    def get_params(self):
        """The model's state as a dict (…py:1798-1823)."""
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
            'shifter': self.shifter,
        }

    def set_params(self, params):
        """Restore get_params' dict (…py:1825-1848; idx_conv comes back in self.dtype, as there)."""
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
        self.shifter = params['shifter']

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
