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
fit / fit_Adam / predict on the gfx950 kernels (csrc/tr_conv.hip for the X pass and the update step,
smoothness term included; csrc/tr_conv_phase.hip for the constraint and its adjoint).  The class body
shared with the other conv models is in _conv_family.py.  Envelope: W odd <= 257, D <= 65536,
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

from ._conv_family import (SmoothConvModel, _lambda3, _series,  # noqa: F401  (kept importable from this module)
                           gaussian, make_BcpInit, non_neg_fn)
from ._engine import ConvPhasePlan
from .convolutional_spectral_tensor_regression import L2_penalty, stepwise_linear_model_multirank
from .convolutional_spectral_tensor_regression import conv as _conv_unfold

__all__ = ["make_BcpInit", "non_neg_fn", "gaussian", "conv", "stepwise_linear_model_multirank", "forward_model",
           "L2_penalty", "diff_highOrder", "smoothness_penalty", "phase_shifter", "CP_linear_regression"]


####################################
######## Helper functions ##########
####################################

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


####################################
########### Main class #############
####################################

class CP_linear_regression(SmoothConvModel):
    _plan_cls = ConvPhasePlan

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
        self._check_ctor(y_shape, dtype, temporal_window)
        self._init_model(X_shape, y_shape, dtype, rank_normal, temporal_window, rank_spectral, non_negative,
                         weights, Bcp_init, Bcp_init_scale, None, device, softplus_kwargs)
        self.shifter = phase_shifter(signal_len=temporal_window, discard_imaginary_component=True,
                                     device=self.device, dtype=self.dtype, pin_memory=False)
        self._init_spectrum(X_shape, do_spectralPenalty, spectrum_smoothing_factor)

    def _shape(self):
        return super()._shape()[:5]  # (W, D, N, Rn, Rs): the phase plan has no component count

    def _check_offered(self, X, verbose, process_group=None):
        if self.do_spectralPenalty:
            raise NotImplementedError("do_spectralPenalty=True (the output-spectrum penalty) is not offered")
        if type(X).__name__ == "HostStream":
            raise NotImplementedError("HostStream is not offered for the convolutional model")
        super()._check_offered(X, verbose, process_group)

    def get_params(self):
        """The model's state as a dict (…py:1798-1823)."""
        return dict(super().get_params(), shifter=self.shifter)

    def set_params(self, params):
        """Restore get_params' dict (…py:1825-1848; idx_conv comes back in self.dtype, as there)."""
        super().set_params(params)
        self.shifter = params['shifter']
