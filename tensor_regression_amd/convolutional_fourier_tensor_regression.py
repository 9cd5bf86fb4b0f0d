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
`y_spectrum`), with fit / fit_Adam / predict on the gfx950 kernels: csrc/tr_conv.hip for the X pass
and the update step (smoothness term included), csrc/tr_conv_spectrum.hip for the spectrum path (a
direct real DFT of any length with exact integer angle indices, its adjoint, and the terms between
them).  The class body shared with the other conv models is in _conv_family.py.  Envelope: the conv
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
import torch

from ._conv_family import (SmoothConvModel, _lambda3, _series,  # noqa: F401  (kept importable from this module)
                           gaussian, make_BcpInit, non_neg_fn)
from ._engine import ConvFourierPlan
from .convolutional_spectral_tensor_regression import L2_penalty, complex_magnitude, stepwise_linear_model_multirank
from .phase_constrained_spectral_convolutional_tensor_regression import conv, diff_highOrder, smoothness_penalty

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


####################################
########### Main class #############
####################################

class CP_linear_regression(SmoothConvModel):
    _plan_cls = ConvFourierPlan
    _verbose_levels = (2,)  # verbose == 3 (live plots) raises

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
        self._check_ctor(y_shape, dtype, temporal_window)
        if Bcp_init is None and rank_spectral > 0 and rank_normal == 1:
            raise ValueError("rank_normal == 1 with rank_spectral > 0: the reference's own forward_model fails there "
                             "(it squeezes the single normal rank away before torch.cat)")
        if Bcp_init is None and rank_spectral > 0 and n_complex_dim == 0:
            raise ValueError("n_complex_dim == 0 with rank_spectral > 0: the reference's own forward_model fails "
                             "there (torch.cat of a 3-D and a 2-D block; a norm over the ranks without normal ranks)")
        self._init_model(X_shape, y_shape, dtype, rank_normal, temporal_window, rank_spectral, non_negative,
                         weights, Bcp_init, Bcp_init_scale, [n_complex_dim + 1], device, softplus_kwargs)
        self._init_spectrum(X_shape, do_spectralPenalty, spectrum_smoothing_factor)

    def _check_offered(self, X, verbose, process_group=None):
        if type(X).__name__ == "HostStream":
            raise NotImplementedError("HostStream is not offered for the convolutional model")
        super()._check_offered(X, verbose, process_group)
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
