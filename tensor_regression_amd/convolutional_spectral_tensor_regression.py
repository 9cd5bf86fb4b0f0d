"""Convolutional spectral CP regression on MI355X — drop-in for the reference's
`convolutional_spectral_tensor_regression.py` (kimerein/tensor_regression).

The model fits a temporal kernel directly on the untiled `(T, D)` series:

    z[t,d,k]  = sum_w X[t+w,d] * phi(K)[w,k]              (valid cross-correlation, T' = T - W + 1)
    u[t,d,r]  = z (normal ranks; spectral ranks when n_complex_dim == 0: signed)
              | ||z[t,d,s,:]||_2 (spectral ranks)
    y_hat     = (sum_d u * phi(Bd)) . phi(Bo)^T + bias       compared with y[idx_conv]

Same module functions and `CP_linear_regression` class as the reference (arguments, RNG draws and
their order, factor layouts Bcp_w = [Kn (W, Rn), Ks (W, Rs, C)], Bcp_n = [Bd (D, R), Bo (N, R)],
`loss_running`), with fit / fit_Adam / predict on the gfx950 single-pass kernel k_conv
(csrc/tr_conv.hip).  Envelope: W odd <= 257, D <= 65536, n_out <= 64, Rn + Rs <= 32,
n_complex_dim + 1 <= 4, Rn + Rs * (n_complex_dim + 1) <= 64; outside it the plan raises ValueError.

Reference behaviour kept as it is: fit_Adam and predict call conv_linear without softplus_kwargs
(beta 50 / threshold 1 whatever the model was built with) while fit and return_Bcp_final use
self.softplus_kwargs; fit_Adam needs a length-3 lambda_L2; `weights` is stored and never used;
predict ignores its Bcp argument.

Deliberate differences: an even temporal_window and a 1-D y raise ValueError at construction (the
reference fails later, inside the first fit); tensors run on a HIP device in fp32; no
process_group / HostStream.
"""
import torch

from ._conv_family import ConvModelBase, _cached_plan, _series, make_BcpInit, non_neg_fn
from ._engine import ConvPlan

__all__ = ["make_BcpInit", "non_neg_fn", "conv", "complex_magnitude", "conv_linear",
           "stepwise_linear_model_multirank", "L2_penalty", "CP_linear_regression"]


####################################
######## Helper functions ##########
####################################

def L2_penalty(B_cp, lambda_L2):
    """sum_k lambda_L2[k] * ||B_k||_F of the raw factors (…py:700-718)."""
    penalty = 0
    for ii, comp in enumerate(B_cp):
        penalty += torch.sqrt(torch.sum(comp ** 2)) * lambda_L2[ii]
    return penalty


def complex_magnitude(convolved):
    """L2 norm over the trailing complex axis; a single component is returned signed (…py:292-303)."""
    if convolved.shape[-1] < 2:
        return convolved.squeeze(-1)
    return torch.norm(convolved, dim=-1)


def stepwise_linear_model_multirank(X, Bcp, weights, bias):
    """einsum('tr,nr->tn', einsum('tdr,dr->tr', X, Bcp[0]), Bcp[1]) + bias (…py:427-475) on a (T, D, R)
    tensor of convolved features: a small torch expression, kept for API parity (the fit and
    predict paths never materialise X_conv)."""
    Bcp = [b[:, None] if b.ndim == 1 else b for b in Bcp]
    if X.ndim < 3:
        X = X[..., None]
    if Bcp[0].shape[1] == 0:
        return torch.zeros(1).to(X.device)
    return torch.einsum('tr,nr->tn', torch.einsum('tdr,dr->tr', X, Bcp[0]), Bcp[1]) + bias


def _kernel_factors(kernel):
    Kn, Ks = kernel
    C = int(Ks.shape[2]) if Ks.ndim == 3 else 1
    return int(Kn.shape[0]), int(Kn.shape[1]), int(Ks.shape[1]), C


def conv(X, kernel):
    """Valid cross-correlation of every column of X (T, D) with every kernel column (…py:259-290):
    kernel (W, R) or (W, R, C) -> (T - W + 1, D, R, C).  Runs as a torch expression on X's device:
    it is the reference's inspection helper, the fit path fuses it into k_conv."""
    k3 = kernel if kernel.ndim == 3 else kernel[..., None]
    Wd, R, C = k3.shape
    Xu = X.unfold(0, Wd, 1)  # (T', D, W)
    return torch.einsum('tdw,wrc->tdrc', Xu, k3)


def conv_linear(X, kernel, Bcp, weights, non_negative, bias, softplus_kwargs=None):
    """y_hat (T - W + 1, n_out) of the convolutional model (…py:650-678) on the gfx950 forward
    kernel.  kernel = [Kn, Ks], Bcp = [Bd, Bo] (raw factors); `weights` is unused, as in the reference."""
    Xd, dev = _series(X)
    W, Rn, Rs, C = _kernel_factors(kernel)
    D, N = int(Bcp[0].shape[0]), int(Bcp[1].shape[0])
    plan = _cached_plan(ConvPlan, (W, D, N, Rn, Rs, C), Xd.shape[0], list(non_negative), softplus_kwargs, dev)
    b = torch.as_tensor(bias, dtype=torch.float32).reshape(-1)
    if b.numel() == 1 and N > 1:
        b = b.expand(N)
    arena = plan.pack(list(kernel), list(Bcp), b)
    return plan.forward(Xd, arena)


####################################
########### Main class #############
####################################

class CP_linear_regression(ConvModelBase):
    _plan_cls = ConvPlan
    _default_softplus_in_adam = True

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
                 softplus_kwargs=None):
        """Convolutional spectral CP regression (…py:750-877; same arguments and attributes;
        `bias_init` is accepted and unused, as in the reference)."""
        self._check_ctor(y_shape, dtype, temporal_window)
        self._init_model(X_shape, y_shape, dtype, rank_normal, temporal_window, rank_spectral, non_negative,
                         weights, Bcp_init, Bcp_init_scale, [n_complex_dim + 1], device, softplus_kwargs)

    def _lambda_fit(self, lambda_L2):
        if isinstance(lambda_L2, (int, float)):
            return [float(lambda_L2)] * (1 + len(self.Bcp_n))
        if isinstance(lambda_L2, list) and len(lambda_L2) == 1:
            return [float(lambda_L2[0])] * (1 + len(self.Bcp_n))
        return lambda_L2

    def _lambda_adam(self, lambda_L2):
        return [lambda_L2[0], lambda_L2[1], lambda_L2[2]]  # a scalar raises TypeError, as in the reference

    @staticmethod
    def _verbose_line(ii, loss, ratio):
        return f'Iteration: {ii}, Loss: {loss}  ;  Variance ratio (y_hat / y_true): {ratio}'

    def fit(self, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
            running_loss_logging_interval=10, LBFGS_kwargs=None):
        """LBFGS fit (…py:879-989): torch.optim.LBFGS drives the parameters, every closure
        evaluation is one k_conv pass; uses self.softplus_kwargs; logs the total loss."""
        return self._fit_lbfgs(X, y, lambda_L2, max_iter, tol, patience, verbose, running_loss_logging_interval,
                               LBFGS_kwargs)

    def fit_Adam(self, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
                 plotting_interval=100, Adam_kwargs=None, process_group=None):
        """Adam fit (…py:992-1069), device resident on gfx950.  lambda_L2 is the length-3 sequence
        (w, d, out); softplus runs with beta 50 / threshold 1 whatever self.softplus_kwargs says,
        as in the reference."""
        return self._fit_adam(X, y, lambda_L2, max_iter, tol, patience, verbose, Adam_kwargs, process_group)

    def set_params(self, params):
        """As the reference (…py:1439-1456), which assigns params['Bcp'] to self.Bcp."""
        self.weights = params['weights']
        self.Bcp = params['Bcp']
        self.non_negative = params['non_negative']
        self.softplus_kwargs = params['softplus_kwargs']
        self.rank = params['rank']
        self.device = params['device']
        self.loss_running = params['loss_running']
