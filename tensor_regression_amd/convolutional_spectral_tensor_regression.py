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
import numpy as np
import torch

from . import _engine
from ._engine import ConvPlan, adam_hparams, as_device_f32, run_adam_fit

__all__ = ["make_BcpInit", "non_neg_fn", "conv", "complex_magnitude", "conv_linear",
           "stepwise_linear_model_multirank", "L2_penalty", "CP_linear_regression"]

_DEFAULT_SOFTPLUS = {'beta': 50, 'threshold': 1}


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
        softplus_kwargs = _DEFAULT_SOFTPLUS
    for A, nn in zip(B_cp, non_negative):
        yield torch.nn.functional.softplus(A, **softplus_kwargs) if nn else A


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


_plan_cache = {}


def _cached_plan(W, D, N, Rn, Rs, C, rows, non_negative, softplus_kwargs, dev):
    beta, thr = _engine.softplus_params(softplus_kwargs)
    key = (W, D, N, Rn, Rs, C, tuple(bool(non_negative[f]) for f in range(3)), beta, thr, dev)
    p = _plan_cache.get(key)
    if p is None or p.max_rows < rows:
        p = ConvPlan(W, D, N, Rn, Rs, C, rows, non_negative, softplus_kwargs, f"cuda:{dev}")
        _plan_cache[key] = p
    return p


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
    plan = _cached_plan(W, D, N, Rn, Rs, C, Xd.shape[0], list(non_negative), softplus_kwargs, dev)
    b = torch.as_tensor(bias, dtype=torch.float32).reshape(-1)
    if b.numel() == 1 and N > 1:
        b = b.expand(N)
    arena = plan.pack(list(kernel), list(Bcp), b)
    return plan.forward(Xd, arena)


class _VerbosePrinter:
    """verbose == 2 / 3 per-iteration print of the reference (…py:1050-1055) from the kernel's y_hat."""

    def __init__(self, plan, X, target, y, norm):
        self.plan, self.X, self.t, self.norm = plan, X, target, norm
        self.var_y = torch.var(y).item()
        self.grad = torch.zeros(plan.num_grads, dtype=torch.float32, device=X.device)
        self.yhat = torch.empty_like(target)

    def before_step(self, arena):
        self.plan.loss_grad(self.X, self.t, None, self.norm, arena, None, self.grad, yhat=self.yhat)

    def after_step(self, ii, loss):
        ratio = torch.var(self.yhat).item() / self.var_y
        print(f'Iteration: {ii}, Loss: {loss}  ;  Variance ratio (y_hat / y_true): {ratio}')


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
                 softplus_kwargs=None):
        """Convolutional spectral CP regression (…py:750-877; same arguments and attributes;
        `bias_init` is accepted and unused, as in the reference)."""
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
        self.y_shape = y_shape
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
        self.loss_running = []

    # ---- plumbing --------------------------------------------------------------------------
    def _shape(self):
        W, Rn, Rs, C = _kernel_factors(self.Bcp_w)
        return W, int(self.Bcp_n[0].shape[0]), int(self.Bcp_n[1].shape[0]), Rn, Rs, C

    def _plan_for(self, X, dev, softplus_kwargs):
        W, D, N, Rn, Rs, C = self._shape()
        if int(X.shape[1]) != D:
            raise ValueError(f"X must be (T, {D}) for these factors; got {tuple(X.shape)}")
        if int(X.shape[0]) < W:
            raise ValueError(f"X has {X.shape[0]} rows, fewer than temporal_window = {W}")
        return _cached_plan(W, D, N, Rn, Rs, C, int(X.shape[0]), self.non_negative, softplus_kwargs, dev)

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

    def _set_grads(self, plan, gtot):
        o = plan.offsets
        for f, A in enumerate(list(self.Bcp_n) + list(self.Bcp_w)):
            A.grad = gtot[o[f]:o[f + 1]].to(A.device).clone().view(A.shape)
        self.bias.grad = gtot[o[4]:].to(self.bias.device).clone().view(self.bias.shape)

    # ---- fitting -----------------------------------------------------------------------------
    def fit(self, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
            running_loss_logging_interval=10, LBFGS_kwargs=None):
        """LBFGS fit (…py:879-989): torch.optim.LBFGS drives the parameters, every closure
        evaluation is one k_conv pass; uses self.softplus_kwargs; logs the total loss."""
        if LBFGS_kwargs is None:
            raise TypeError("torch.optim.lbfgs.LBFGS() argument after ** must be a mapping, not NoneType")
        if isinstance(lambda_L2, (int, float)):
            lambda_L2 = [float(lambda_L2)] * (1 + len(self.Bcp_n))
        elif isinstance(lambda_L2, list) and len(lambda_L2) == 1:
            lambda_L2 = [float(lambda_L2[0])] * (1 + len(self.Bcp_n))
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev, self.softplus_kwargs)
        optimizer = torch.optim.LBFGS(list(self.Bcp_n) + list(self.Bcp_w) + [self.bias], **LBFGS_kwargs)
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
            plan.finalize_grad(arena, grad, lambda_L2, gtot, loss_out)
            if with_grads:
                self._set_grads(plan, gtot)
            return loss_out[0].clone()

        def closure():
            optimizer.zero_grad()
            return total_loss(True)

        convergence_reached = False
        for ii in range(max_iter):
            if ii % running_loss_logging_interval == 0:
                self.loss_running.append(total_loss(False).item())
                if verbose in (2, 3):
                    print(f'Iteration: {ii}, Loss: {self.loss_running[-1]}  ;  Variance ratio (y_hat / y_true): '
                          f'{torch.var(yhat).item() / var_y}')
            if len(self.loss_running) > patience:
                if np.sum(np.abs(np.diff(self.loss_running[-patience + 1:]))) < tol:
                    convergence_reached = True
                    break
            elif np.isnan(self.loss_running[-1]):
                convergence_reached = False
                print('Loss is NaN. Stopping.')
                break
            optimizer.step(closure)
        if (verbose is True) or (verbose >= 1):
            print('Convergence reached' if convergence_reached else
                  'Reached maximum number of iterations without convergence')
        return convergence_reached

    def fit_Adam(self, X, y, lambda_L2=0.01, max_iter=1000, tol=1e-5, patience=10, verbose=False,
                 plotting_interval=100, Adam_kwargs=None, process_group=None):
        """Adam fit (…py:992-1069), device resident on gfx950.  lambda_L2 is the length-3 sequence
        (w, d, out); softplus runs with beta 50 / threshold 1 whatever self.softplus_kwargs says,
        as in the reference."""
        if process_group is not None:
            raise NotImplementedError("process_group is not offered for the convolutional model")
        hp = adam_hparams(Adam_kwargs)
        lam = [lambda_L2[0], lambda_L2[1], lambda_L2[2]]  # a scalar raises TypeError, as in the reference
        X, y, target, dev = self._inputs(X, y)
        plan = self._plan_for(X, dev, None)
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
        """conv_linear with the model's own factors (the Bcp argument is ignored, …py:1297) and
        softplus beta 50 / threshold 1, as a detached CPU tensor (T - W + 1, n_out)."""
        if device is None:
            device = self.device
        dev = None if isinstance(X, torch.Tensor) and X.device.type == "cuda" else _engine.device_index(device)
        Xd, dev = _series(X, dev)
        plan = self._plan_for(Xd, dev, None)
        arena = plan.pack(self.Bcp_w, self.Bcp_n, self.bias)
        return plan.forward(Xd, arena).cpu().detach()

    def get_idxConv(self, input_length):
        return torch.arange(self.temporal_window // 2, input_length - self.temporal_window // 2)

    def return_Bcp_final(self):
        """softplus-applied (Bcp_n, Bcp_w) as numpy lists, with self.softplus_kwargs (…py:1392-1407)."""
        Bcp_n = list(non_neg_fn(self.Bcp_n, self.non_negative[1:], softplus_kwargs=self.softplus_kwargs))
        Bcp_w = list(non_neg_fn(self.Bcp_w, [self.non_negative[0]] * 2, softplus_kwargs=self.softplus_kwargs))
        return [A.detach().cpu().numpy() for A in Bcp_n], [A.detach().cpu().numpy() for A in Bcp_w]

    def set_params(self, params):
        """As the reference (…py:1439-1456), which assigns params['Bcp'] to self.Bcp."""
        self.weights = params['weights']
        self.Bcp = params['Bcp']
        self.non_negative = params['non_negative']
        self.softplus_kwargs = params['softplus_kwargs']
        self.rank = params['rank']
        self.device = params['device']
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
