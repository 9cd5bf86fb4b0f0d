"""Test-local restatement of the convolutional Fourier model: conv_ref's y_hat (unfold + einsum),
phase_ref's smoothness stencil (Ks seen as (W, Rs C)), and the output-spectrum penalty written as an
explicit DFT matrix with its closed-form gradient into y_hat; torch autograd for the rest, in the
dtype of its inputs.  tests/test_fourier_host.py checks the closed form against autograd through
torch.fft.rfft and the whole restatement against every cfs_* fixture; the GPU tests then use it in
fp64 as their yardstick."""
import numpy as np
import torch

import conv_ref
import phase_ref
from conv_ref import data_loss, lam3, leaf_params, load, penalty, y_hat  # noqa: F401
from phase_ref import arena_of, rel, softplus_of  # noqa: F401

PENALTY_FIXTURES = ["cfs_base", "cfs_rn0", "cfs_rs0", "cfs_c3", "cfs_n1", "cfs_ssf100", "cfs_ssf1", "cfs_nn_all",
                    "cfs_lam1", "cfs_wide", "cfs_amsgrad_wd", "cfs_converge", "cfs_f32x"]
ADAM_FIXTURES = PENALTY_FIXTURES + ["cfs_off", "cfs_off_c4"]
ALL_FIXTURES = ADAM_FIXTURES + ["cfs_lbfgs"]
FACTORS = conv_ref.FACTORS


def smoothing_kernel(ssf, dtype=torch.float64):
    """The constructor's gaussian (…py:1042-1048): 2 (ssf // 2) + 1 taps, sigma = ssf / 7."""
    x = np.arange(-(ssf // 2), ssf // 2 + 1)
    sig = ssf / 7
    return torch.tensor(1 / (np.sqrt(2 * np.pi) * sig) * np.exp(-np.power(x / sig, 2) / 2), dtype=dtype)


def dft_parts(x, n_fft):
    """C[k] = sum_t x[t] cos(2 pi k t / n), S[k] = sum_t x[t] sin(2 pi k t / n), k < n // 2 + 1, with
    the angle index (k t) mod n formed in integers: rfft(x, n) = C - i S."""
    rows = x.shape[0]
    k = torch.arange(n_fft // 2 + 1, dtype=torch.int64)[:, None]
    t = torch.arange(rows, dtype=torch.int64)[None, :]
    th = (2.0 * np.pi / n_fft) * ((k * t) % n_fft).to(torch.float64)
    return torch.cos(th).to(x.dtype) @ x, torch.sin(th).to(x.dtype) @ x, th


def smooth(A, g):
    """M[j] = sum_s A[j + s] g[s] (valid, no flip)."""
    S = g.shape[0]
    return torch.einsum('jsn,s->jn', A.unfold(0, S, 1).permute(0, 2, 1), g)


def spectrum(x, n_fft, g):
    C, S, _ = dft_parts(x, n_fft)
    return smooth(torch.sqrt(C * C + S * S), g)


def spectrum_penalty(x, n_fft, g, M_y, lam):
    """lam * mean(((M - M_y) / (M_y + 1e-8))^2)."""
    return lam * torch.mean(((spectrum(x, n_fft, g) - M_y) / (M_y + 1e-8)) ** 2)


def spectrum_penalty_grad(x, n_fft, g, M_y, lam):
    """(value, d pen / d x) by the closed form: dM = 2 lam / (Fs N) (M - M_y) / (M_y + 1e-8)^2,
    dA[k] = sum_s dM[k - s] g[s], G = dA Y / |Y| (0 where |Y| = 0),
    d pen / d x[t] = sum_{k < F} (Re G cos - Im G sin); no factor 2 for the mirrored half."""
    C, S, th = dft_parts(x, n_fft)
    A = torch.sqrt(C * C + S * S)
    M = smooth(A, g)
    r = (M - M_y) / (M_y + 1e-8)
    val = lam * torch.mean(r ** 2)
    dM = (2.0 * lam / M.numel()) * r / (M_y + 1e-8)
    dA = torch.zeros_like(A)
    for s in range(g.shape[0]):
        dA[s:s + M.shape[0]] += dM * g[s]
    f = torch.where(A > 0, dA / torch.where(A > 0, A, torch.ones_like(A)), torch.zeros_like(A))
    # Re G = f C, Im G = -f S
    grad = torch.cos(th).to(x.dtype).T @ (f * C) + torch.sin(th).to(x.dtype).T @ (f * S)
    return val, grad


def smoothness(Kn, Ks, lam_s, q):
    """sum over the non-empty factors of lam_s mean((Delta^q F)^2), Delta^q along the window axis."""
    return phase_ref.smoothness(Kn, Ks.reshape(Ks.shape[0], -1), lam_s, q)


def value_and_grads(X, y, P, nn, lam=None, lam_s=0.0, q=2, beta=50.0, thr=1.0, spec=None):
    """y_hat, (loss_rec, pen, total) and the gradients of every parameter.  lam None: the data term
    alone; spec = (n_fft, g, M_y, lam_sp) adds the spectrum penalty."""
    for A in P.values():
        A.grad = None
    yh = y_hat(X, P["Kn"], P["Ks"], P["Bd"], P["Bo"], P["bias"], nn, beta, thr)
    rec = data_loss(yh, y, P["Kn"].shape[0])
    pen = spectrum_penalty(yh, *spec) if spec is not None else torch.zeros((), dtype=yh.dtype)
    loss = rec
    if lam is not None:
        loss = rec + penalty(P["Kn"], P["Ks"], P["Bd"], P["Bo"], lam) + pen + smoothness(P["Kn"], P["Ks"], lam_s, q)
    elif spec is not None:
        loss = rec + pen
    loss.backward()
    grads = {k: (A.grad.detach().clone() if A.grad is not None else torch.zeros_like(A)) for k, A in P.items()}
    return yh.detach(), (float(rec.item()), float(pen.item()), float(loss.item())), grads


def fixture_spec(d, dtype=torch.float64):
    """(n_fft, g, M_y, lam_sp) of a fixture, M_y restated from y (None with the flag off)."""
    m = d["meta"]
    if not m["do_spectralPenalty"]:
        return None
    W, T = m["W"], m["T"]
    g = smoothing_kernel(m["spectrum_smoothing_factor"], dtype)
    y = torch.tensor(d["y"], dtype=dtype)
    return T, g, spectrum(y[W // 2: T - W // 2], T, g), m["lambda_spectralPenalty"]
