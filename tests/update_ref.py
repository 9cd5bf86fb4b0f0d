"""Test-local reference of the update step (tr_finalize_grad / tr_adam_step): the penalty of each
plan family and its gradient by torch autograd in fp64, the Adam / AMSGrad formulas of
include/tensor_regression_hip.h (the tr_adam_step comment) in fp64, and the reference's own
optimizer (torch.optim.Adam on the CPU, foreach=False, state preloaded) as the yardstick a device
result is measured with.  Everything works on the flat parameter arena
[factor 0 | factor 1 | ... | bias entries]; `offsets` / `shapes` are the plan's.

tests/test_gpu_update.py is the user; nothing here needs a GPU."""
import numpy as np
import torch

import conv_ref
import fourier_ref
import phase_ref

# Adam hyperparameters in the form of tensor_regression_amd._engine.adam_hparams
HP_DEFAULT = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.0, amsgrad=False)


def hparams(**kw):
    hp = dict(HP_DEFAULT)
    hp.update(kw)
    return hp


def factors_of(arena, offsets, shapes):
    """The factor views of a flat arena tensor (bias entries, after offsets[len(shapes)], left out)."""
    return [arena[offsets[f]:offsets[f + 1]].reshape(shp) for f, shp in enumerate(shapes)]


def make_penalty(kind, offsets, shapes, lam, lam_smooth=0.0, order=2):
    """penalty(arena) -> scalar tensor in arena's dtype.
    kind "l2":    lam * sum_f sqrt(sum(A_f^2)) over the raw factors (linear, multinomial, spectral, f64)
    kind "conv":  conv_ref.penalty with lam = (w, d, out); arena order Bd | Bo | Kn | Ks
    kind "phase": phase_ref.penalty + phase_ref.smoothness(lam_smooth, order); same arena order
    kind "fourier": conv_ref.penalty + fourier_ref.smoothness (Ks (W, Rs, C) seen as (W, Rs C)); same arena
                  order; the spectrum penalty is off"""
    def penalty(arena):
        A = factors_of(arena, offsets, shapes)
        if kind == "l2":
            tot = 0
            for F in A:
                tot = tot + torch.sqrt(torch.sum(F ** 2))
            return lam * tot
        Bd, Bo, Kn, Ks = A
        if kind == "conv":
            return conv_ref.penalty(Kn, Ks, Bd, Bo, lam)
        if kind == "phase":
            return phase_ref.penalty(Kn, Ks, Bd, Bo, lam) + phase_ref.smoothness(Kn, Ks, lam_smooth, order)
        if kind == "fourier":
            return conv_ref.penalty(Kn, Ks, Bd, Bo, lam) + fourier_ref.smoothness(Kn, Ks, lam_smooth, order)
        raise ValueError(kind)
    return penalty


def total_grad(params, grad_data, loss_data, penalty, dtype=torch.float64):
    """(data gradient + autograd of the penalty, data loss + penalty) in `dtype` as numpy arrays / float."""
    p = torch.tensor(np.asarray(params, dtype=np.float64), dtype=dtype, requires_grad=True)
    pen = penalty(p)
    pg = torch.autograd.grad(pen, p)[0] if isinstance(pen, torch.Tensor) and pen.requires_grad else torch.zeros_like(p)
    g = torch.tensor(np.asarray(grad_data, dtype=np.float64), dtype=dtype) + pg
    total = torch.tensor(float(loss_data), dtype=dtype) + (pen.detach() if isinstance(pen, torch.Tensor) else pen)
    return g.numpy(), total.numpy()[()]


def total_grad_longdouble(params, grad_data, loss_data, offsets, n_factors, lam):
    """The "l2" penalty in numpy.longdouble: lam * A_f / ||A_f|| per factor, total = loss + lam * sum ||A_f||."""
    ld = np.longdouble
    p = np.asarray(params).astype(ld)
    g = np.asarray(grad_data).astype(ld).copy()
    total = ld(loss_data)
    for f in range(n_factors):
        A = p[offsets[f]:offsets[f + 1]]
        n = np.sqrt(np.sum(A * A))
        g[offsets[f]:offsets[f + 1]] += ld(lam) * A / n
        total = total + ld(lam) * n
    return g, total


def adam_ref(params, g, m, v, vmax, hp, t, ftype=np.float64):
    """One step of the header's formulas in `ftype` (float64 or longdouble) from the total gradient g:
      g += wd * p; m = lerp(m, g, 1 - b1); v = v * b2 + (1 - b2) g^2; vmax = max(vmax, v) if amsgrad;
      denom = sqrt(v or vmax) / sqrt(1 - b2^t) + eps; p -= lr / (1 - b1^t) * m / denom.
    Returns (params, m, v, vmax); vmax is returned unchanged (None allowed) without amsgrad."""
    c = lambda x: ftype(x)  # noqa: E731
    p, g, m, v = (np.asarray(a).astype(ftype) for a in (params, g, m, v))
    b1, b2 = c(hp["beta1"]), c(hp["beta2"])
    g = g + c(hp["weight_decay"]) * p
    m = m + (c(1) - b1) * (g - m)
    v = v * b2 + (c(1) - b2) * g * g
    if hp["amsgrad"]:
        vmax = np.maximum(np.asarray(vmax).astype(ftype), v)
        src = vmax
    else:
        src = v
    denom = np.sqrt(src) / np.sqrt(c(1) - b2 ** int(t)) + c(hp["eps"])
    p = p - c(hp["lr"]) / (c(1) - b1 ** int(t)) * m / denom
    return p, m, v, vmax


class TorchAdam:
    """The reference's optimizer on the same inputs: torch.optim.Adam (CPU, foreach=False) on the arena as
    one parameter, the penalty by autograd in `dtype`, the state preloaded as after step t0 - 1."""

    def __init__(self, params, m, v, vmax, hp, t0, penalty, dtype=torch.float32):
        self.dtype = dtype
        self.penalty = penalty
        self.p = torch.tensor(np.asarray(params), dtype=dtype, requires_grad=True)
        self.opt = torch.optim.Adam([self.p], lr=hp["lr"], betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"],
                                    weight_decay=hp["weight_decay"], amsgrad=hp["amsgrad"], foreach=False)
        st = {"step": torch.tensor(float(t0 - 1)),
              "exp_avg": torch.tensor(np.asarray(m), dtype=dtype).clone(),
              "exp_avg_sq": torch.tensor(np.asarray(v), dtype=dtype).clone()}
        if hp["amsgrad"]:
            st["max_exp_avg_sq"] = torch.tensor(np.asarray(vmax), dtype=dtype).clone()
        self.opt.state[self.p] = st

    def step(self, grad_data):
        """loss.backward() of data term + penalty, then optimizer.step(); returns (params, m, v, vmax | None)."""
        self.opt.zero_grad()
        pen = self.penalty(self.p)
        if isinstance(pen, torch.Tensor) and pen.requires_grad:
            pen.backward()
        gd = torch.tensor(np.asarray(grad_data), dtype=self.dtype)
        self.p.grad = gd if self.p.grad is None else self.p.grad + gd
        self.opt.step()
        st = self.opt.state[self.p]
        vm = st["max_exp_avg_sq"].numpy().copy() if "max_exp_avg_sq" in st else None
        return self.p.detach().numpy().copy(), st["exp_avg"].numpy().copy(), st["exp_avg_sq"].numpy().copy(), vm


def err(got, ref):
    """e = max_i |got_i - ref_i| / (|ref_i| + rms(ref)), in the precision of ref (inf on a shape or NaN mismatch)."""
    ref = np.asarray(ref)
    got = np.asarray(got).astype(ref.dtype)
    if got.shape != ref.shape or np.isnan(got).any() or np.isnan(ref).any():
        return float("inf")
    if ref.size == 0:
        return 0.0
    rms = np.sqrt(np.mean(ref * ref))
    den = np.abs(ref) + rms
    if not np.all(den > 0):
        return 0.0 if np.array_equal(got, ref) else float("inf")
    return float(np.max(np.abs(got - ref) / den))
