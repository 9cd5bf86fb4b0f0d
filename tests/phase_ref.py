"""Test-local restatement of the phase-constrained spectral convolutional model (unfold + einsum,
the quadrature map H built from its closed form, the smoothness term as a stencil; torch autograd),
in the dtype of its inputs.  tests/test_phase_host.py qualifies it against every pcs_* fixture; the
GPU shape sweep then uses it in fp64 as its yardstick."""
import json
import math
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADAM_FIXTURES = ["pcs_base", "pcs_rn0", "pcs_rs0", "pcs_r1", "pcs_n1", "pcs_w1", "pcs_wide", "pcs_nn_all", "pcs_nn_w",
                 "pcs_order1", "pcs_order3", "pcs_smooth0", "pcs_zero", "pcs_amsgrad_wd", "pcs_converge", "pcs_f32x"]
ALL_FIXTURES = ADAM_FIXTURES + ["pcs_lbfgs"]
FACTORS = ("Kn", "Ks", "Bd", "Bo", "bias")
ARENA = ("Bd", "Bo", "Kn", "Ks", "bias")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    d["X"] = d["X_f32"] if "X_f32" in d else d["X_q"].astype(np.float32) / 8.0
    return d


def softplus_of(meta):
    kw = meta["softplus_kwargs"]
    return float(kw.get("beta", 1.0)), float(kw.get("threshold", 20.0))


def quadrature_h(W):
    """h[d] = (2 / W) sum_{j=1..(W-1)/2} sin(2 pi j d / W), fp64."""
    return torch.tensor([2.0 / W * sum(math.sin(2.0 * math.pi * j * d / W) for j in range(1, (W - 1) // 2 + 1))
                         for d in range(W)], dtype=torch.float64)


def quadrature_H(W, dtype=torch.float64):
    """H[n, m] = h[(n - m) mod W]."""
    n = torch.arange(W)
    return quadrature_h(W)[(n[:, None] - n[None, :]) % W].to(dtype)


def _phi(A, flag, beta, thr):
    return torch.nn.functional.softplus(A, beta=beta, threshold=thr) if flag else A


def y_hat(X, Kn, Ks, Bd, Bo, bias, nn, beta=50.0, thr=1.0):
    """(T - W + 1, N) model output; nn = (w, d, out) flags; Ks is (W, Rs)."""
    W = Kn.shape[0]
    Xu = X.unfold(0, W, 1)  # (T', D, W)
    parts = []
    if Kn.shape[1] > 0:
        parts.append(torch.einsum('tdw,wr->tdr', Xu, _phi(Kn, nn[0], beta, thr)))
    if Ks.shape[1] > 0:
        k = _phi(Ks, nn[0], beta, thr)
        z0 = torch.einsum('tdw,ws->tds', Xu, k)
        z1 = torch.einsum('tdw,ws->tds', Xu, quadrature_H(W, k.dtype) @ k)
        parts.append(torch.linalg.vector_norm(torch.stack([z0, z1], dim=-1), dim=-1))
    u = torch.cat(parts, dim=-1)
    q = torch.einsum('tdr,dr->tr', u, _phi(Bd, nn[1], beta, thr))
    return q @ _phi(Bo, nn[2], beta, thr).T + bias


def data_loss(yh, y, W):
    return torch.mean((yh - y[W // 2: y.shape[0] - W // 2]) ** 2)


def penalty(Kn, Ks, Bd, Bo, lam):
    n = lambda A: torch.sqrt(torch.sum(A ** 2))  # noqa: E731
    return lam[0] * (n(Kn) + n(Ks)) + lam[1] * n(Bd) + lam[2] * n(Bo)


def stencil_diff(F, q):
    """(Delta^q F)[i] = sum_j (-1)^j C(q, j) F[i - j], i = 0..W+q-1 (F zero outside its rows)."""
    W = F.shape[0]
    out = torch.zeros((W + q,) + tuple(F.shape[1:]), dtype=F.dtype)
    for j in range(q + 1):
        out[j:j + W] = out[j:j + W] + ((-1) ** j) * math.comb(q, j) * F
    return out


def smoothness(Kn, Ks, lam_s, q):
    tot = 0
    for F in (Kn, Ks):
        if F.numel() > 0:
            tot = tot + lam_s * torch.mean(stencil_diff(F, q) ** 2)
    return tot


def leaf_params(d, dtype, sfx="0"):
    return {k: torch.tensor(d[k + sfx], dtype=dtype, requires_grad=True) for k in FACTORS}


def value_and_grads(X, y, P, nn, lam=None, lam_s=0.0, q=2, beta=50.0, thr=1.0):
    """y_hat, data loss (+ L2 and smoothness when lam is given) and the gradients of every parameter."""
    for A in P.values():
        A.grad = None
    yh = y_hat(X, P["Kn"], P["Ks"], P["Bd"], P["Bo"], P["bias"], nn, beta, thr)
    loss = data_loss(yh, y, P["Kn"].shape[0])
    if lam is not None:
        loss = loss + penalty(P["Kn"], P["Ks"], P["Bd"], P["Bo"], lam) + smoothness(P["Kn"], P["Ks"], lam_s, q)
    loss.backward()
    grads = {k: (A.grad.detach().clone() if A.grad is not None else torch.zeros_like(A)) for k, A in P.items()}
    return yh.detach(), float(loss.item()), grads


def lam3(meta):
    lam = meta["lambda_L2"]
    return [lam] * 3 if not isinstance(lam, list) else lam


def rel(a, b):
    """normwise relative distance ||a - b|| / ||b|| (0 / 0 = 0) over the entries where b is not NaN;
    a must be NaN exactly where b is (else inf)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    if a.shape != b.shape or not np.array_equal(np.isnan(a), np.isnan(b)):
        return float("inf")
    ok = ~np.isnan(b)
    a, b = a[ok], b[ok]
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))


def arena_of(g):
    return np.concatenate([np.asarray(g[k], np.float64).ravel() for k in ARENA])
