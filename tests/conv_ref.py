"""Test-local restatement of the convolutional spectral model (unfold + einsum, torch autograd,
torch.optim.Adam), in the dtype of its inputs.  tests/test_conv_host.py qualifies it in fp32
against every cvs_* fixture; the GPU shape sweep then uses it in fp64 as its yardstick."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
ADAM_FIXTURES = ["cvs_base", "cvs_nn_all", "cvs_nn_d", "cvs_c1", "cvs_c3", "cvs_rn0", "cvs_rs0", "cvs_amsgrad_wd",
                 "cvs_wide_n1", "cvs_f32x", "cvs_zero", "cvs_converge"]
ALL_FIXTURES = ADAM_FIXTURES + ["cvs_lbfgs"]
FACTORS = ("Kn", "Ks", "Bd", "Bo", "bias")


def load(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    d = {k: z[k] for k in z.files}
    d["meta"] = json.loads(str(d["meta"]))
    d["X"] = d["X_f32"] if "X_f32" in d else d["X_q"].astype(np.float32) / 8.0
    return d


def fit_softplus(meta):
    """(beta, threshold) the reference's fit of this fixture ran with: fit_Adam always 50 / 1,
    fit (LBFGS) the model's softplus_kwargs."""
    if meta["lbfgs_kwargs"] is None:
        return 50.0, 1.0
    kw = meta["softplus_kwargs"]
    return float(kw.get("beta", 1.0)), float(kw.get("threshold", 20.0))


def _phi(A, flag, beta, thr):
    return torch.nn.functional.softplus(A, beta=beta, threshold=thr) if flag else A


def y_hat(X, Kn, Ks, Bd, Bo, bias, nn, beta=50.0, thr=1.0):
    """(T - W + 1, N) model output; nn = (w, d, out) flags; Ks is (W, Rs) or (W, Rs, C)."""
    W = Kn.shape[0]
    Xu = X.unfold(0, W, 1)  # (T', D, W)
    parts = []
    if Kn.shape[1] > 0:
        parts.append(torch.einsum('tdw,wr->tdr', Xu, _phi(Kn, nn[0], beta, thr)))
    if Ks.shape[1] > 0:
        k = _phi(Ks, nn[0], beta, thr)
        k = k if k.ndim == 3 else k[..., None]
        z = torch.einsum('tdw,wsc->tdsc', Xu, k)
        parts.append(z[..., 0] if k.shape[2] == 1 else torch.linalg.vector_norm(z, dim=-1))
    u = torch.cat(parts, dim=-1)
    q = torch.einsum('tdr,dr->tr', u, _phi(Bd, nn[1], beta, thr))
    return q @ _phi(Bo, nn[2], beta, thr).T + bias


def data_loss(yh, y, W):
    return torch.mean((yh - y[W // 2: y.shape[0] - W // 2]) ** 2)


def penalty(Kn, Ks, Bd, Bo, lam):
    n = lambda A: torch.sqrt(torch.sum(A ** 2))  # noqa: E731
    return lam[0] * (n(Kn) + n(Ks)) + lam[1] * n(Bd) + lam[2] * n(Bo)


def leaf_params(d, dtype, sfx="0"):
    return {k: torch.tensor(d[k + sfx], dtype=dtype, requires_grad=True) for k in FACTORS}


def value_and_grads(X, y, P, nn, lam=None, beta=50.0, thr=1.0):
    """y_hat, data loss (+ penalty when lam is given) and the gradients of every parameter."""
    for A in P.values():
        A.grad = None
    yh = y_hat(X, P["Kn"], P["Ks"], P["Bd"], P["Bo"], P["bias"], nn, beta, thr)
    loss = data_loss(yh, y, P["Kn"].shape[0])
    if lam is not None:
        loss = loss + penalty(P["Kn"], P["Ks"], P["Bd"], P["Bo"], lam)
    loss.backward()
    grads = {k: (A.grad.detach().clone() if A.grad is not None else torch.zeros_like(A)) for k, A in P.items()}
    return yh.detach(), float(loss.item()), grads


def adam_losses(X, y, P, nn, lam, adam_kwargs, iters):
    opt = torch.optim.Adam([P[k] for k in ("Bd", "Bo", "Kn", "Ks", "bias")], **adam_kwargs)
    losses = []
    for _ in range(iters):
        opt.zero_grad()
        yh = y_hat(X, P["Kn"], P["Ks"], P["Bd"], P["Bo"], P["bias"], nn)
        loss = data_loss(yh, y, P["Kn"].shape[0]) + penalty(P["Kn"], P["Ks"], P["Bd"], P["Bo"], lam)
        loss.backward()
        opt.step()
        losses.append(loss.item())
    return losses


def lam3(meta):
    lam = meta["lambda_L2"]
    return [lam] * 3 if not isinstance(lam, list) else lam


def rel(a, b):
    """normwise relative distance ||a - b|| / ||b|| (0 / 0 = 0)."""
    a, b = np.asarray(a, np.float64).ravel(), np.asarray(b, np.float64).ravel()
    nb = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / nb) if nb > 0 else float(np.linalg.norm(a - b))
