"""Test-local torch restatement of the hierarchical multinomial module's fit_Adam
(multinomial_tensor_regression_hierarchical.py:383-470 with tensorly's cp_to_tensor / inner of the
pytorch backend): one torch.optim.Adam param group for each of Bcp[0], Bcp[1], Bcp[2], factors past
the third in no group (gradient and L2 term, no step), the unweighted CrossEntropyLoss on the
softmax output (the reference's double softmax), and the module's `group_lr` extension executed as
`optimizer.param_groups[g]['lr'] = lr` at the top of iteration first_iteration.

fp32 reproduces the fixtures of tools/gen_golden_hier.py bitwise (tests/test_hier_host.py); fp64 is
the accuracy yardstick of tests/test_gpu_hier.py.  Nothing here needs a GPU."""
import json
import os

import numpy as np
import torch

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
DEFAULT_SOFTPLUS = {"beta": 50, "threshold": 1}
ADAM_FIXTURES = ["hier_kim", "hier_signed", "hier_cpw", "hier_converge", "hier_wd", "hier_4d", "hier_group_lr"]


def load(name):
    """A hier_* fixture: arrays as stored, `meta` decoded, factor lists split by meta['factor_shapes']."""
    d = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    meta = json.loads(str(d.pop("meta")))
    d["meta"] = meta
    shapes = [tuple(s) for s in meta["factor_shapes"]]
    for key in list(d):
        if key.startswith("Bcp") or key.startswith("grads"):
            flat, out, k = d[key], [], 0
            for s in shapes:
                n = int(np.prod(s))
                out.append(flat[k:k + n].reshape(s))
                k += n
            d[key + "_list"] = out
    return d


def model(X, Bcp, weights, non_negative, softplus_kwargs=None):
    kw = DEFAULT_SOFTPLUS if softplus_kwargs is None else softplus_kwargs
    F = [torch.nn.functional.softplus(A, **kw) if non_negative[i] else A for i, A in enumerate(Bcp)]
    # tensorly khatri_rao(skip_matrix=0) and cp_to_tensor, pytorch backend
    kr = F[1]
    for e in F[2:]:
        kr = torch.reshape(kr[:, None, :] * e[None, :, :], (-1, kr.shape[1]))
    B = torch.reshape(torch.matmul(F[0] * weights, torch.transpose(kr, 0, 1)), [f.shape[0] for f in F])
    n = len(Bcp) - 1
    P = int(np.prod(X.shape[X.ndim - n:]))
    Z = torch.matmul(torch.reshape(X, (-1, P)), torch.reshape(B, (P, -1)))
    return torch.nn.functional.softmax(Z, dim=1)


def l2_penalty(Bcp):
    ii = 0
    for comp in Bcp:
        ii += torch.sqrt(torch.sum(comp ** 2))
    return ii


def lr_schedule(group_lr, lr):
    """[(first_iteration, lr), ...] for each of the three groups."""
    if group_lr is None:
        return [[(0, lr)]] * 3
    return [[(0, e)] if np.isscalar(e) else [tuple(p) for p in e] for e in group_lr]


def loss_grad(X, y, Bcp0, weights, non_negative, lambda_L2, softplus_kwargs=None, dtype=torch.float32):
    """probabilities, total loss and autograd gradients of every factor at Bcp0."""
    Bcp = [torch.tensor(np.asarray(A), dtype=dtype, requires_grad=True) for A in Bcp0]
    X = torch.as_tensor(np.asarray(X), dtype=dtype)
    y = torch.as_tensor(np.asarray(y), dtype=torch.long)
    w = torch.as_tensor(np.asarray(weights), dtype=dtype)
    S = model(X, Bcp, w, non_negative, softplus_kwargs)
    data = torch.nn.CrossEntropyLoss()(S, y)
    loss = data + lambda_L2 * l2_penalty(Bcp)
    loss.backward()
    return {"probs": S.detach().numpy(), "loss": loss.item(), "data_loss": data.item(),
            "grads": [A.grad.numpy().copy() for A in Bcp]}


def fit_adam(X, y, Bcp0, weights, non_negative, lambda_L2, max_iter, tol, patience, Adam_kwargs, group_lr=None,
             softplus_kwargs=None, dtype=torch.float32, loss_running=None):
    """The module's fit_Adam.  Returns dict(loss_running, Bcp, converged)."""
    Bcp = [torch.tensor(np.asarray(A), dtype=dtype, requires_grad=True) for A in Bcp0]
    X = torch.as_tensor(np.asarray(X), dtype=dtype)
    y = torch.as_tensor(np.asarray(y), dtype=torch.long)
    w = torch.as_tensor(np.asarray(weights), dtype=dtype)
    optimizer = torch.optim.Adam([{"params": Bcp[0], "lr": Adam_kwargs["lr"]},
                                  {"params": Bcp[1], "lr": Adam_kwargs["lr"]},
                                  {"params": Bcp[2], "lr": Adam_kwargs["lr"]}], **Adam_kwargs)
    sched = lr_schedule(group_lr, Adam_kwargs["lr"])
    loss_fn = torch.nn.CrossEntropyLoss()
    loss_running = [] if loss_running is None else loss_running
    converged = False
    for ii in range(max_iter):
        for g in range(3):
            for start, lr in sched[g]:
                if start == ii:
                    optimizer.param_groups[g]["lr"] = lr
        optimizer.zero_grad()
        S = model(X, Bcp, w, non_negative, softplus_kwargs)
        loss = loss_fn(S, y) + lambda_L2 * l2_penalty(Bcp)
        loss.backward()
        optimizer.step()
        loss_running.append(loss.item())
        if ii > patience and np.sum(np.abs(np.diff(loss_running[ii - patience:]))) < tol:
            converged = True
            break
    return {"loss_running": loss_running, "Bcp": [A.detach().numpy().copy() for A in Bcp], "converged": converged}


def fit_from_fixture(d, max_iter=None, dtype=torch.float32, group_lr="meta"):
    """fit_adam on a fixture's inputs and hyperparameters."""
    m = d["meta"]
    glr = m.get("group_lr") if group_lr == "meta" else group_lr
    return fit_adam(d["X_f32"], d["y"], d["Bcp0_list"], d["cp_weights"], m["non_negative"], m["lambda_L2"],
                    m["max_iter"] if max_iter is None else max_iter, m["tol"], m["patience"], m["adam_kwargs"],
                    group_lr=glr, softplus_kwargs=m["softplus_kwargs"], dtype=dtype)


def normwise_rel(a, b):
    a = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in a]) if isinstance(a, list) else \
        np.asarray(a, dtype=np.float64).ravel()
    b = np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in b]) if isinstance(b, list) else \
        np.asarray(b, dtype=np.float64).ravel()
    den = np.linalg.norm(b)
    return float(np.linalg.norm(a - b) / (den if den > 0 else 1.0))
