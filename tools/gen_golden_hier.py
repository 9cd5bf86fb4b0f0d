#!/usr/bin/env python3
"""Generate the hier_* golden fixtures by running the REFERENCE's hierarchical multinomial module
(build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_hier.py

Imports kimerein/tensor_regression's multinomial_tensor_regression_hierarchical from /root/reference
(read-only) with the tensorly stand-in of oracle/tensorly_standin on sys.path, like
tools/gen_golden.py, and writes inputs + outputs to tests/golden/hier_*.npz (data only).  X is
stored as float32 with its full mantissa.

Every Adam fixture holds: the inputs (X_f32, y, cp_weights, Bcp0), the model output, total loss and
autograd gradients at the initial point, a 10-iteration snapshot, the full trajectory of the
reference class's own fit_Adam, and `drift_loss` / `drift_factors`: the distance of that fp32 run
from the same algorithm in fp64 (max relative loss difference, normwise factor difference), the
fp64 run driving the reference's own `model` and `L2_penalty` with torch.optim.Adam param groups.
hier_group_lr has no class method to call (the reference's schedule is a commented-out line), so
both its fp32 and fp64 runs come from that driver.
"""
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF = "/root/reference"
sys.path.insert(0, os.path.join(REPO, "oracle", "tensorly_standin"))
sys.path.insert(0, REF)
sys.dont_write_bytecode = True

import tensorly as tl  # noqa: E402  (the stand-in)
import multinomial_tensor_regression_hierarchical as HIER  # noqa: E402  (reference)

OUT = os.path.join(REPO, "tests", "golden")


def save(name, **arrays):
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


def flat(Bcp):
    return np.concatenate([(A.detach().numpy() if isinstance(A, torch.Tensor) else np.asarray(A)).reshape(-1)
                           for A in Bcp])


def make_data(seed, shape, n_classes, center=False):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal(shape).astype(np.float32)
    if center:
        X = (X - X.mean(axis=1, keepdims=True)).astype(np.float32)
    y = rng.integers(0, n_classes, size=shape[0])
    y[:n_classes] = np.arange(n_classes)
    return X, y.astype(np.int64)


def drive(X, y, Bcp0, weights, non_negative, softplus_kwargs, lam, iters, tol, patience, adam_kwargs, group_lr,
          dtype):
    """The reference's fit_Adam loop (hierarchical…py:436-464) on its own model / L2_penalty in `dtype`,
    with `optimizer.param_groups[g]['lr'] = lr` at the top of the stated iterations."""
    tl.set_backend('pytorch')
    Bcp = [torch.tensor(np.asarray(A), dtype=dtype, requires_grad=True) for A in Bcp0]
    X = torch.as_tensor(X, dtype=dtype)
    y = torch.as_tensor(y, dtype=torch.long)
    w = torch.as_tensor(np.asarray(weights), dtype=dtype)
    optimizer = torch.optim.Adam([{'params': Bcp[0], 'lr': adam_kwargs['lr']},
                                  {'params': Bcp[1], 'lr': adam_kwargs['lr']},
                                  {'params': Bcp[2], 'lr': adam_kwargs['lr']}], **adam_kwargs)
    loss_fn = torch.nn.CrossEntropyLoss()
    losses, conv = [], False
    for ii in range(iters):
        if group_lr is not None:
            for g in range(3):
                for start, lr in group_lr[g]:
                    if start == ii:
                        optimizer.param_groups[g]['lr'] = lr
        optimizer.zero_grad()
        y_hat = HIER.model(X, Bcp, w, non_negative, softplus_kwargs=softplus_kwargs)
        loss = loss_fn(y_hat, y) + lam * HIER.L2_penalty(Bcp)
        loss.backward()
        optimizer.step()
        losses.append(loss.item())
        if ii > patience:
            if np.sum(np.abs(np.diff(losses[ii - patience:]))) < tol:
                conv = True
                break
    return losses, [A.detach().numpy().copy() for A in Bcp], conv


def adam_case(name, seed, shape, n_classes, rank, non_negative, lam, adam_kwargs, iters, tol=0.0, patience=10,
              cp_weights=None, center=False, group_lr=None):
    X, y = make_data(seed, shape, n_classes, center)
    w_arg = None if cp_weights is None else np.asarray(cp_weights, dtype=np.float32)

    def fresh():
        torch.manual_seed(seed)
        return HIER.CP_logistic_regression(X, y, rank=rank, non_negative=non_negative, weights=w_arg)

    m = fresh()
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    w = m.weights.detach().numpy().astype(np.float32)
    tl.set_backend('pytorch')
    y_hat = HIER.model(m.X, m.Bcp, m.weights, m.non_negative, softplus_kwargs=m.softplus_kwargs)
    loss = torch.nn.CrossEntropyLoss()(y_hat, m.y) + lam * HIER.L2_penalty(m.Bcp)
    loss.backward()
    grads0 = [A.grad.numpy().copy() for A in m.Bcp]
    for A in m.Bcp:
        A.grad = None
    if group_lr is None:
        m10 = fresh()
        m10.fit_Adam(lambda_L2=lam, max_iter=min(10, iters), tol=tol, patience=patience, verbose=False,
                     Adam_kwargs=dict(adam_kwargs))
        l10, B10 = list(m10.loss_running), [A.detach().numpy() for A in m10.Bcp]
        conv = m.fit_Adam(lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, verbose=False,
                          Adam_kwargs=dict(adam_kwargs))
        losses, Bf = list(m.loss_running), [A.detach().numpy() for A in m.Bcp]
    else:
        args = (X, y, Bcp0, w, m.non_negative, m.softplus_kwargs, lam)
        l10, B10, _ = drive(*args, min(10, iters), tol, patience, adam_kwargs, group_lr, torch.float32)
        losses, Bf, conv = drive(*args, iters, tol, patience, adam_kwargs, group_lr, torch.float32)
    l64, B64, conv64 = drive(X, y, Bcp0, w, m.non_negative, m.softplus_kwargs, lam, iters, tol, patience,
                             adam_kwargs, group_lr, torch.float64)
    n = min(len(losses), len(l64))
    a, b = np.asarray(losses[:n]), np.asarray(l64[:n])
    drift_loss = float(np.max(np.abs(a - b) / np.abs(b)))
    fa, fb = flat(Bf).astype(np.float64), flat(B64)
    drift_fac = float(np.linalg.norm(fa - fb) / np.linalg.norm(fb))
    print(f"{name}: {len(losses)} iterations, converged {conv} (fp64 {conv64}, {len(l64)}), "
          f"drift loss {drift_loss:.2e} factors {drift_fac:.2e}")
    meta = dict(model="hierarchical", seed=seed, shape=list(shape), n_classes=n_classes, rank=rank,
                non_negative=list(map(bool, m.non_negative)), lambda_L2=lam, adam_kwargs=adam_kwargs, max_iter=iters,
                tol=tol, patience=patience, softplus_kwargs=m.softplus_kwargs, center=center,
                group_lr=group_lr, factor_shapes=[list(a.shape) for a in Bcp0], torch=torch.__version__)
    save(name, X_f32=X, y=y, cp_weights=w, Bcp0=flat(Bcp0), probs0=y_hat.detach().numpy(),
         loss0=np.float64(loss.item()), grads0=flat(grads0), Bcp_10=flat(B10),
         loss_running_10=np.array(l10, dtype=np.float64), loss_running=np.array(losses, dtype=np.float64),
         Bcp_final=flat(Bf), converged=np.int32(conv), drift_loss=np.float64(drift_loss),
         drift_factors=np.float64(drift_fac), meta=np.array(json.dumps(meta)))


def lbfgs_case(name, seed, shape, n_classes, rank, lam, iters, lbfgs_kwargs, logging_interval=1):
    X, y = make_data(seed, shape, n_classes)
    torch.manual_seed(seed)
    m = HIER.CP_logistic_regression(X, y, rank=rank)
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    conv = m.fit(lambda_L2=lam, max_iter=iters, tol=0.0, patience=100, verbose=False,
                 running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
    pred = m.predict()
    cm, acc = m.make_confusion_matrix(prob_or_pred='pred')
    meta = dict(model="hierarchical_lbfgs", seed=seed, shape=list(shape), n_classes=n_classes, rank=rank,
                lambda_L2=lam, max_iter=iters, lbfgs_kwargs=lbfgs_kwargs, logging_interval=logging_interval,
                non_negative=[False] * len(shape), softplus_kwargs=m.softplus_kwargs,
                factor_shapes=[list(a.shape) for a in Bcp0], torch=torch.__version__)
    save(name, X_f32=X, y=y, cp_weights=m.weights.numpy(), Bcp0=flat(Bcp0),
         loss_running=np.array(m.loss_running, dtype=np.float64), Bcp_final=flat(m.Bcp), converged=np.int32(conv),
         probs_final=pred[0], pred_final=pred[1].astype(np.int64), n_predict_outputs=np.int32(len(pred)),
         confusion=cm, accuracy=np.float64(acc), meta=np.array(json.dumps(meta)))


def init_rng_case(name):
    """The constructor's RNG draws (hierarchical…py:283-288 -> make_BcpInit :111): seed, arguments, Bcp."""
    cases = [dict(seed=3, shape=[9, 4, 5], n_classes=3, rank=2, non_negative=False, scale=1),
             dict(seed=4, shape=[12, 3, 6], n_classes=4, rank=5, non_negative=True, scale=0.5),
             dict(seed=5, shape=[8, 2, 3, 4], n_classes=2, rank=3, non_negative=[True, False, False, True], scale=2)]
    arrays = {}
    for k, c in enumerate(cases):
        y = np.arange(c["shape"][0]) % c["n_classes"]
        torch.manual_seed(c["seed"])
        m = HIER.CP_logistic_regression(np.zeros(c["shape"], np.float32), y, rank=c["rank"],
                                        non_negative=c["non_negative"], Bcp_init_scale=c["scale"])
        arrays[f"Bcp_{k}"] = flat(m.Bcp)
        arrays[f"after_{k}"] = torch.rand(4).numpy()  # the generator's state after the constructor
        c["factor_shapes"] = [list(A.shape) for A in m.Bcp]
        c["weights"] = m.weights.tolist()
        c["softplus_kwargs"] = m.softplus_kwargs
    save(name, meta=np.array(json.dumps(dict(cases=cases, torch=torch.__version__))), **arrays)


def main():
    os.makedirs(OUT, exist_ok=True)
    # kim_MultinomialTensorRegression.ipynb: shape and hyperparameters, X mean-subtracted along axis 1
    adam_case("hier_kim", 71, (227, 8, 12), 4, 6, [True] * 3, 0.005,
              {'lr': 0.05, 'amsgrad': True}, 150, tol=1e-6, patience=100, center=True)
    adam_case("hier_signed", 72, (61, 5, 7), 3, 2, False, 0.01, {'lr': 0.02}, 60, tol=0.0, patience=10)
    adam_case("hier_cpw", 73, (50, 4, 6), 3, 3, [True, False, True], 0.01, {'lr': 0.02, 'amsgrad': True}, 40,
              cp_weights=[0.5, 1.5, 1.0])
    adam_case("hier_converge", 74, (48, 4, 5), 3, 2, [True] * 3, 0.01, {'lr': 0.01, 'amsgrad': True}, 400,
              tol=2e-3, patience=5)
    adam_case("hier_wd", 75, (55, 6, 3), 2, 3, [False, True, False], 0.02,
              {'lr': 0.01, 'weight_decay': 0.01, 'betas': (0.8, 0.99), 'eps': 1e-6}, 40)
    adam_case("hier_4d", 76, (40, 3, 4, 5), 3, 2, [True, False, True, False], 0.01, {'lr': 0.02, 'amsgrad': True}, 40)
    # group learning rates set at stated iterations, the class factor's group at lr 0 for the first
    # stretch.  The rates are kept moderate: at 0.03 / 0.05 / 0.03 over 90 iterations the reference's
    # own fp32 algorithm with only the sample order permuted (six orders) ended up to 2.6e-5 normwise
    # from its fp64 run, past the 1e-5 bar of the GPU tests; at these settings every order stays
    # within 8e-7.
    adam_case("hier_group_lr", 77, (70, 6, 5), 3, 3, [True] * 3, 0.005, {'lr': 0.02, 'amsgrad': True}, 60,
              group_lr=[[(0, 0.02), (40, 0.005)], [(0, 0.03)], [(0, 0.0), (20, 0.02), (50, 0.002)]])
    # five logged steps: over them the reference's own fp32 run with only the sample order permuted
    # (six orders) stays within 5e-7 of its fp64 run; from the seventh step on it is 1e-5 .. 3e-5 away,
    # past the 1e-5 bar of the GPU test (multinomial LBFGS is ill-conditioned in fp32)
    lbfgs_case("hier_lbfgs", 78, (96, 6, 5), 4, 3, 1e-2, 5,
               {'lr': 0.5, 'max_iter': 3, 'history_size': 10, 'line_search_fn': None})
    init_rng_case("hier_init_rng")


if __name__ == "__main__":
    main()
