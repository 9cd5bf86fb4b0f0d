#!/usr/bin/env python3
"""Generate golden fixtures by running the REFERENCE itself (build container only).

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden.py [--kat]

Imports kimerein/tensor_regression from /root/reference (read-only) with the tensorly stand-in
of oracle/tensorly_standin on sys.path, runs small seeded cases through the reference's own
classes and functions, and writes inputs + outputs to tests/golden/*.npz (data only: nothing
of the reference's source travels).  Inputs are exactly representable (X = int8 / 8), so the
fixtures stay small and any consumer reconstructs bit-identical fp32 inputs.

--kat additionally replays the two notebook known-answer traces (KAT-1: LBFGS fp64,
demo_TensorRegression.ipynb; KAT-2: Adam-amsgrad fp32, demo_MultinomialTensorRegression.ipynb)
through the reference + stand-in and records the agreement in tests/golden/kat_replay.json.
"""
import argparse
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

import standard_tensor_regression as STR  # noqa: E402  (reference)
import multinomial_tensor_regression as MTR  # noqa: E402  (reference)
import spectral_tensor_regression as SPR  # noqa: E402  (reference)
import util as RUTIL  # noqa: E402  (reference util.py: WindowedDataset)

OUT = os.path.join(REPO, "tests", "golden")


def exact_X(rng, shape):
    q = rng.integers(-8, 9, size=shape).astype(np.int8)
    return q, torch.tensor(q.astype(np.float32) / 8.0)


PART_BYTES = 896 * 1024  # no committed file above 1 MiB


def save(name, **arrays):
    # a full-mantissa X of more than 1 MiB (it barely compresses) goes beside the .npz in row
    # blocks, <name>.X_f32.<k>.npy; tests/golden_util.py puts them back together
    X = arrays.get("X_f32")
    if X is not None and X.nbytes > (1 << 20):
        del arrays["X_f32"]
        for k, blk in enumerate(np.array_split(X, -(-X.nbytes // PART_BYTES))):
            np.save(os.path.join(OUT, f"{name}.X_f32.{k}.npy"), blk)
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **arrays)
    print("wrote", path, os.path.getsize(path), "bytes")


def planted_y(rng, Xq, rank):
    """configs[0] recipe: y = <X, [[A*]]> + 0.1 N(0,1) with A* ~ N(0,1) of rank `rank`,
    evaluated in fp64 from the exact int8/8 X, stored as fp32."""
    A = [rng.standard_normal((d, rank)) for d in Xq.shape[1:]]
    B = A[0]
    for a in A[1:]:
        B = (B[:, None, :] * a[None, :, :]).reshape(-1, rank)
    Bd = B.sum(1)
    Xf = Xq.reshape(Xq.shape[0], -1).astype(np.float64) / 8.0
    return torch.tensor((Xf @ Bd + 0.1 * rng.standard_normal(Xq.shape[0])).astype(np.float32))


def linear_case(name, seed, shape, rank, non_negative, bias_init, lam, adam_kwargs, iters, tol=0.0, patience=10,
                softplus=None, second_fit=0, planted=False):
    rng = np.random.default_rng(seed)
    Xq, X = exact_X(rng, shape)
    if planted:
        y = planted_y(rng, Xq, rank)
    else:
        y = torch.tensor(rng.standard_normal(shape[0]).astype(np.float32))
    torch.manual_seed(seed)
    m = STR.CP_linear_regression(X.shape, rank=rank, non_negative=non_negative, bias_init=bias_init,
                                 softplus_kwargs=softplus)
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    b0 = m.bias.detach().numpy().copy()
    # one forward + loss + backward at the initial point (standard…py:459-462)
    y_hat = STR.lin_model(X, m.Bcp, m.weights, m.non_negative, m.bias, softplus_kwargs=m.softplus_kwargs)
    loss = torch.nn.MSELoss()(y_hat, y) + lam * STR.L2_penalty(m.Bcp)
    loss.backward()
    grads = [A.grad.numpy().copy() for A in m.Bcp]
    bgrad = m.bias.grad.numpy().copy()
    for A in m.Bcp:
        A.grad = None
    m.bias.grad = None
    # 10-iteration snapshot from the same initial point (a fresh model, same seed)
    torch.manual_seed(seed)
    m10 = STR.CP_linear_regression(X.shape, rank=rank, non_negative=non_negative, bias_init=bias_init,
                                   softplus_kwargs=softplus)
    m10.fit_Adam(X, y, lambda_L2=lam, max_iter=min(10, iters), tol=tol, patience=patience, verbose=False,
                 Adam_kwargs=dict(adam_kwargs))
    conv = m.fit_Adam(X, y, lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, verbose=False,
                      Adam_kwargs=dict(adam_kwargs))
    out = dict(
        Bcp_10=np.concatenate([A.detach().numpy().reshape(-1) for A in m10.Bcp]),
        bias_10=m10.bias.detach().numpy().copy(), loss_running_10=np.array(m10.loss_running),
        X_q=Xq, y=y.numpy(), Bcp0=np.concatenate([a.reshape(-1) for a in Bcp0]), bias0=b0,
        y_hat0=y_hat.detach().numpy(), loss0=np.float64(loss.item()),
        grads0=np.concatenate([g.reshape(-1) for g in grads]), bias_grad0=bgrad,
        loss_running=np.array(m.loss_running, dtype=np.float64),
        Bcp_final=np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp]),
        bias_final=m.bias.detach().numpy().copy(), converged=np.int32(conv))
    if second_fit:
        m.fit_Adam(X, y, lambda_L2=lam, max_iter=second_fit, tol=tol, patience=patience, verbose=False,
                   Adam_kwargs=dict(adam_kwargs))
        out.update(loss_running2=np.array(m.loss_running, dtype=np.float64),
                   Bcp_final2=np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp]),
                   bias_final2=m.bias.detach().numpy().copy())
    meta = dict(model="linear", seed=seed, shape=list(shape), rank=rank, non_negative=list(map(bool, non_negative)),
                bias_init=bias_init, lambda_L2=lam, adam_kwargs=adam_kwargs, max_iter=iters, tol=tol,
                patience=patience, softplus_kwargs=m.softplus_kwargs, second_fit=second_fit, planted=planted,
                factor_shapes=[list(a.shape) for a in Bcp0], torch=torch.__version__)
    out["meta"] = np.array(json.dumps(meta))
    save(name, **out)


def linear_lbfgs_case(name, seed, shape, rank, lam, iters, lbfgs_kwargs, logging_interval=1):
    rng = np.random.default_rng(seed)
    Xq, X = exact_X(rng, shape)
    y = torch.tensor(rng.standard_normal(shape[0]).astype(np.float32))
    torch.manual_seed(seed)
    m = STR.CP_linear_regression(X.shape, rank=rank)
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    conv = m.fit(X, y, lambda_L2=lam, max_iter=iters, tol=0.0, patience=100, verbose=False,
                 running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
    meta = dict(model="linear_lbfgs", seed=seed, shape=list(shape), rank=rank, lambda_L2=lam, max_iter=iters,
                lbfgs_kwargs=lbfgs_kwargs, logging_interval=logging_interval,
                factor_shapes=[list(a.shape) for a in Bcp0], torch=torch.__version__)
    save(name, X_q=Xq, y=y.numpy(), Bcp0=np.concatenate([a.reshape(-1) for a in Bcp0]),
         loss_running=np.array(m.loss_running), Bcp_final=np.concatenate(
             [A.detach().numpy().reshape(-1) for A in m.Bcp]), bias_final=m.bias.detach().numpy(),
         converged=np.int32(conv), meta=np.array(json.dumps(meta)))


def mnl_case(name, seed, shape, n_classes, rank, non_negative, class_w, lam, adam_kwargs, iters, tol=0.0,
             patience=10, x_scale=None):
    """x_scale: X = N(0, 1) * x_scale in float32 (full mantissa, stored as X_f32) instead of the exact
    int8 / 8 X: every bf16 piece of a split kernel's X representation then carries data, at a
    magnitude far from 1 (the f16 second piece of round 5's split body lost precision below
    |x| = 2^-5)."""
    rng = np.random.default_rng(seed)
    if x_scale is None:
        Xq, X = exact_X(rng, shape)
    else:
        Xq = None
        X = torch.tensor((rng.standard_normal(shape) * x_scale).astype(np.float32))
    y = rng.integers(0, n_classes, size=shape[0])
    y[:n_classes] = np.arange(n_classes)  # every class present (n_classes = len(unique(y)))
    torch.manual_seed(seed)
    m = MTR.CP_logistic_regression(X.numpy(), y, rank=rank, non_negative=non_negative)
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    S = MTR.model(m.X, m.Bcp, m.weights, m.non_negative, softplus_kwargs=m.softplus_kwargs)
    loss_fn = torch.nn.CrossEntropyLoss(weight=torch.as_tensor(class_w, dtype=torch.float32))
    loss = loss_fn(S, m.y) + lam * MTR.L2_penalty(m.Bcp)
    loss.backward()
    grads = [A.grad.numpy().copy() for A in m.Bcp]
    for A in m.Bcp:
        A.grad = None
    torch.manual_seed(seed)
    m10 = MTR.CP_logistic_regression(X.numpy(), y, rank=rank, non_negative=non_negative)
    m10.fit_Adam(lambda_L2=lam, max_iter=min(10, iters), tol=tol, patience=patience, weights=np.asarray(class_w),
                 verbose=False, Adam_kwargs=dict(adam_kwargs))
    conv = m.fit_Adam(lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, weights=np.asarray(class_w),
                      verbose=False, Adam_kwargs=dict(adam_kwargs))
    meta = dict(model="multinomial", seed=seed, shape=list(shape), n_classes=n_classes, rank=rank,
                non_negative=list(map(bool, non_negative)), class_weights=list(map(float, class_w)), lambda_L2=lam,
                adam_kwargs=adam_kwargs, max_iter=iters, tol=tol, patience=patience,
                softplus_kwargs=m.softplus_kwargs, factor_shapes=[list(a.shape) for a in Bcp0],
                torch=torch.__version__)
    xarr = dict(X_q=Xq) if Xq is not None else dict(X_f32=X.numpy())
    save(name, **xarr, y=y.astype(np.int64), Bcp0=np.concatenate([a.reshape(-1) for a in Bcp0]),
         probs0=S.detach().numpy(), loss0=np.float64(loss.item()),
         grads0=np.concatenate([g.reshape(-1) for g in grads]),
         loss_running=np.array(m.loss_running, dtype=np.float64),
         Bcp_final=np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp]), converged=np.int32(conv),
         Bcp_10=np.concatenate([A.detach().numpy().reshape(-1) for A in m10.Bcp]),
         loss_running_10=np.array(m10.loss_running), meta=np.array(json.dumps(meta)))


def f64_case(name, seed, shape, rank, lam, iters, adam_kwargs=None, lbfgs_kwargs=None, non_negative=None,
             logging_interval=1):
    """CP_linear_regression(dtype=torch.float64) (standard…py:206): fit_Adam or fit (LBFGS) in
    float64 through the reference, plus one loss + gradient at the initial point."""
    rng = np.random.default_rng(seed)
    Xq, X32 = exact_X(rng, shape)
    X = X32.double()
    y = torch.tensor(rng.standard_normal(shape[0]))
    nn = non_negative if non_negative is not None else [False] * len(shape)
    torch.manual_seed(seed)
    m = STR.CP_linear_regression(X.shape, dtype=torch.float64, rank=rank, non_negative=nn, bias_init=0.1)
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    b0 = m.bias.detach().numpy().copy()
    y_hat = STR.lin_model(X, m.Bcp, m.weights, m.non_negative, m.bias, softplus_kwargs=m.softplus_kwargs)
    loss = torch.nn.MSELoss()(y_hat, y) + lam * STR.L2_penalty(m.Bcp)
    loss.backward()
    grads = [A.grad.numpy().copy() for A in m.Bcp]
    bgrad = m.bias.grad.numpy().copy()
    for A in m.Bcp:
        A.grad = None
    m.bias.grad = None
    if lbfgs_kwargs is not None:
        conv = m.fit(X, y, lambda_L2=lam, max_iter=iters, tol=0.0, patience=100, verbose=False,
                     running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
    else:
        conv = m.fit_Adam(X, y, lambda_L2=lam, max_iter=iters, tol=0.0, patience=10, verbose=False,
                          Adam_kwargs=dict(adam_kwargs))
    meta = dict(model="linear_f64", seed=seed, shape=list(shape), rank=rank, non_negative=list(map(bool, nn)),
                lambda_L2=lam, max_iter=iters, adam_kwargs=adam_kwargs, lbfgs_kwargs=lbfgs_kwargs,
                logging_interval=logging_interval, softplus_kwargs=m.softplus_kwargs,
                factor_shapes=[list(a.shape) for a in Bcp0], torch=torch.__version__)
    save(name, X_q=Xq, y=y.numpy(), Bcp0=np.concatenate([a.reshape(-1) for a in Bcp0]), bias0=b0,
         y_hat0=y_hat.detach().numpy(), loss0=np.float64(loss.item()),
         grads0=np.concatenate([g.reshape(-1) for g in grads]), bias_grad0=bgrad,
         loss_running=np.array(m.loss_running, dtype=np.float64),
         Bcp_final=np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp]),
         bias_final=m.bias.detach().numpy().copy(), converged=np.int32(conv), meta=np.array(json.dumps(meta)))


def mnl_lbfgs_case(name, seed, shape, n_classes, rank, class_w, lam, iters, lbfgs_kwargs, logging_interval=1):
    """CP_logistic_regression.fit (LBFGS, multinomial…py:291-387): logged loss = data CE only (:372)."""
    rng = np.random.default_rng(seed)
    Xq, X = exact_X(rng, shape)
    y = rng.integers(0, n_classes, size=shape[0])
    y[:n_classes] = np.arange(n_classes)
    torch.manual_seed(seed)
    m = MTR.CP_logistic_regression(X.numpy(), y, rank=rank)
    Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
    conv = m.fit(lambda_L2=lam, max_iter=iters, tol=0.0, patience=100, weights=np.asarray(class_w), verbose=False,
                 running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
    meta = dict(model="multinomial_lbfgs", seed=seed, shape=list(shape), n_classes=n_classes, rank=rank,
                class_weights=list(map(float, class_w)), lambda_L2=lam, max_iter=iters, lbfgs_kwargs=lbfgs_kwargs,
                logging_interval=logging_interval, non_negative=[False] * (len(shape)),
                softplus_kwargs=m.softplus_kwargs, factor_shapes=[list(a.shape) for a in Bcp0],
                torch=torch.__version__)
    save(name, X_q=Xq, y=y.astype(np.int64), Bcp0=np.concatenate([a.reshape(-1) for a in Bcp0]),
         loss_running=np.array(m.loss_running, dtype=np.float64),
         Bcp_final=np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp]), converged=np.int32(conv),
         meta=np.array(json.dumps(meta)))


def windowed_case(name, seed, series_shape, win_range, rank, lam, adam_kwargs, iters, n_classes=0):
    """Windowed data path (util.py:67-98): the reference's WindowedDataset over an untiled series,
    every usable window materialised in usable_idx order and fitted by the reference's fit_Adam
    (standard…py:400-476, or multinomial…py:389-471 when n_classes > 0).  The fixture keeps only
    the untiled series; consumers rebuild the windows (windowed_view / HostStream)."""
    rng = np.random.default_rng(seed)
    Sq, S = exact_X(rng, series_shape)
    T = series_shape[0]
    if n_classes:
        ys = rng.integers(0, n_classes, size=T)
        ys[-win_range[0]:-win_range[0] + n_classes] = np.arange(n_classes)  # every class in a usable window
        ys_t = torch.tensor(ys)
    else:
        ys_t = torch.tensor(rng.standard_normal(T).astype(np.float32))
    ds = RUTIL.WindowedDataset(S, ys_t, win_range)
    items = [ds[int(i)] for i in ds.usable_idx]
    X = torch.stack([a for a, _ in items])
    y = torch.stack([b for _, b in items])
    if n_classes:
        y_np = y.numpy().astype(np.int64)
        assert len(np.unique(y_np)) == n_classes
        torch.manual_seed(seed)
        m = MTR.CP_logistic_regression(X.numpy(), y_np, rank=rank)
        Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
        Sp = MTR.model(m.X, m.Bcp, m.weights, m.non_negative, softplus_kwargs=m.softplus_kwargs)
        loss = torch.nn.CrossEntropyLoss(weight=torch.ones(n_classes))(Sp, m.y) + lam * MTR.L2_penalty(m.Bcp)
        loss.backward()
        grads = [A.grad.numpy().copy() for A in m.Bcp]
        for A in m.Bcp:
            A.grad = None
        torch.manual_seed(seed)
        m10 = MTR.CP_logistic_regression(X.numpy(), y_np, rank=rank)
        m10.fit_Adam(lambda_L2=lam, max_iter=min(10, iters), tol=0.0, patience=10, weights=np.ones(n_classes),
                     verbose=False, Adam_kwargs=dict(adam_kwargs))
        conv = m.fit_Adam(lambda_L2=lam, max_iter=iters, tol=0.0, patience=10, weights=np.ones(n_classes),
                          verbose=False, Adam_kwargs=dict(adam_kwargs))
        extra = dict(probs0=Sp.detach().numpy(), y_series=ys.astype(np.int64))
        bias = {}
    else:
        torch.manual_seed(seed)
        m = STR.CP_linear_regression(X.shape, rank=rank)
        Bcp0 = [A.detach().numpy().copy() for A in m.Bcp]
        b0 = m.bias.detach().numpy().copy()
        yh = STR.lin_model(X, m.Bcp, m.weights, m.non_negative, m.bias, softplus_kwargs=m.softplus_kwargs)
        loss = torch.nn.MSELoss()(yh, y) + lam * STR.L2_penalty(m.Bcp)
        loss.backward()
        grads = [A.grad.numpy().copy() for A in m.Bcp]
        bgrad = m.bias.grad.numpy().copy()
        for A in m.Bcp:
            A.grad = None
        m.bias.grad = None
        torch.manual_seed(seed)
        m10 = STR.CP_linear_regression(X.shape, rank=rank)
        m10.fit_Adam(X, y, lambda_L2=lam, max_iter=min(10, iters), tol=0.0, patience=10, verbose=False,
                     Adam_kwargs=dict(adam_kwargs))
        conv = m.fit_Adam(X, y, lambda_L2=lam, max_iter=iters, tol=0.0, patience=10, verbose=False,
                          Adam_kwargs=dict(adam_kwargs))
        extra = dict(y_hat0=yh.detach().numpy(), y_series=ys_t.numpy(), bias0=b0, bias_grad0=bgrad,
                     bias_10=m10.bias.detach().numpy().copy(), bias_final=m.bias.detach().numpy().copy())
    meta = dict(model="windowed_" + ("multinomial" if n_classes else "linear"), seed=seed,
                series_shape=list(series_shape), win_range=list(win_range), n_windows=len(items),
                window_shape=list(X.shape[1:]), n_classes=n_classes, rank=rank, lambda_L2=lam,
                adam_kwargs=adam_kwargs, max_iter=iters, tol=0.0, patience=10,
                non_negative=list(map(bool, m.non_negative)), softplus_kwargs=m.softplus_kwargs,
                factor_shapes=[list(a.shape) for a in Bcp0], torch=torch.__version__)
    save(name, X_q=Sq, Bcp0=np.concatenate([a.reshape(-1) for a in Bcp0]), loss0=np.float64(loss.item()),
         grads0=np.concatenate([g.reshape(-1) for g in grads]),
         Bcp_10=np.concatenate([A.detach().numpy().reshape(-1) for A in m10.Bcp]),
         loss_running_10=np.array(m10.loss_running, dtype=np.float64),
         loss_running=np.array(m.loss_running, dtype=np.float64),
         Bcp_final=np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp]), converged=np.int32(conv),
         meta=np.array(json.dumps(meta)), **extra)


def _flat(ts):
    ts = [t.detach().numpy() if isinstance(t, torch.Tensor) else t for t in ts]
    return np.concatenate([t.reshape(-1) for t in ts]) if ts else np.zeros(0, np.float32)


def spectral_case(name, seed, shape, n_out, rank_normal, rank_spectral, n_complex_dim, non_negative, lam,
                  adam_kwargs, iters, tol=0.0, patience=10, softplus=None, nan_y=False, lbfgs_kwargs=None,
                  logging_interval=1, full_mantissa=False):
    """spectral_tensor_regression.CP_linear_regression: one forward/loss/backward at the init point
    (fit model = lin_model + stepwise_spectral_model, spectral…py:716-720), predict (spectral_model,
    :959-960), a 10-iteration and a full fit_Adam run (or LBFGS fit when lbfgs_kwargs is given).
    full_mantissa: X = |N(0,1)| in float32 (all 24 significand bits in use, |rfft|-like magnitudes),
    stored as X_f32 instead of the int8/8 X_q, so a kernel that rounds X (e.g. to bf16 pieces)
    cannot pass on exactly representable inputs."""
    rng = np.random.default_rng(seed)
    if full_mantissa:
        Xf = np.abs(rng.standard_normal(shape)).astype(np.float32)
        Xq, X = None, torch.tensor(Xf)
    else:
        Xq, X = exact_X(rng, shape)
    y = torch.tensor(rng.standard_normal((shape[0], n_out)).astype(np.float32))
    if nan_y:
        y[3, 0] = float("nan")

    def make():
        torch.manual_seed(seed)
        return SPR.CP_linear_regression(X.shape, y.shape, rank_normal=rank_normal, rank_spectral=rank_spectral,
                                        non_negative=non_negative, n_complex_dim=n_complex_dim,
                                        softplus_kwargs=softplus)

    m = make()
    Bn0, Bc0 = _flat(m.Bcp_n), _flat(m.Bcp_c)
    w = m.weights
    y_hat = (SPR.lin_model(X, m.Bcp_n, w[:m.rank_normal], m.non_negative, m.bias, softplus_kwargs=m.softplus_kwargs) +
             SPR.stepwise_spectral_model(X, m.Bcp_c, w[m.rank_normal:], m.non_negative, m.bias,
                                         softplus_kwargs=m.softplus_kwargs))
    loss = torch.nn.MSELoss()(y_hat, y) + lam * (SPR.L2_penalty(m.Bcp_n) + SPR.L2_penalty(m.Bcp_c))
    loss.backward()
    gn = _flat([A.grad for A in m.Bcp_n if A.grad is not None]) if rank_normal else np.zeros(0, np.float32)
    gc_ = _flat([A.grad for A in m.Bcp_c if A.grad is not None]) if rank_spectral else np.zeros(0, np.float32)
    bg = m.bias.grad.numpy().copy()
    pred0 = m.predict(X).numpy()
    out = dict(y=y.numpy(), Bcp_n0=Bn0, Bcp_c0=Bc0, y_hat0=y_hat.detach().numpy(),
               loss0=np.float64(loss.item()), grads_n0=gn, grads_c0=gc_, bias_grad0=bg, predict0=pred0)
    if full_mantissa:
        out["X_f32"] = X.numpy()
    else:
        out["X_q"] = Xq
    if lbfgs_kwargs is None:
        m10 = make()
        m10.fit_Adam(X, y, lambda_L2=lam, max_iter=min(10, iters), tol=tol, patience=patience, verbose=False,
                     Adam_kwargs=dict(adam_kwargs))
        out.update(Bcp_n_10=_flat(m10.Bcp_n), Bcp_c_10=_flat(m10.Bcp_c), bias_10=m10.bias.detach().numpy().copy(),
                   loss_running_10=np.array(m10.loss_running, dtype=np.float64))
        m = make()
        conv = m.fit_Adam(X, y, lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, verbose=False,
                          Adam_kwargs=dict(adam_kwargs))
    else:
        m = make()
        conv = m.fit(X, y, lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, verbose=False,
                     running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
    out.update(loss_running=np.array(m.loss_running, dtype=np.float64), Bcp_n_final=_flat(m.Bcp_n),
               Bcp_c_final=_flat(m.Bcp_c), bias_final=m.bias.detach().numpy().copy(), converged=np.int32(conv),
               predict_final=m.predict(X).numpy())
    meta = dict(model="spectral", seed=seed, shape=list(shape), n_out=n_out, rank_normal=rank_normal,
                rank_spectral=rank_spectral, n_complex_dim=n_complex_dim, non_negative=m.non_negative,
                lambda_L2=lam, adam_kwargs=adam_kwargs, lbfgs_kwargs=lbfgs_kwargs, logging_interval=logging_interval,
                max_iter=iters, tol=tol, patience=patience, softplus_kwargs=m.softplus_kwargs, nan_y=nan_y,
                full_mantissa=full_mantissa, factor_shapes_n=[list(a.shape) for a in m.Bcp_n], factor_shapes_c=[list(a.shape) for a in m.Bcp_c],
                torch=torch.__version__)
    out["meta"] = np.array(json.dumps(meta))
    save(name, **out)


def init_case(name):
    """make_BcpInit RNG parity: the reference's initialisers for fixed seeds."""
    out = {}
    for seed, dims, rank, nn, scale in [(0, [7, 5], 3, [False, False], 1.0), (1, [6, 4, 3], 2, [True, False, True], 0.5),
                                        (2, [1, 9], 2, [True, True], 1.0)]:
        torch.manual_seed(seed)
        B = STR.make_BcpInit(dims, rank, nn, scale=scale)
        out[f"std_{seed}"] = np.concatenate([b.numpy().reshape(-1) for b in B])
        torch.manual_seed(seed)
        M = MTR.make_BcpInit(dims, rank, nn, scale=scale)
        out[f"mnl_{seed}"] = np.concatenate([b.detach().numpy().reshape(-1) for b in M])
    save(name, **out)


def kat_replay():
    import scipy.signal
    sys.path.insert(0, os.path.join(REPO, "tests"))
    from kat_data import kat_inputs, KAT1_TRACE, KAT2_TRACE  # noqa: E402
    res = {}
    # KAT-2 (multinomial, Adam amsgrad, fp32): notebook cells 2/4, one extra make_BcpInit draw
    X, y = kat_inputs("kat2")
    MTR.make_BcpInit(np.concatenate((X.shape[1:], [5])), 4, [False] * 3, scale=1)
    m = MTR.CP_logistic_regression(X, y, rank=4, non_negative=[False] * 3, Bcp_init_scale=1,
                                   softplus_kwargs={'beta': 50, 'threshold': 1})
    m.fit_Adam(lambda_L2=0.01, max_iter=len(KAT2_TRACE), tol=1e-6, patience=100, weights=np.ones(5),
               Adam_kwargs={'lr': 0.01, 'amsgrad': True})
    rel = np.max(np.abs(np.array(m.loss_running) - KAT2_TRACE) / np.abs(KAT2_TRACE))
    res["kat2_max_rel"] = float(rel)
    res["kat2_loss_running"] = m.loss_running
    del m, X
    # KAT-1 (linear, LBFGS, fp64)
    X, y = kat_inputs("kat1")
    m = STR.CP_linear_regression(X.shape, dtype=X.dtype, rank=10, non_negative=[False, False], Bcp_init_scale=0.005,
                                 softplus_kwargs={'beta': 50, 'threshold': 1})
    m.fit(X, y, lambda_L2=1e-5, max_iter=200, tol=1e-50, patience=10, running_loss_logging_interval=1,
          LBFGS_kwargs={'lr': 1, 'max_iter': 20, 'max_eval': None, 'tolerance_grad': 1e-07,
                        'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})
    n = min(len(m.loss_running), len(KAT1_TRACE))
    rel = np.max(np.abs(np.array(m.loss_running[:n]) - KAT1_TRACE[:n]) / np.abs(KAT1_TRACE[:n]))
    res["kat1_max_rel"] = float(rel)
    res["kat1_len"] = len(m.loss_running)
    res["kat1_loss_running"] = m.loss_running
    with open(os.path.join(OUT, "kat_replay.json"), "w") as f:
        json.dump(res, f, indent=1)
    print("KAT replay:", {k: v for k, v in res.items() if "rel" in k or "len" in k})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kat", action="store_true")
    ap.add_argument("--only", default=None,
                    help="generate only the cases whose name starts with one of these comma-separated prefixes")
    args = ap.parse_args()
    os.makedirs(OUT, exist_ok=True)
    torch.set_num_threads(1)  # fixed summation order for the golden outputs
    if args.only:
        global save
        _save = save

        def save(name, **arrays):  # noqa: F811
            if name.startswith(tuple(args.only.split(","))):
                _save(name, **arrays)
    adam = {'lr': 0.01}
    linear_case("lin_basic", 11, (64, 8, 4), 2, [False, False, False], 0.3, 0.01, adam, 50)
    linear_case("lin_nonneg_amsgrad_wd", 12, (96, 12, 8), 3, [True, False, True], -0.2, 0.05,
                {'lr': 0.02, 'amsgrad': True, 'weight_decay': 0.01, 'betas': (0.8, 0.99), 'eps': 1e-6}, 50)
    linear_case("lin_4d_unaligned", 13, (40, 4, 3, 5), 4, [False, True, False, False], 0.0, 0.01, adam, 50)
    linear_case("lin_fused_shape", 14, (256, 16, 16), 8, [False, False, False], 0.1, 0.01, adam, 50)
    linear_case("lin_one_mode", 15, (64, 40), 2, [False, False], 0.0, 0.01, adam, 30)
    linear_case("lin_converge", 16, (64, 8, 4), 2, [False, False, False], 0.0, 0.01, {'lr': 0.001}, 400,
                tol=0.05, patience=5, second_fit=30)
    linear_case("lin_softplus_kw", 17, (48, 6, 4), 2, [True, True, False], 0.0, 0.01, adam, 30,
                softplus={'beta': 5, 'threshold': 2})
    linear_lbfgs_case("lin_lbfgs", 18, (64, 8, 4), 2, 1e-3, 6,
                      {'lr': 1, 'max_iter': 20, 'max_eval': None, 'tolerance_grad': 1e-07,
                       'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})
    # BASELINE configs[0]: X (1024, 32, 16), rank 2, planted y, 200 Adam iterations
    linear_case("lin_cfg1", 41, (1024, 32, 16), 2, [False, False, False], 0.0, 0.01, adam, 200, planted=True)
    linear_case("lin_cfg1_amsgrad", 41, (1024, 32, 16), 2, [False, False, False], 0.0, 0.01,
                {'lr': 0.01, 'amsgrad': True}, 200, planted=True)
    mnl_lbfgs_case("mnllbfgs_basic", 25, (128, 8, 4), 3, 2, [1.0, 1.0, 1.0], 1e-3, 6,
                   {'lr': 1, 'max_iter': 20, 'max_eval': None, 'tolerance_grad': 1e-07,
                    'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})
    # well-conditioned: few inner iterations, no line search -> the fp32 trajectory is reproducible
    mnl_lbfgs_case("mnllbfgs_weighted", 26, (96, 6, 5), 4, 3, [0.5, 2.0, 1.0, 1.5], 1e-2, 8,
                   {'lr': 0.05, 'max_iter': 3, 'max_eval': None, 'tolerance_grad': 1e-07,
                    'tolerance_change': 1e-09, 'history_size': 10, 'line_search_fn': None}, logging_interval=2)
    f64_case("f64_adam", 61, (200, 12, 9), 3, 0.01, 60, adam_kwargs={'lr': 0.02, 'amsgrad': True},
             non_negative=[True, False, False])
    f64_case("f64_lbfgs", 62, (150, 10, 8), 2, 1e-3, 8,
             lbfgs_kwargs={'lr': 1, 'max_iter': 20, 'max_eval': None, 'tolerance_grad': 1e-07,
                           'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})
    windowed_case("win_lin", 51, (300, 12), (-4, 4), 3, 0.01, adam, 50)
    windowed_case("win_lin_asym", 52, (200, 6, 5), (0, 5), 2, 0.01, {'lr': 0.02, 'amsgrad': True}, 30)
    windowed_case("win_mnl", 53, (260, 10), (-3, 5), 2, 0.01, adam, 40, n_classes=3)
    mnl_case("mnl_basic", 21, (128, 8, 4), 3, 2, [False, False, False], [1, 1, 1], 0.01, adam, 50)
    mnl_case("mnl_nonneg_weighted_amsgrad", 22, (160, 6, 5), 4, 3, [True, False, True], [0.5, 2.0, 1.0, 1.5], 0.02,
             {'lr': 0.01, 'amsgrad': True}, 50)
    mnl_case("mnl_c10", 23, (256, 16, 8), 10, 4, [False, False, False], [1.0] * 10, 0.01, adam, 50)
    mnl_case("mnl_converge", 24, (96, 4, 4), 2, 2, [False, False, False], [1, 1], 0.01, {'lr': 0.001}, 300,
             tol=0.01, patience=5)
    # the shapes of the two round-2 hot kernels (k_mnl_duo: (., 128, 64) / (., 64, 128) at rank 5-8;
    # k_spec_slice: W = 256, 97 <= D <= 130) fitted by the reference's own fit_Adam
    mnl_case("mnl_duo_shape", 42, (96, 128, 64), 10, 8, [False, False, False], [1.0] * 10, 0.01, adam, 40)
    mnl_case("mnl_duo_t", 43, (80, 64, 128), 6, 7, [True, False, True], [0.5, 2.0, 1.0, 1.5, 0.8, 1.2], 0.02,
             {'lr': 0.01, 'amsgrad': True}, 40)
    # full-mantissa X of small magnitude on the split body's shapes ((64, 64) rank 3: two 32-row waves;
    # (64, 128) rank 5: four 16-row waves), fitted by the reference's own fit_Adam
    mnl_case("mnl_bsp_f32x_small", 48, (32, 64, 64), 4, 3, [False, False, False], [1.0, 0.5, 2.0, 1.5], 0.01,
             {'lr': 0.01}, 40, x_scale=1e-3)
    mnl_case("mnl_bsp_f32x_j128", 49, (16, 64, 128), 6, 5, [False, False, False], [1.0] * 6, 0.01,
             {'lr': 0.01, 'amsgrad': True}, 30, x_scale=2e-2)
    # ranks 9..16 on the split body's 16-rank form (round 6): (96, 64) rank 12 (three 32-row waves,
    # a non-negative mode) and config 3's sample shape at rank 16
    mnl_case("mnl_bsp_r16_w3", 50, (40, 96, 64), 7, 12, [False, True, False], [1.0, 0.5, 2.0, 1.5, 1.0, 0.8, 1.2],
             0.01, {'lr': 0.01}, 30)
    mnl_case("mnl_bsp_r16_c3", 51, (24, 128, 64), 10, 16, [False, False, False], [1.0] * 10, 0.01,
             {'lr': 0.01, 'amsgrad': True}, 30)
    # samples above 64 KiB on the split body's row blocks (round 6): (512, 64) as two (256, 64)
    # blocks, (256, 128) as two (128, 128) blocks with full-mantissa X
    mnl_case("mnl_bsp_rowblk_512x64", 52, (10, 512, 64), 5, 6, [False, False, False], [1.0, 2.0, 0.5, 1.0, 1.5],
             0.01, {'lr': 0.01}, 30)
    mnl_case("mnl_bsp_rowblk_256x128", 53, (8, 256, 128), 4, 8, [True, False, False], [1.0] * 4, 0.01,
             {'lr': 0.005}, 30, x_scale=2e-2)
    # the split body's 32-wide form (round 6): (128, 32) rank 6 (four 32-row waves, a non-negative
    # mode), and a padded (100, 24) sample (to (128, 32)) with full-mantissa X of small magnitude
    mnl_case("mnl_bsp_j32_128x32", 54, (40, 128, 32), 5, 6, [False, True, False], [1.0, 2.0, 0.5, 1.0, 1.5],
             0.01, {'lr': 0.01}, 30)
    mnl_case("mnl_bsp_j32_pad_100x24", 55, (30, 100, 24), 4, 3, [False, False, False], [1.0, 0.5, 1.5, 1.0],
             0.01, {'lr': 0.01, 'amsgrad': True}, 30, x_scale=2e-2)
    init_case("init_rng")
    spectral_case("spec_basic", 31, (64, 12, 9), 3, 2, 2, 1, False, 0.01, adam, 50)
    spectral_case("spec_nonneg_amsgrad_wd", 32, (80, 16, 17), 2, 3, 2, 2, [True, False, True], 0.02,
                  {'lr': 0.02, 'amsgrad': True, 'weight_decay': 0.01, 'betas': (0.8, 0.99), 'eps': 1e-6}, 50)
    spectral_case("spec_c5_shape", 33, (128, 32, 33), 2, 8, 8, 1, False, 0.01, adam, 40)
    spectral_case("spec_slice_shape", 44, (40, 256, 129), 2, 8, 8, 1, False, 0.01, adam, 40)
    spectral_case("spec_slice_d100", 45, (32, 256, 100), 3, 3, 5, 1, [True, False, True], 0.02,
                  {'lr': 0.02, 'amsgrad': True}, 30)
    # full-mantissa X at config 5's sample shape: every split piece of X carries data in k_spec_slice's
    # bf16-split GEMMs (X in two pieces by default, x1 + x2; in three with TR_SLICE_XPIECES=3); Rn = 12
    # takes the unpacked-lin form (slsp=2)
    # (learning rates chosen so the reference's own fp32 trajectory stays within 1.1e-6 / 8.8e-7 of
    # its fp64 restatement over the whole horizon: at lr 0.01 this X drives Adam into oscillation
    # and the reference's fp32 run is 9e-6 from fp64, too close to the 1e-5 bar to test against)
    spectral_case("spec_slice_f32x", 46, (12, 256, 129), 2, 8, 8, 1, False, 0.01, {'lr': 0.002}, 40,
                  full_mantissa=True)
    spectral_case("spec_slice_rn12_f32x", 47, (10, 256, 129), 2, 12, 4, 1, [False, False, True], 0.01,
                  {'lr': 0.001, 'amsgrad': True}, 30, full_mantissa=True)
    spectral_case("spec_rn0", 34, (48, 8, 5), 2, 0, 3, 1, False, 0.01, adam, 30)
    spectral_case("spec_rs0", 35, (48, 8, 5), 2, 3, 0, 1, False, 0.01, adam, 30)
    spectral_case("spec_cc1_softplus", 36, (40, 6, 7), 4, 2, 3, 0, [True, True, True], 0.01, adam, 30,
                  softplus={'beta': 5, 'threshold': 2})
    spectral_case("spec_converge", 37, (64, 8, 5), 2, 2, 2, 1, False, 0.01, {'lr': 0.001}, 400, tol=0.02,
                  patience=5)
    spectral_case("spec_nan", 38, (32, 6, 5), 2, 2, 2, 1, False, 0.01, adam, 20, nan_y=True)
    spectral_case("spec_lbfgs", 39, (64, 8, 5), 2, 2, 2, 1, False, 1e-3, None, 5, tol=0.0, patience=100,
                  lbfgs_kwargs={'lr': 1, 'max_iter': 20, 'max_eval': None, 'tolerance_grad': 1e-07,
                                'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})
    if args.kat:
        kat_replay()


if __name__ == "__main__":
    main()
