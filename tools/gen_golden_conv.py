#!/usr/bin/env python3
"""Generate the convolutional-model fixtures tests/golden/cvs_*.npz by running the REFERENCE itself.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_conv.py [--reference DIR] [--only NAME ...]

Imports kimerein/tensor_regression's convolutional_spectral_tensor_regression from a read-only
checkout (default: a `reference` directory beside the repository) with the tensorly stand-in of
oracle/tensorly_standin on sys.path, runs small seeded cases through the reference's own class
and writes inputs + outputs only (nothing of the reference's source travels).  X is int8 / 8
(exactly representable) except in the one X_f32 case.  Every file stays far below 1 MiB.
"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(REPO, "tests", "golden")
sys.dont_write_bytecode = True
CSR = None  # the reference module, imported in main()
ONLY = None  # --only


def _np(ts):
    return [t.detach().numpy().copy() for t in ts]


def conv_case(name, seed, T, D, N, W, Rn, Rs, n_complex_dim, non_negative, lam, adam_kwargs, iters, tol=0.0,
              patience=10, softplus=None, lbfgs_kwargs=None, logging_interval=1, full_mantissa=False, zero_col=False):
    """One forward / loss / backward at the initial point with fit_Adam's own expression
    (…py:1044-1047: conv_linear WITHOUT softplus_kwargs), a 10-iteration and a full fit_Adam run
    (or fit, the LBFGS loop with self.softplus_kwargs, when lbfgs_kwargs is given)."""
    if ONLY is not None and name not in ONLY:
        return
    rng = np.random.default_rng(seed)
    if full_mantissa:
        Xf = rng.standard_normal((T, D)).astype(np.float32)
        Xq, X = None, torch.tensor(Xf)
    else:
        Xq = rng.integers(-8, 9, size=(T, D)).astype(np.int8)
        if zero_col:
            Xq[T // 3: T // 3 + 2 * W, 1] = 0  # ||zs|| = 0 over W + 1 outputs of column 1
        X = torch.tensor(Xq.astype(np.float32) / 8.0)
    y = torch.tensor(rng.standard_normal((T, N)).astype(np.float32))

    def make():
        torch.manual_seed(seed)
        return CSR.CP_linear_regression(X.shape, y.shape, rank_normal=Rn, temporal_window=W, rank_spectral=Rs,
                                        non_negative=non_negative, n_complex_dim=n_complex_dim,
                                        softplus_kwargs=softplus)

    m = make()
    out = dict(y=y.numpy(), Kn0=_np(m.Bcp_w)[0], Ks0=_np(m.Bcp_w)[1], Bd0=_np(m.Bcp_n)[0], Bo0=_np(m.Bcp_n)[1],
               bias0=m.bias.detach().numpy().copy(), idx_conv=m.idx_conv.numpy())
    lam3 = [lam] * 3 if np.isscalar(lam) else list(lam)
    sp = m.softplus_kwargs if lbfgs_kwargs is not None else None  # the quirk: fit_Adam passes none
    y_hat = CSR.conv_linear(X, m.Bcp_w, m.Bcp_n, m.weights[:m.rank_normal], m.non_negative, m.bias, sp)
    loss = torch.nn.MSELoss()(y_hat, y[m.idx_conv]) + CSR.L2_penalty(m.Bcp_w, [lam3[0]] * 2) + \
        CSR.L2_penalty(m.Bcp_n, lam3[1:])
    loss.backward()

    def g(A):
        return A.grad.numpy().copy() if A.grad is not None else np.zeros(tuple(A.shape), np.float32)

    out.update(y_hat0=y_hat.detach().numpy(), loss0=np.float64(loss.item()), gKn0=g(m.Bcp_w[0]), gKs0=g(m.Bcp_w[1]),
               gBd0=g(m.Bcp_n[0]), gBo0=g(m.Bcp_n[1]), gbias0=g(m.bias))
    if zero_col:
        zs = CSR.conv(X, m.Bcp_w[1].detach())
        assert (torch.norm(zs, dim=-1) == 0).any(), "the zero stretch must give ||zs|| = 0"
        assert all(np.isfinite(out[k]).all() for k in ("gKn0", "gKs0", "gBd0", "gBo0"))
    if full_mantissa:
        out["X_f32"] = X.numpy()
    else:
        out["X_q"] = Xq
    if lbfgs_kwargs is None:
        m10 = make()
        m10.fit_Adam(X, y, lambda_L2=lam3, max_iter=min(10, iters), tol=tol, patience=patience, verbose=False,
                     Adam_kwargs=dict(adam_kwargs))
        out.update(Kn_10=_np(m10.Bcp_w)[0], Ks_10=_np(m10.Bcp_w)[1], Bd_10=_np(m10.Bcp_n)[0], Bo_10=_np(m10.Bcp_n)[1],
                   bias_10=m10.bias.detach().numpy().copy(),
                   loss_running_10=np.array(m10.loss_running, dtype=np.float64))
        m = make()
        conv = m.fit_Adam(X, y, lambda_L2=lam3, max_iter=iters, tol=tol, patience=patience, verbose=False,
                          Adam_kwargs=dict(adam_kwargs))
        if tol > 0:
            assert conv and len(m.loss_running) < iters, "the plateau rule must fire before max_iter"
    else:
        m = make()
        conv = m.fit(X, y, lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, verbose=False,
                     running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
        # A fixture can pin an implementation at 1e-5 only if the trajectory is that well determined:
        # strong-Wolfe line searches amplify rounding step by step (with 20 inner iterations per
        # step the reference's own fp32 run was 1.4e-4 away from its fp64 run by the third logged
        # loss).  So the reference is run again in fp64 from the same initial factors, and the
        # LBFGS settings must keep its fp32 trajectory, final factors and predict() within a tenth
        # of the bar of that (the factors are less well determined than the loss: at 4 inner
        # iterations per step the losses agreed to 2e-7 and the factors only to 1e-5).
        torch.manual_seed(seed)
        m0 = make()
        init64 = ([A.detach().double().requires_grad_(True) for A in m0.Bcp_w],
                  [A.detach().double().requires_grad_(True) for A in m0.Bcp_n])
        m64 = CSR.CP_linear_regression(X.shape, y.shape, dtype=torch.float64, rank_normal=Rn, temporal_window=W,
                                       rank_spectral=Rs, non_negative=non_negative, n_complex_dim=n_complex_dim,
                                       Bcp_init=init64, softplus_kwargs=softplus)
        m64.fit(X.double(), y.double(), lambda_L2=lam, max_iter=iters, tol=tol, patience=patience, verbose=False,
                running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))
        l32, l64 = np.array(m.loss_running), np.array(m64.loss_running)
        dev = float(np.max(np.abs(l32 - l64) / np.abs(l64)))
        print(f"{name}: the reference's fp32 LBFGS trajectory is {dev:.1e} relative from its fp64 one")
        assert len(l32) == len(l64) and dev < 1e-6, (name, dev)

        def nrel(a, b):
            a, b = a.detach().double().numpy().ravel(), b.detach().numpy().ravel()
            return float(np.linalg.norm(a - b) / np.linalg.norm(b))

        devs = [nrel(a, b) for a, b in zip(m.Bcp_w + m.Bcp_n + [m.bias], m64.Bcp_w + m64.Bcp_n + [m64.bias])]
        devs.append(nrel(m.predict(X), m64.predict(X.double())))
        print(f"{name}: final factors / bias / predict, fp32 from fp64: " + " ".join(f"{v:.1e}" for v in devs))
        assert max(devs) < 1e-6, (name, devs)
    out.update(loss_running=np.array(m.loss_running, dtype=np.float64), Kn_final=_np(m.Bcp_w)[0],
               Ks_final=_np(m.Bcp_w)[1], Bd_final=_np(m.Bcp_n)[0], Bo_final=_np(m.Bcp_n)[1],
               bias_final=m.bias.detach().numpy().copy(), converged=np.int32(bool(conv)),
               predict_final=m.predict(X).numpy())
    meta = dict(model="conv_spectral", seed=seed, T=T, D=D, N=N, W=W, rank_normal=Rn, rank_spectral=Rs,
                n_complex_dim=n_complex_dim, non_negative=list(m.non_negative), lambda_L2=lam,
                adam_kwargs=adam_kwargs, lbfgs_kwargs=lbfgs_kwargs, logging_interval=logging_interval, max_iter=iters,
                tol=tol, patience=patience, softplus_kwargs=m.softplus_kwargs, full_mantissa=full_mantissa,
                zero_col=zero_col, torch=torch.__version__)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, (name, size)
    print("wrote", path, size, "bytes")


def main():
    global CSR
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"))
    ap.add_argument("--only", nargs="*", default=None, help="fixture names to (re)write; default: all")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "oracle", "tensorly_standin"))
    sys.path.insert(0, args.reference)
    import matplotlib
    matplotlib.use("Agg")
    import convolutional_spectral_tensor_regression as mod  # the reference
    CSR = mod
    global ONLY
    ONLY = args.only
    os.makedirs(OUT, exist_ok=True)
    adam = {'lr': 0.01}
    lam = [0.01, 0.02, 0.03]
    conv_case("cvs_base", 61, 400, 12, 3, 7, 2, 3, 1, False, lam, adam, 40)
    conv_case("cvs_nn_all", 62, 300, 9, 2, 5, 2, 2, 1, [True, True, True], lam, adam, 30,
              softplus={'beta': 5, 'threshold': 3})
    conv_case("cvs_nn_d", 63, 300, 9, 2, 5, 2, 2, 1, [False, True, False], lam, adam, 30)
    conv_case("cvs_c1", 64, 300, 10, 3, 9, 2, 3, 0, False, lam, adam, 30)
    conv_case("cvs_c3", 65, 300, 10, 2, 9, 1, 2, 2, False, lam, adam, 30)
    conv_case("cvs_rn0", 66, 300, 8, 2, 5, 0, 3, 1, False, lam, adam, 30)
    conv_case("cvs_rs0", 67, 300, 8, 2, 5, 3, 0, 1, False, lam, adam, 30)
    conv_case("cvs_amsgrad_wd", 68, 300, 8, 2, 5, 2, 2, 1, [True, False, True], lam,
              {'lr': 0.01, 'amsgrad': True, 'weight_decay': 0.01}, 30)
    conv_case("cvs_wide_n1", 69, 600, 130, 1, 33, 2, 2, 1, False, lam, adam, 20)
    conv_case("cvs_f32x", 70, 400, 12, 3, 7, 2, 3, 1, False, lam, adam, 30, full_mantissa=True)
    conv_case("cvs_zero", 71, 300, 6, 2, 5, 1, 2, 1, False, lam, adam, 30, zero_col=True)
    conv_case("cvs_converge", 72, 300, 8, 2, 5, 2, 2, 1, False, lam, {'lr': 0.001}, 400, tol=0.02, patience=10)
    # one inner iteration per step (not torch's 20): see the conditioning check in conv_case
    conv_case("cvs_lbfgs", 73, 300, 8, 2, 5, 2, 2, 1, [True, False, True], 1e-3, None, 5, tol=0.0, patience=100,
              softplus={'beta': 5, 'threshold': 3},
              lbfgs_kwargs={'lr': 1, 'max_iter': 1, 'max_eval': 5, 'tolerance_grad': 1e-07,
                            'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})


if __name__ == "__main__":
    main()
