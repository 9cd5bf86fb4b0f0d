#!/usr/bin/env python3
"""Generate the convolutional Fourier model's fixtures tests/golden/cfs_*.npz by running the REFERENCE itself.

    PYTHONDONTWRITEBYTECODE=1 python tools/gen_golden_fourier.py [--reference DIR] [--only NAME ...]

Imports kimerein/tensor_regression's convolutional_fourier_tensor_regression from a read-only checkout
(default: a `reference` directory beside the repository) with the tensorly stand-in of
oracle/tensorly_standin on sys.path, runs small seeded cases through the reference's own class and
writes inputs + outputs only (nothing of the reference's source travels).  X is int8 / 8 (exactly
representable) except in the one X_f32 case.  Every file stays below 512 KiB.

Every case is also run in fp64 (dtype=torch.float64, same initial factors): a trajectory whose
fp32 run is more than 1e-6 from the fp64 run is not written, so the tests' 1e-5 bar measures the
implementation and not the reference's rounding.
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
REF = None  # the reference module, imported in main()
ONLY = None  # --only
FACTORS = ("Kn", "Ks", "Bd", "Bo", "bias")


def _np(ts):
    return [t.detach().numpy().copy() for t in ts]


def _nan_rel(a, b):
    """max relative distance of two trajectories with the same NaN pattern."""
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    assert a.shape == b.shape and np.array_equal(np.isnan(a), np.isnan(b)), (a, b)
    ok = ~np.isnan(b)
    return float(np.max(np.abs(a[ok] - b[ok]) / np.abs(b[ok]))) if ok.any() else 0.0


def fourier_case(name, seed, T, D, N, W, Rn, Rs, ncd, ssf, lam_sp, non_negative=False, lam=(0.01, 0.02, 0.03),
                 lam_s=0.05, order=2, adam_kwargs=None, iters=30, tol=0.0, patience=10, softplus=None,
                 lbfgs_kwargs=None, logging_interval=1, full_mantissa=False, penalty=True):
    """One forward / loss / backward at the initial point with fit_Adam's own expressions
    (…py:1269-1282, 1301), a 10-iteration and a full fit_Adam run (or fit, the LBFGS loop, when
    lbfgs_kwargs is given)."""
    if ONLY is not None and name not in ONLY:
        return
    adam_kwargs = {'lr': 0.01} if adam_kwargs is None else adam_kwargs
    rng = np.random.default_rng(seed)
    if full_mantissa:
        Xq, X = None, torch.tensor(rng.standard_normal((T, D)).astype(np.float32))
    else:
        Xq = rng.integers(-8, 9, size=(T, D)).astype(np.int8)
        X = torch.tensor(Xq.astype(np.float32) / 8.0)
    y = torch.tensor(rng.standard_normal((T, N)).astype(np.float32))
    kw = dict(rank_normal=Rn, temporal_window=W, rank_spectral=Rs, non_negative=non_negative, n_complex_dim=ncd,
              do_spectralPenalty=penalty, spectrum_smoothing_factor=ssf, softplus_kwargs=softplus)

    torch.manual_seed(seed)
    drawn = REF.CP_linear_regression(X.shape, y.shape, **kw)  # the constructor's own draws
    init = [A.detach().clone() for A in drawn.Bcp_w + drawn.Bcp_n]

    def make(dtype=torch.float32):
        leaves = [A.to(dtype).clone().requires_grad_(True) for A in init]
        return REF.CP_linear_regression(X.shape, y.shape, dtype=dtype, Bcp_init=(leaves[:2], leaves[2:]), **kw)

    m = make()
    out = dict(y=y.numpy(), Kn_drawn=_np(drawn.Bcp_w)[0], Ks_drawn=_np(drawn.Bcp_w)[1], Bd_drawn=_np(drawn.Bcp_n)[0],
               Bo_drawn=_np(drawn.Bcp_n)[1], Kn0=_np(m.Bcp_w)[0], Ks0=_np(m.Bcp_w)[1], Bd0=_np(m.Bcp_n)[0],
               Bo0=_np(m.Bcp_n)[1], bias0=m.bias.detach().numpy().copy(), idx_conv=m.idx_conv.numpy(),
               smoothing_kernel=m.spectral_smoothing_kernel.numpy().copy())
    lam3 = [lam] * 3 if np.isscalar(lam) else list(lam)
    leaves = m.Bcp_w + m.Bcp_n + [m.bias]

    def g(A):
        return A.grad.numpy().copy() if A.grad is not None else np.zeros(tuple(A.shape), np.float32)

    def fwd():
        return REF.forward_model(X, m.Bcp_w, m.Bcp_n, m.weights, m.non_negative, m.bias, m.softplus_kwargs)

    def pen(y_hat, y_spec):
        return REF.spectral_penalty(y_pred=y_hat, y_true_fft=y_spec, n_fft=m.y_shape[0],
                                    smoothing_kernel=m.spectral_smoothing_kernel, passthrough=1 - m.do_spectralPenalty,
                                    lam=lam_sp, plot_pref=False)

    y_spec = None
    if penalty:  # fit_Adam's own expression (…py:1261)
        y_spec = REF.conv(torch.abs(torch.fft.rfft(y[m.idx_conv], n=m.y_shape[0], dim=0)), m.spectral_smoothing_kernel)
        out["y_spectrum"] = y_spec.numpy().copy()
    # the data term alone, the penalty alone (its gradient into y_hat), then the total
    y_hat = fwd()
    loss_rec = torch.nn.MSELoss()(y_hat, y[m.idx_conv])
    loss_rec.backward()
    out.update({"d" + k + "0": g(A) for k, A in zip(FACTORS, leaves)})
    out["loss_rec0"] = np.float64(loss_rec.item())
    for A in leaves:
        A.grad = None
    if penalty:
        y_hat = fwd()
        y_hat.retain_grad()
        p0 = pen(y_hat, y_spec)
        p0.backward()
        out.update(loss_spectral0=np.float64(p0.item()), dpen_dyhat0=y_hat.grad.numpy().copy())
        for A in leaves:
            A.grad = None
    y_hat = fwd()
    loss = torch.nn.MSELoss()(y_hat, y[m.idx_conv]) + REF.L2_penalty(m.Bcp_w, [lam3[0]] * 2) + \
        REF.L2_penalty(m.Bcp_n, lam3[1:]) + pen(y_hat, y_spec) + \
        REF.smoothness_penalty(m.Bcp_w, derivative_order=order, lambda_smooth=lam_s)
    loss.backward()
    out.update({"g" + k + "0": g(A) for k, A in zip(FACTORS, leaves)})
    out.update(y_hat0=y_hat.detach().numpy(), loss0=np.float64(loss.item()))
    if full_mantissa:
        out["X_f32"] = X.numpy()
    else:
        out["X_q"] = Xq

    def run(model, Xr, yr, n_iter):
        if lbfgs_kwargs is None:
            return model.fit_Adam(Xr, yr, lambda_L2=lam3, lambda_spectralPenalty=lam_sp, lambda_smooth=lam_s,
                                  smooth_diff_order=order, max_iter=n_iter, tol=tol, patience=patience, verbose=False,
                                  Adam_kwargs=dict(adam_kwargs))
        return model.fit(Xr, yr, lambda_L2=lam, lambda_spectralPenalty=lam_sp, lambda_smooth=lam_s,
                         smooth_diff_order=order, max_iter=n_iter, tol=tol, patience=patience, verbose=False,
                         running_loss_logging_interval=logging_interval, LBFGS_kwargs=dict(lbfgs_kwargs))

    if lbfgs_kwargs is None:
        m10 = make()
        run(m10, X, y, min(10, iters))
        out.update({k + "_10": a for k, a in zip(FACTORS, _np(m10.Bcp_w + m10.Bcp_n + [m10.bias]))})
        out["loss_running_10"] = np.array(m10.loss_running, dtype=np.float64)
    m = make()
    conv = run(m, X, y, iters)
    if tol > 0:
        assert conv and len(m.loss_running) < iters, "the plateau rule must fire before max_iter"
    # the conditioning check: the reference's own fp64 run from the same initial factors
    m64 = make(torch.float64)
    conv64 = run(m64, X.double(), y.double(), iters)
    assert bool(conv) == bool(conv64) and len(m.loss_running) == len(m64.loss_running), name
    dev = _nan_rel(m.loss_running, m64.loss_running)

    def nrel(a, b):  # normwise over the finite entries; the NaN patterns must agree
        a, b = a.detach().double().numpy().ravel(), b.detach().numpy().ravel()
        assert np.array_equal(np.isnan(a), np.isnan(b)), name
        ok = ~np.isnan(b)
        nb = np.linalg.norm(b[ok])
        return float(np.linalg.norm(a[ok] - b[ok]) / nb) if nb > 0 else float(np.linalg.norm(a[ok] - b[ok]))

    fdev = [nrel(a, b) for a, b in zip(m.Bcp_w + m.Bcp_n + [m.bias], m64.Bcp_w + m64.Bcp_n + [m64.bias])]
    print(f"{name}: fp32 from fp64, losses {dev:.1e} relative; final factors / bias normwise " +
          " ".join(f"{v:.1e}" for v in fdev))
    assert dev < 1e-6, (name, dev)
    if lbfgs_kwargs is not None:
        assert max(fdev) < 1e-6, (name, fdev)
    out.update({k + "_final": a for k, a in zip(FACTORS, _np(m.Bcp_w + m.Bcp_n + [m.bias]))})
    out.update(loss_running=np.array(m.loss_running, dtype=np.float64), converged=np.int32(bool(conv)),
               predict_final=m.predict(X).numpy())
    meta = dict(model="conv_fourier", seed=seed, T=T, D=D, N=N, W=W, rank_normal=Rn, rank_spectral=Rs,
                n_complex_dim=ncd, spectrum_smoothing_factor=ssf, do_spectralPenalty=bool(penalty),
                lambda_spectralPenalty=lam_sp, non_negative=list(m.non_negative), lambda_L2=lam,
                lambda_smooth=lam_s, smooth_diff_order=order, adam_kwargs=adam_kwargs, lbfgs_kwargs=lbfgs_kwargs,
                logging_interval=logging_interval, max_iter=iters, tol=tol, patience=patience,
                softplus_kwargs=m.softplus_kwargs, full_mantissa=full_mantissa, torch=torch.__version__)
    out["meta"] = np.array(json.dumps(meta))
    path = os.path.join(OUT, name + ".npz")
    np.savez_compressed(path, **out)
    size = os.path.getsize(path)
    assert size < 512 * 1024, (name, size)
    print("wrote", path, size, "bytes")


def main():
    global REF, ONLY
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", default=os.path.join(os.path.dirname(REPO), "reference"))
    ap.add_argument("--only", nargs="*", default=None, help="fixture names to (re)write; default: all")
    args = ap.parse_args()
    sys.path.insert(0, os.path.join(REPO, "oracle", "tensorly_standin"))
    sys.path.insert(0, args.reference)
    import matplotlib
    matplotlib.use("Agg")
    import convolutional_fourier_tensor_regression as mod  # the reference
    REF = mod
    ONLY = args.only
    os.makedirs(OUT, exist_ok=True)
    sp = {'beta': 5, 'threshold': 3}
    #            name          seed   T   D  N   W Rn Rs ncd ssf lam_sp
    fourier_case("cfs_base", 101, 400, 6, 3, 7, 2, 3, 1, 8, .05, iters=40)
    fourier_case("cfs_rn0", 102, 300, 5, 2, 5, 0, 2, 1, 8, .05)
    fourier_case("cfs_rs0", 103, 300, 5, 2, 5, 2, 0, 1, 8, .05)
    fourier_case("cfs_c3", 104, 300, 5, 2, 9, 2, 2, 2, 8, .05)
    fourier_case("cfs_n1", 105, 301, 5, 1, 5, 2, 2, 1, 8, .05)
    fourier_case("cfs_ssf100", 106, 1031, 5, 2, 7, 2, 2, 1, 100, .5)
    fourier_case("cfs_ssf1", 107, 211, 4, 2, 5, 2, 2, 1, 1, .05)
    fourier_case("cfs_nn_all", 108, 300, 5, 2, 5, 2, 2, 1, 8, .05, non_negative=[True, True, True], softplus=sp)
    fourier_case("cfs_lam1", 109, 300, 5, 2, 5, 2, 2, 1, 8, 1.0)
    fourier_case("cfs_wide", 110, 600, 130, 2, 33, 2, 2, 1, 20, .05, iters=20)
    fourier_case("cfs_off", 111, 300, 5, 2, 5, 2, 2, 1, 8, .05, penalty=False)
    fourier_case("cfs_off_c4", 112, 300, 5, 2, 7, 3, 2, 3, 8, .05, penalty=False, order=1, lam_s=1.0)
    fourier_case("cfs_amsgrad_wd", 113, 300, 5, 2, 5, 2, 2, 1, 8, .05, non_negative=[True, False, True],
                 adam_kwargs={'lr': 0.01, 'amsgrad': True, 'weight_decay': 0.01})
    fourier_case("cfs_converge", 114, 300, 5, 2, 5, 2, 2, 1, 8, .05, adam_kwargs={'lr': 0.001}, iters=400, tol=0.02,
                 patience=10)
    # one inner iteration per step (not torch's 20): strong-Wolfe line searches amplify rounding
    fourier_case("cfs_lbfgs", 115, 300, 5, 2, 5, 2, 2, 1, 8, .05, non_negative=[True, False, True], lam=1e-3, iters=5,
                 patience=100, softplus=sp,
                 lbfgs_kwargs={'lr': 1, 'max_iter': 1, 'max_eval': 5, 'tolerance_grad': 1e-07,
                               'tolerance_change': 1e-09, 'history_size': 100, 'line_search_fn': "strong_wolfe"})
    fourier_case("cfs_f32x", 116, 400, 6, 3, 7, 2, 3, 1, 8, .05, full_mantissa=True)


if __name__ == "__main__":
    main()
