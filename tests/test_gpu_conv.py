"""GPU checks of the convolutional spectral model (tensor_regression_amd.
convolutional_spectral_tensor_regression, kernel k_conv in csrc/tr_conv.hip).

  * fixture parity (tests/golden/cvs_*.npz, written by the reference): y_hat0, loss0, every
    gradient, the 10-step and full loss trajectories, the final factors, `converged`, predict
  * a shape sweep against the fp64 restatement of tests/conv_ref.py (qualified against the fixtures
    by tests/test_conv_host.py): loss 1e-5 relative, y_hat and the gradient arena 1e-5 normwise
  * misaligned / strided X, run-to-run bitwise determinism, zero magnitudes, the envelope, the
    NaN stop and the plateau stop

Bars: RTOL = 1e-5 as in tests/test_gpu_spectral.py (the reference's own fp32 sits near 1e-7
normwise from fp64 at these sizes, so the bar is loose for an fp32-accumulating kernel).
"""
import functools

import numpy as np
import pytest
import torch

import conv_ref as cr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5
TT = 256  # k_conv's time tile


def _plan(W, D, N, Rn, Rs, C, T, nn, softplus=None):
    from tensor_regression_amd import _engine
    return _engine.ConvPlan(W, D, N, Rn, Rs, C, T, nn, softplus, DEV)


def _gpu_eval(plan, X, y, P, lam=None):
    """y_hat, loss and the gradient arena (data term; total with `lam`) as fp64 numpy."""
    W = plan.dims[0]
    dev = lambda a: a.detach().to(DEV, torch.float32).contiguous()  # noqa: E731
    arena = plan.pack([dev(P["Kn"]), dev(P["Ks"])], [dev(P["Bd"]), dev(P["Bo"])], dev(P["bias"]))
    target = y[W // 2: y.shape[0] - W // 2].contiguous()
    grad = torch.zeros(plan.num_grads, device=DEV)
    yhat = torch.empty_like(target)
    plan.loss_grad(X, target, None, float(target.numel()), arena, None, grad, yhat=yhat)
    assert float(grad[plan.num_params + 1]) == 0.0  # status slot
    if lam is None:
        return yhat.cpu().numpy(), float(grad[plan.num_params]), grad[:plan.num_params].cpu().numpy(), arena
    gtot = torch.zeros(plan.num_params, device=DEV)
    loss = torch.zeros(1, device=DEV)
    plan.finalize_grad(arena, grad, lam, gtot, loss)
    return yhat.cpu().numpy(), float(loss[0]), gtot.cpu().numpy(), arena


def _arena_of(g):
    return np.concatenate([np.asarray(g[k], np.float64).ravel() for k in ("Bd", "Bo", "Kn", "Ks", "bias")])


def _check(tag, got, want):
    yh, loss, grads = got
    yh_w, loss_w, g_w = want
    e_y, e_l, e_g = cr.rel(yh, yh_w), abs(loss - loss_w) / abs(loss_w), cr.rel(grads, g_w)
    print(f"{tag}: y_hat {e_y:.2e} loss {e_l:.2e} grad arena {e_g:.2e}")
    assert e_y < RTOL and e_l < RTOL and e_g < RTOL, (tag, e_y, e_l, e_g)


# ---- 1. fixture parity ---------------------------------------------------------------------

def _model_from(d):
    from tensor_regression_amd.convolutional_spectral_tensor_regression import CP_linear_regression
    m = d["meta"]
    t = lambda a: torch.tensor(a, device=DEV).requires_grad_(True)  # noqa: E731
    mod = CP_linear_regression((m["T"], m["D"]), (m["T"], m["N"]), rank_normal=m["rank_normal"],
                               temporal_window=m["W"], rank_spectral=m["rank_spectral"],
                               non_negative=m["non_negative"], Bcp_init=([t(d["Kn0"]), t(d["Ks0"])],
                                                                         [t(d["Bd0"]), t(d["Bo0"])]),
                               n_complex_dim=m["n_complex_dim"], device=DEV, softplus_kwargs=m["softplus_kwargs"])
    return mod


@pytest.mark.parametrize("name", cr.ALL_FIXTURES)
def test_fixture_first_step(name):
    d = cr.load(name)
    m = d["meta"]
    sp = m["softplus_kwargs"] if m["lbfgs_kwargs"] is not None else None
    plan = _plan(m["W"], m["D"], m["N"], m["rank_normal"], m["rank_spectral"], m["n_complex_dim"] + 1, m["T"],
                 m["non_negative"], sp)
    assert "conv-1pass" in plan.describe
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    P = {k: torch.tensor(d[k + "0"]) for k in cr.FACTORS}
    yh, loss, g, _ = _gpu_eval(plan, X, y, P, cr.lam3(m))
    assert cr.rel(yh, d["y_hat0"]) < RTOL
    assert abs(loss - float(d["loss0"])) < RTOL * abs(float(d["loss0"]))
    o = plan.offsets + [plan.num_params]
    for f, k in enumerate(("Bd", "Bo", "Kn", "Ks", "bias")):
        e = cr.rel(g[o[f]:o[f + 1]], d["g" + k + "0"])
        print(f"{name} grad {k}: {e:.2e}")
        assert e < RTOL, (k, e)


@pytest.mark.parametrize("name", cr.ADAM_FIXTURES)
def test_fixture_fit_adam(name):
    d = cr.load(name)
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    lam = cr.lam3(m)
    m10 = _model_from(d)
    m10.fit_Adam(X, y, lambda_L2=lam, max_iter=min(10, m["max_iter"]), tol=m["tol"], patience=m["patience"],
                 Adam_kwargs=dict(m["adam_kwargs"]))
    np.testing.assert_allclose(m10.loss_running, d["loss_running_10"], rtol=RTOL)
    mod = _model_from(d)
    conv = mod.fit_Adam(X, y, lambda_L2=lam, max_iter=m["max_iter"], tol=m["tol"], patience=m["patience"],
                        Adam_kwargs=dict(m["adam_kwargs"]))
    assert bool(conv) == bool(d["converged"])
    assert len(mod.loss_running) == len(d["loss_running"])
    np.testing.assert_allclose(mod.loss_running, d["loss_running"], rtol=RTOL)
    for A, k in zip(list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias], cr.FACTORS):
        e = cr.rel(A.detach().cpu().numpy(), d[k + "_final"])
        print(f"{name} final {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    pred = mod.predict(X)
    assert isinstance(pred, torch.Tensor) and pred.device.type == "cpu" and not pred.requires_grad
    assert pred.shape == (m["T"] - m["W"] + 1, m["N"])
    assert cr.rel(pred.numpy(), d["predict_final"]) < RTOL
    # predict == the training kernel's y_hat at the final factors (fit_Adam's softplus 50 / 1)
    plan = mod._plan_for(X, 0, None)
    P = {k: A.detach().cpu() for k, A in zip(cr.FACTORS, list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias])}
    yh, _, _, _ = _gpu_eval(plan, X, y, P)
    assert cr.rel(pred.numpy(), yh) < 1e-6
    assert pred.numpy().shape == yh.shape


def test_fixture_lbfgs_fit():
    """fit (LBFGS, strong Wolfe) with a scalar lambda and the model's own softplus_kwargs against the
    reference's fp32 trajectory, final factors and predict, to RTOL.  The fixture's LBFGS settings
    (one inner iteration per step, five steps sharing one history) keep the fit well determined:
    tools/gen_golden_conv.py asserts that the reference's own fp32 and fp64 runs agree to 1e-6 in the
    losses, every final factor and predict (measured 2e-7 to 6e-7), so 1e-5 separates a wrong
    gradient from rounding.  (At torch's 20 inner iterations the reference's fp32 run is itself
    1.4e-4 from its fp64 run, at 4 its final factors 1e-5.)"""
    d = cr.load("cvs_lbfgs")
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    mod = _model_from(d)
    conv = mod.fit(X, y, lambda_L2=m["lambda_L2"], max_iter=m["max_iter"], tol=m["tol"], patience=m["patience"],
                   running_loss_logging_interval=m["logging_interval"], LBFGS_kwargs=dict(m["lbfgs_kwargs"]))
    assert bool(conv) == bool(d["converged"])
    assert len(mod.loss_running) == len(d["loss_running"])
    print("lbfgs rel to fixture", np.abs(np.asarray(mod.loss_running) - d["loss_running"]) / d["loss_running"])
    np.testing.assert_allclose(mod.loss_running, d["loss_running"], rtol=RTOL)
    for A, k in zip(list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias], cr.FACTORS):
        e = cr.rel(A.detach().cpu().numpy(), d[k + "_final"])
        print(f"cvs_lbfgs final {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    assert cr.rel(mod.predict(X).numpy(), d["predict_final"]) < RTOL


# ---- 2. shape sweep against the fp64 restatement -------------------------------------------

SWEEP = [
    # fewer outputs than any tile; W = 1, no halo
    (1, 1, 1, 1, 1, 0, 2), (1, 33, 3, 1, 0, 1, 2),
    # around 64 and around the kernel's own tile edge
    (63, 3, 17, 3, 2, 3, 2), (64, 3, 17, 3, 2, 3, 2), (65, 3, 17, 3, 2, 3, 2),
    (TT - 1, 3, 17, 3, 2, 3, 2), (TT, 3, 17, 3, 2, 3, 2), (TT + 1, 3, 17, 3, 2, 3, 2),
    # halo longer than a tile
    (257, 129, 4, 2, 2, 2, 2), (40, 257, 5, 2, 1, 1, 2),
    # D chunking and odd D
    (300, 33, 130, 4, 3, 5, 3), (200, 17, 300, 7, 8, 8, 2), (1000, 9, 64, 3, 16, 4, 4),
    # C = 1 and empty ranks
    (129, 5, 33, 64, 1, 2, 1), (500, 7, 12, 2, 32, 0, 2), (500, 7, 12, 2, 0, 16, 4),
]


def _inputs(case, seed=0, zero_col=False):
    Tp, W, D, N, Rn, Rs, C = case
    T = Tp + W - 1
    g = torch.Generator().manual_seed(1000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    X = rn(T, D).float()
    if zero_col:
        X[T // 3: T // 3 + 2 * W, 0] = 0
    y = rn(T, N).float()
    P = dict(Kn=rn(W, Rn) / W ** 0.5, Ks=(rn(W, Rs, C) if C > 1 else rn(W, Rs)) / W ** 0.5,
             Bd=rn(D, Rn + Rs) / D ** 0.5, Bo=rn(N, Rn + Rs), bias=0.1 * rn(N))
    P = {k: v.float() for k, v in P.items()}  # fp32-representable parameters, shared by both sides
    return X, y, P


@functools.lru_cache(maxsize=None)
def _reference(case, nn, zero_col=False):
    """fp64 restatement, computed once per (case, flags) and shared."""
    X, y, P = _inputs(case, zero_col=zero_col)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    yh, loss, g = cr.value_and_grads(X.double(), y.double(), P64, nn)
    return yh.numpy(), loss, _arena_of({k: v.numpy() for k, v in g.items()})


@pytest.mark.parametrize("nn", [(False, False, False), (True, True, True)], ids=["plain", "softplus"])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "x".join(map(str, c)))
def test_sweep_against_fp64(case, nn):
    Tp, W, D, N, Rn, Rs, C = case
    X, y, P = _inputs(case)
    plan = _plan(W, D, N, Rn, Rs, C, Tp + W - 1, list(nn))
    yh, loss, g, _ = _gpu_eval(plan, X.to(DEV), y.to(DEV), P)
    assert yh.shape == (Tp, N)
    _check(f"{case} {nn}", (yh, loss, g), _reference(case, nn))


# ---- 3. misaligned and strided X -----------------------------------------------------------

def test_misaligned_x():
    case = (300, 5, 17, 3, 2, 3, 2)
    X, y, P = _inputs(case)
    T = X.shape[0]
    buf = torch.zeros(T * 17 + 1, device=DEV)
    buf[1:] = X.to(DEV).reshape(-1)
    Xm = buf[1:].view(T, 17)
    assert Xm.data_ptr() % 16 == 4
    plan = _plan(5, 17, 3, 2, 3, 2, T, [False] * 3)
    yh, loss, g, _ = _gpu_eval(plan, Xm, y.to(DEV), P)
    _check("misaligned", (yh, loss, g), _reference(case, (False, False, False)))


def test_strided_and_noncontiguous_x():
    from tensor_regression_amd.convolutional_spectral_tensor_regression import _series, conv_linear
    case = (300, 5, 17, 3, 2, 3, 2)
    X, y, P = _inputs(case)
    T = X.shape[0]
    want = _reference(case, (False, False, False))
    plan = _plan(5, 17, 3, 2, 3, 2, T, [False] * 3)
    wide = torch.zeros(T, 40, device=DEV)
    wide[:, :17] = X.to(DEV)
    Xs, _ = _series(wide[:, :17])  # contiguous rows at a stride of 40 floats: read in place
    assert Xs.data_ptr() == wide.data_ptr() and Xs.stride(0) == 40
    yh, loss, g, _ = _gpu_eval(plan, Xs, y.to(DEV), P)
    _check("row-strided", (yh, loss, g), want)
    inter = torch.zeros(T, 34, device=DEV)
    inter[:, ::2] = X.to(DEV)
    Xn, _ = _series(inter[:, ::2])  # elements not contiguous: made contiguous
    assert Xn.is_contiguous()
    yh, loss, g, _ = _gpu_eval(plan, Xn, y.to(DEV), P)
    _check("non-contiguous", (yh, loss, g), want)
    dv = lambda a: a.to(DEV)  # noqa: E731
    out = conv_linear(inter[:, ::2], [dv(P["Kn"]), dv(P["Ks"])], [dv(P["Bd"]), dv(P["Bo"])], None, [False] * 3,
                      dv(P["bias"]))
    assert cr.rel(out.cpu().numpy(), want[0]) < RTOL


# ---- 4. determinism ------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(5000, 9, 16, 3, 2, 3, 2), (100, 9, 16, 3, 2, 3, 2)], ids=["many-wg", "one-wg"])
def test_loss_grad_is_bitwise_reproducible(case):
    Tp, W, D, N, Rn, Rs, C = case
    X, y, P = _inputs(case)
    plan = _plan(W, D, N, Rn, Rs, C, Tp + W - 1, [False] * 3)
    Xd, yd = X.to(DEV), y.to(DEV)
    dev = lambda a: a.to(DEV).contiguous()  # noqa: E731
    arena = plan.pack([dev(P["Kn"]), dev(P["Ks"])], [dev(P["Bd"]), dev(P["Bo"])], dev(P["bias"]))
    target = yd[W // 2: yd.shape[0] - W // 2].contiguous()
    grads = []
    for _ in range(2):
        g = torch.full((plan.num_grads,), float("nan"), device=DEV)
        plan.loss_grad(Xd, target, None, float(target.numel()), arena, None, g)
        grads.append(g.cpu())
    assert torch.isfinite(grads[0]).all()
    assert torch.equal(grads[0], grads[1])


# ---- 5. zero magnitude ---------------------------------------------------------------------

def test_zero_magnitude_gradients():
    case = (300, 7, 12, 3, 2, 3, 2)
    X, y, P = _inputs(case, zero_col=True)
    z = torch.einsum('tdw,wsc->tdsc', X.unfold(0, 7, 1), P["Ks"])
    assert (z.pow(2).sum(-1) == 0).any()  # ||zs|| = 0 does occur
    plan = _plan(7, 12, 3, 2, 3, 2, X.shape[0], [False] * 3)
    yh, loss, g, _ = _gpu_eval(plan, X.to(DEV), y.to(DEV), P)
    assert np.isfinite(g).all() and np.isfinite(yh).all()
    _check("zero-magnitude", (yh, loss, g), _reference(case, (False, False, False), True))


# ---- 6. envelope ---------------------------------------------------------------------------

def test_envelope_and_describe():
    with pytest.raises(ValueError, match="W <= 257"):
        _plan(259, 4, 2, 1, 1, 2, 600, [False] * 3)
    with pytest.raises(ValueError, match="<= 32"):
        _plan(7, 4, 2, 17, 16, 1, 600, [False] * 3)
    plan = _plan(7, 4, 2, 1, 1, 2, 600, [False] * 3)
    assert "model=conv_spectral" in plan.describe and "path=conv-1pass-fmaf" in plan.describe
    assert plan.offsets == [0, 8, 12, 19, 33]
    assert plan.num_params == 35 and plan.num_grads == 37


# ---- 7. NaN stop and plateau stop ----------------------------------------------------------

def test_nan_stop_on_inf_target(capsys):
    d = cr.load("cvs_base")
    m = d["meta"]
    X, y = torch.tensor(d["X"]), torch.tensor(d["y"])
    y[50, 1] = float("inf")
    want = cr.adam_losses(X, y, cr.leaf_params(d, torch.float32), m["non_negative"], cr.lam3(m), {'lr': 0.01}, 3)
    first_nan = int(np.argmax(np.isnan(want)))
    assert np.isnan(want).any() and first_nan <= 2
    mod = _model_from(d)
    conv = mod.fit_Adam(X.to(DEV), y.to(DEV), lambda_L2=cr.lam3(m), max_iter=3, tol=0.0, patience=10,
                        Adam_kwargs={'lr': 0.01})
    assert conv is False
    assert len(mod.loss_running) == first_nan + 1  # stopped at the first NaN loss (ii <= patience)
    assert np.isnan(mod.loss_running[-1])
    assert "Loss is NaN. Stopping." in capsys.readouterr().out


def test_plateau_stop_fires_before_max_iter():
    d = cr.load("cvs_converge")
    m = d["meta"]
    assert bool(d["converged"]) and len(d["loss_running"]) < m["max_iter"]
    mod = _model_from(d)
    conv = mod.fit_Adam(torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV), lambda_L2=cr.lam3(m),
                        max_iter=m["max_iter"], tol=m["tol"], patience=m["patience"],
                        Adam_kwargs=dict(m["adam_kwargs"]))
    assert conv is True and len(mod.loss_running) == len(d["loss_running"])


def test_verbose_prints_variance_ratio(capsys):
    d = cr.load("cvs_base")
    m = d["meta"]
    mod = _model_from(d)
    mod.fit_Adam(torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV), lambda_L2=cr.lam3(m),
                 max_iter=2, tol=0.0, patience=10, verbose=3, Adam_kwargs={'lr': 0.01})
    out = capsys.readouterr().out
    assert out.count("Variance ratio (y_hat / y_true)") == 2 and "Iteration: 1, Loss:" in out


def test_lbfgs_verbose_lines_and_nan_stop(capsys):
    """fit's per-iteration line (verbose=3: the logged loss and the variance ratio), its convergence
    line, and its NaN notice: a NaN target makes the first logged loss NaN and the fit stops there."""
    d = cr.load("cvs_base")
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    lbfgs = {'lr': 1, 'max_iter': 2}
    mod = _model_from(d)
    conv = mod.fit(X, y, lambda_L2=cr.lam3(m), max_iter=2, tol=0.0, verbose=3, running_loss_logging_interval=1,
                   LBFGS_kwargs=lbfgs)
    assert conv is False and len(mod.loss_running) == 2
    lines = capsys.readouterr().out.splitlines()
    for ii, loss in enumerate(mod.loss_running):
        head = f'Iteration: {ii}, Loss: {loss}  ;  Variance ratio (y_hat / y_true): '
        assert lines[ii].startswith(head) and float(lines[ii][len(head):]) > 0, lines[ii]
    assert lines[2:] == ["Reached maximum number of iterations without convergence"]
    y[50, 1] = float("nan")
    mod = _model_from(d)
    conv = mod.fit(X, y, lambda_L2=cr.lam3(m), max_iter=3, tol=0.0, running_loss_logging_interval=1,
                   LBFGS_kwargs=lbfgs)
    assert conv is False and len(mod.loss_running) == 1 and np.isnan(mod.loss_running[0])
    assert capsys.readouterr().out == "Loss is NaN. Stopping.\n"
