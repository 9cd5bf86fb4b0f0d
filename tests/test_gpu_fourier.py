"""GPU checks of the convolutional Fourier model (tensor_regression_amd.
convolutional_fourier_tensor_regression; the spectrum path k_dft / k_spec_* of
csrc/tr_conv_spectrum.hip around k_conv and k_update_conv of csrc/tr_conv.hip).

  * fixture parity (tests/golden/cfs_*.npz, written by the reference) through the public class:
    y_hat0, the data loss, the penalty value, d pen / d y_hat, y_spectrum, every gradient (total and
    data term alone), the 10-step and full loss trajectories, the final factors, `converged`, predict
  * the spectrum path alone (tr_conv_spectrum, tr_conv_spectrum_penalty) against torch.fft in fp64,
    up to a transform length whose angle products pass 2^32
  * a plan sweep against the fp64 restatement of tests/fourier_ref.py (qualified against the fixtures
    and against autograd by tests/test_fourier_host.py)
  * flag off == the conv plan bitwise, lambda_sp = 0 == flag off, run-to-run bitwise determinism with
    the penalty on, the envelope, the describe string and the ABI's order of calls

Bars: RTOL = 1e-5 as in tests/test_gpu_conv.py, unchanged: losses relative, gradients and spectra
normwise, trajectories.

Measured on an MI355X (the tests print these), against fp64:
  spectrum path alone, (rows, n_fft, N, S):     M_y      M        value    gradient
    (1, 7, 1, 1)                                3.1e-08  9.5e-09  6.5e-08  7.2e-08
    (93, 97, 3, 5)                              9.2e-08  8.4e-08  9.9e-08  4.5e-07
    (294, 300, 2, 9)                            9.8e-08  1.0e-07  5.7e-08  6.8e-07
    (295, 301, 1, 9)                            1.0e-07  8.7e-08  5.6e-08  7.7e-07
    (8, 16, 2, 9)                               3.7e-08  8.0e-08  4.6e-07  2.5e-07
    (50, 64, 64, 3)                             8.9e-08  8.9e-08  2.1e-08  3.7e-07
    (1025, 1031, 2, 101)                        1.5e-07  1.5e-07  1.3e-08  8.2e-07
    (2040, 2048, 2, 101)                        1.4e-07  1.4e-07  1.8e-07  7.9e-07
    (99971, 100003, 1, 101)                     1.5e-07  1.5e-07  7.6e-09  9.5e-07
  plan sweep with the penalty on (14 cases) and the three smoothness orders: y_hat <= 3.3e-07, data
  loss <= 3.5e-07, penalty value <= 3.2e-07, total loss <= 2.5e-07, total gradients <= 4.8e-07
  fixtures (against the reference's own fp32 outputs): d pen / d y_hat <= 1.7e-06, first-step
  gradients <= 1.2e-06, loss trajectories <= 2.7e-07, final factors <= 1.3e-06, LBFGS losses <= 2.2e-07
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import fourier_ref as fr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5


def _plan(W, D, N, Rn, Rs, C, T, nn, softplus=None, lam_s=0.0, q=2):
    from tensor_regression_amd import _engine
    return _engine.ConvFourierPlan(W, D, N, Rn, Rs, C, T, nn, softplus, DEV, lam_s, q)


def _arena(plan, P):
    dev = lambda a: a.detach().to(DEV, torch.float32).contiguous()  # noqa: E731
    return plan.pack([dev(P["Kn"]), dev(P["Ks"])], [dev(P["Bd"]), dev(P["Bo"])], dev(P["bias"]))


def _gpu_eval(plan, X, y, P, lam):
    """y_hat, (loss slot, gradient arena of loss_grad), (total loss, total gradient arena) as numpy."""
    W = plan.dims[0]
    arena = _arena(plan, P)
    target = y[W // 2: y.shape[0] - W // 2].contiguous()
    grad = torch.full((plan.num_grads,), float("nan"), device=DEV)
    yhat = torch.empty_like(target)
    plan.loss_grad(X, target, None, float(target.numel()), arena, None, grad, yhat=yhat)
    assert float(grad[plan.num_params + 1]) == 0.0  # status slot
    gtot = torch.full((plan.num_params,), float("nan"), device=DEV)
    loss = torch.zeros(1, device=DEV)
    plan.finalize_grad(arena, grad, lam, gtot, loss)
    return (yhat.cpu().numpy(), (float(grad[plan.num_params]), grad[:plan.num_params].cpu().numpy()),
            (float(loss[0]), gtot.cpu().numpy()))


# ---- 1. fixture parity ---------------------------------------------------------------------

def _model_from(d):
    from tensor_regression_amd.convolutional_fourier_tensor_regression import CP_linear_regression
    m = d["meta"]
    t = lambda a: torch.tensor(a, device=DEV).requires_grad_(True)  # noqa: E731
    return CP_linear_regression((m["T"], m["D"]), (m["T"], m["N"]), rank_normal=m["rank_normal"],
                                temporal_window=m["W"], rank_spectral=m["rank_spectral"],
                                non_negative=m["non_negative"], n_complex_dim=m["n_complex_dim"],
                                Bcp_init=([t(d["Kn0"]), t(d["Ks0"])], [t(d["Bd0"]), t(d["Bo0"])]), device=DEV,
                                do_spectralPenalty=m["do_spectralPenalty"],
                                spectrum_smoothing_factor=m["spectrum_smoothing_factor"],
                                softplus_kwargs=m["softplus_kwargs"])


def _fit_kwargs(m):
    return dict(lambda_spectralPenalty=m["lambda_spectralPenalty"], lambda_smooth=m["lambda_smooth"],
                smooth_diff_order=m["smooth_diff_order"], max_iter=m["max_iter"], tol=m["tol"],
                patience=m["patience"])


@pytest.mark.parametrize("name", fr.ALL_FIXTURES)
def test_fixture_first_step(name):
    d = fr.load(name)
    m = d["meta"]
    mod = _model_from(d)
    assert np.array_equal(mod.spectral_smoothing_kernel.cpu().numpy(), d["smoothing_kernel"])
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    W = m["W"]
    target = y[W // 2: y.shape[0] - W // 2].contiguous()
    plan = mod._plan_for(X, 0)
    P = {k: torch.tensor(d[k + "0"]) for k in fr.FACTORS}
    o = plan.offsets + [plan.num_params]
    # the data term alone: the flag off
    plan.set_smoothness(m["lambda_smooth"], m["smooth_diff_order"])
    plan.set_spectrum_penalty(0.0, None, 0, None)
    assert "path=conv-1pass-fmaf+fourier " in plan.describe and "model=conv_fourier" in plan.describe
    yh, (dl, dg), _ = _gpu_eval(plan, X, y, P, fr.lam3(m))
    assert fr.rel(yh, d["y_hat0"]) < RTOL
    assert abs(dl - float(d["loss_rec0"])) < RTOL * abs(float(d["loss_rec0"]))
    for f, k in enumerate(fr.phase_ref.ARENA):
        e = fr.rel(dg[o[f]:o[f + 1]], d["d" + k + "0"])
        print(f"{name} data grad {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    # the model's own setting
    mod._set_penalties(plan, target, m["lambda_spectralPenalty"], m["lambda_smooth"], m["smooth_diff_order"])
    if m["do_spectralPenalty"]:
        assert "path=conv-1pass-fmaf+fourier+spectrum-dft" in plan.describe
        e = fr.rel(mod.y_spectrum.cpu().numpy(), d["y_spectrum"])
        val, gy = plan.conv_spectrum_penalty(torch.tensor(d["y_hat0"], device=DEV))
        ev = abs(float(val) - float(d["loss_spectral0"])) / abs(float(d["loss_spectral0"]))
        eg = fr.rel(gy.cpu().numpy(), d["dpen_dyhat0"])
        print(f"{name} y_spectrum {e:.2e} penalty value {ev:.2e} d pen / d y_hat {eg:.2e}")
        assert e < RTOL and ev < RTOL and eg < RTOL
    else:
        assert mod.y_spectrum is None
    yh, (dl, _), (loss, g) = _gpu_eval(plan, X, y, P, fr.lam3(m))
    assert fr.rel(yh, d["y_hat0"]) < RTOL
    assert abs(dl - float(d["loss_rec0"])) < RTOL * abs(float(d["loss_rec0"]))  # the slot keeps loss_rec alone
    assert abs(loss - float(d["loss0"])) < RTOL * abs(float(d["loss0"]))
    for f, k in enumerate(fr.phase_ref.ARENA):
        e = fr.rel(g[o[f]:o[f + 1]], d["g" + k + "0"])
        print(f"{name} total grad {k}: {e:.2e}")
        assert e < RTOL, (k, e)


@pytest.mark.parametrize("name", fr.ADAM_FIXTURES)
def test_fixture_fit_adam(name):
    d = fr.load(name)
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    lam = fr.lam3(m)
    kw = _fit_kwargs(m)
    m10 = _model_from(d)
    m10.fit_Adam(X, y, lambda_L2=lam, Adam_kwargs=dict(m["adam_kwargs"]), **dict(kw, max_iter=min(10, m["max_iter"])))
    np.testing.assert_allclose(m10.loss_running, d["loss_running_10"], rtol=RTOL)
    for A, k in zip(list(m10.Bcp_w) + list(m10.Bcp_n) + [m10.bias], fr.FACTORS):
        assert fr.rel(A.detach().cpu().numpy(), d[k + "_10"]) < RTOL, k
    mod = _model_from(d)
    conv = mod.fit_Adam(X, y, lambda_L2=lam, Adam_kwargs=dict(m["adam_kwargs"]), **kw)
    assert isinstance(mod.optimizer, torch.optim.Adam)
    assert bool(conv) == bool(d["converged"])
    assert len(mod.loss_running) == len(d["loss_running"])
    print(f"{name} trajectory: {np.max(np.abs(np.asarray(mod.loss_running) - d['loss_running']) / d['loss_running']):.2e}")
    np.testing.assert_allclose(mod.loss_running, d["loss_running"], rtol=RTOL)
    for A, k in zip(list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias], fr.FACTORS):
        e = fr.rel(A.detach().cpu().numpy(), d[k + "_final"])
        print(f"{name} final {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    pred = mod.predict(X)
    assert isinstance(pred, torch.Tensor) and pred.device.type == "cpu" and not pred.requires_grad
    assert pred.shape == (m["T"] - m["W"] + 1, m["N"])
    assert fr.rel(pred.numpy(), d["predict_final"]) < RTOL
    assert fr.rel(mod.predict(X, Bcp=([None], [None])).numpy(), pred.numpy()) == 0.0  # Bcp is ignored


def test_fixture_lbfgs_fit():
    """fit (LBFGS, strong Wolfe) with a scalar lambda against the reference's fp32 trajectory, final
    factors and predict, to RTOL.  The fixture's LBFGS settings (one inner iteration per step) keep
    the fit well determined: tools/gen_golden_fourier.py asserts that the reference's own fp32 and
    fp64 runs agree to 1e-6 in the losses and every final factor."""
    d = fr.load("cfs_lbfgs")
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    mod = _model_from(d)
    conv = mod.fit(X, y, lambda_L2=m["lambda_L2"], running_loss_logging_interval=m["logging_interval"],
                   LBFGS_kwargs=dict(m["lbfgs_kwargs"]), **_fit_kwargs(m))
    assert isinstance(mod.optimizer, torch.optim.LBFGS)
    assert bool(conv) == bool(d["converged"])
    assert len(mod.loss_running) == len(d["loss_running"])
    print("lbfgs rel to fixture", np.abs(np.asarray(mod.loss_running) - d["loss_running"]) / d["loss_running"])
    np.testing.assert_allclose(mod.loss_running, d["loss_running"], rtol=RTOL)
    for A, k in zip(list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias], fr.FACTORS):
        e = fr.rel(A.detach().cpu().numpy(), d[k + "_final"])
        print(f"cfs_lbfgs final {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    assert fr.rel(mod.predict(X).numpy(), d["predict_final"]) < RTOL


def test_verbose_prints_variance_ratio(capsys):
    d = fr.load("cfs_base")
    mod = _model_from(d)
    mod.fit_Adam(torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV), lambda_L2=fr.lam3(d["meta"]),
                 max_iter=2, tol=0.0, patience=10, verbose=2, Adam_kwargs={'lr': 0.01})
    out = capsys.readouterr().out
    assert out.count("var_ratio (y_hat/y_true)") == 2 and "Iter: 1, loss:" in out


# ---- 2. the spectrum path alone -------------------------------------------------------------

SPECTRUM = [
    # (rows, n_fft, N, S)
    (1, 7, 1, 1),
    (93, 97, 3, 5),             # prime, odd
    (294, 300, 2, 9),           # even: Nyquist bin
    (295, 301, 1, 9),
    (8, 16, 2, 9),              # F = S: one row of M
    (50, 64, 64, 3),            # N = 64
    (1025, 1031, 2, 101),       # bins and rows past 256 / 1024 blocking
    (2040, 2048, 2, 101),
    (99971, 100003, 1, 101),    # a * b past 2^32
]
LAM_SP = 0.5


@functools.lru_cache(maxsize=None)
def _spectrum_reference(case):
    """series, target, g (fp32-representable) and M, M_y, value, gradient by torch.fft + autograd in fp64
    (tests/test_fourier_host.py ties that to the closed form)."""
    rows, n_fft, N, S = case
    gen = torch.Generator().manual_seed(3000 + rows)
    x = torch.randn(rows, N, generator=gen, dtype=torch.float64).float()
    tgt = torch.randn(rows, N, generator=gen, dtype=torch.float64).float()
    g = (torch.rand(S, generator=gen, dtype=torch.float64) + 0.5).float()
    spec = lambda s: torch.nn.functional.conv1d(  # noqa: E731
        torch.abs(torch.fft.rfft(s, n=n_fft, dim=0)).T[:, None, :], g.double()[None, None, :])[:, 0, :].T
    My = spec(tgt.double())
    xr = x.double().requires_grad_(True)
    M = spec(xr)
    pen = LAM_SP * torch.mean(((M - My) / (My + 1e-8)) ** 2)
    (gx,) = torch.autograd.grad(pen, xr)
    return x, tgt, g, M.detach().numpy(), My.numpy(), float(pen.detach()), gx.numpy()


@pytest.mark.parametrize("case", SPECTRUM, ids=lambda c: "x".join(map(str, c)))
def test_spectrum_path_against_fp64(case):
    rows, n_fft, N, S = case
    x, tgt, g, M_w, My_w, pen_w, gx_w = _spectrum_reference(case)
    assert My_w.min() > 0.5  # the 1e-8 floor is never in play (one row and one tap give 0.77; else >= 4.6)
    plan = _plan(1, 1, N, 1, 0, 1, rows, [False] * 3)
    shape = plan.set_spectrum_penalty(LAM_SP, g.numpy(), n_fft, tgt.to(DEV))
    assert shape == M_w.shape == (n_fft // 2 + 1 - S + 1, N)
    My = plan.conv_spectrum(tgt.to(DEV)).cpu().numpy()
    M = plan.conv_spectrum(x.to(DEV)).cpu().numpy()
    val, grad = plan.conv_spectrum_penalty(x.to(DEV))
    errs = (fr.rel(My, My_w), fr.rel(M, M_w), abs(float(val) - pen_w) / abs(pen_w), fr.rel(grad.cpu().numpy(), gx_w))
    print(f"spectrum {case}: M_y {errs[0]:.2e} M {errs[1]:.2e} value {errs[2]:.2e} gradient {errs[3]:.2e}")
    assert grad.shape == (rows, N) and max(errs) < RTOL, (case, errs)


# ---- 3. plan sweep against the fp64 restatement ---------------------------------------------

SWEEP = [
    # (T, D, W, N, Rn, Rs, C, ssf)
    (7, 1, 7, 1, 0, 1, 2, 1),         # T' = 1
    (263, 3, 7, 2, 2, 1, 2, 8),       # T' = 257
    (300, 3, 5, 2, 0, 16, 4, 8),      # 64 kernel columns
    (300, 3, 5, 2, 16, 16, 3, 8),     # R = 32, K = 64
    (520, 5, 257, 2, 2, 2, 2, 8),
    (332, 130, 33, 4, 3, 5, 3, 20),   # D chunks
    (1031, 5, 7, 2, 2, 2, 2, 100),
]
LAM = [0.01, 0.02, 0.03]
LAM_S, ORDER = 0.3, 2


def _inputs(case, seed=0):
    T, D, W, N, Rn, Rs, C = case[:7]
    g = torch.Generator().manual_seed(4000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    X = rn(T, D).float()
    y = rn(T, N).float()
    P = dict(Kn=rn(W, Rn) / W ** 0.5, Ks=rn(W, Rs, C) / W ** 0.5, Bd=rn(D, Rn + Rs) / D ** 0.5, Bo=rn(N, Rn + Rs),
             bias=0.1 * rn(N))
    P = {k: v.float() for k, v in P.items()}  # fp32-representable parameters, shared by both sides
    return X, y, P


def _spec_of(case, y, lam_sp=LAM_SP):
    """(n_fft, g, M_y, lam_sp) in fp64 with the fp32 gaussian the module builds."""
    T, W, ssf = case[0], case[2], case[7]
    g = fr.smoothing_kernel(ssf, torch.float32).double()
    return T, g, fr.spectrum(y.double()[W // 2: T - W // 2], T, g), lam_sp


@functools.lru_cache(maxsize=None)
def _reference(case, nn, lam_s=LAM_S, q=ORDER):
    """fp64 restatement with the penalty on, computed once per (case, flags, smoothness) and shared:
    (y_hat, loss_rec, pen, total, total gradient arena)."""
    X, y, P = _inputs(case)
    P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
    yh, (rec, pen, tot), g = fr.value_and_grads(X.double(), y.double(), P64, nn, LAM, lam_s, q, spec=_spec_of(case, y))
    return yh.numpy(), rec, pen, tot, fr.arena_of({k: v.numpy() for k, v in g.items()})


def _run_on(case, nn, lam_s=LAM_S, q=ORDER, lam_sp=LAM_SP):
    T, D, W, N, Rn, Rs, C, ssf = case
    X, y, P = _inputs(case)
    plan = _plan(W, D, N, Rn, Rs, C, T, list(nn), None, lam_s, q)
    yd = y.to(DEV)
    target = yd[W // 2: T - W // 2].contiguous()
    plan.set_spectrum_penalty(lam_sp, fr.smoothing_kernel(ssf, torch.float32).numpy(), T, target)
    got = _gpu_eval(plan, X.to(DEV), yd, P, LAM)
    val, _ = plan.conv_spectrum_penalty(torch.tensor(got[0], device=DEV))
    return got, float(val)


def _check(tag, got, val, want):
    yh, (dl, _), (tl, tg) = got
    yh_w, rec_w, pen_w, tot_w, tg_w = want
    errs = (fr.rel(yh, yh_w), abs(dl - rec_w) / abs(rec_w), abs(val - pen_w) / abs(pen_w), abs(tl - tot_w) / abs(tot_w),
            fr.rel(tg, tg_w))
    print(f"{tag}: y_hat {errs[0]:.2e} data loss {errs[1]:.2e} penalty {errs[2]:.2e} total loss {errs[3]:.2e} "
          f"total grads {errs[4]:.2e}")
    assert max(errs) < RTOL, (tag, errs)


@pytest.mark.parametrize("nn", [(False, False, False), (True, True, True)], ids=["fff", "ttt"])
@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "x".join(map(str, c)))
def test_sweep_against_fp64(case, nn):
    got, val = _run_on(case, nn)
    assert got[0].shape == (case[0] - case[2] + 1, case[3])
    _check(f"{case} {nn}", got, val, _reference(case, nn))


@pytest.mark.parametrize("q", [0, 1, 8])
def test_smoothness_orders_at_the_largest_columns(q):
    """W + q rows x 64 columns of Delta^q in the update kernel's dynamic LDS (265 x 64 at q = 8)."""
    case = (300, 2, 257, 2, 0, 16, 4, 8)
    got, val = _run_on(case, (False, False, False), 1.0, q)
    _check(f"order {q}", got, val, _reference(case, (False, False, False), 1.0, q))


# ---- 4. consistency ------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(332, 130, 33, 4, 3, 5, 3, 20), (300, 3, 5, 2, 0, 16, 4, 8)],
                         ids=lambda c: "x".join(map(str, c)))
def test_flag_off_is_the_conv_plan_bitwise_and_zero_lambda_is_flag_off(case):
    from tensor_regression_amd import _engine
    T, D, W, N, Rn, Rs, C, ssf = case
    X, y, P = _inputs(case)
    nn = [True, False, True]
    Xd, yd = X.to(DEV), y.to(DEV)
    target = yd[W // 2: T - W // 2].contiguous()
    conv = _engine.ConvPlan(W, D, N, Rn, Rs, C, T, nn, None, DEV)
    four = _plan(W, D, N, Rn, Rs, C, T, nn, None, LAM_S, ORDER)
    assert conv.offsets == four.offsets and conv.num_grads == four.num_grads

    def run(plan):
        arena = _arena(plan, P)
        g = torch.full((plan.num_grads,), float("nan"), device=DEV)
        yh = torch.empty_like(target)
        plan.loss_grad(Xd, target, None, float(target.numel()), arena, None, g, yhat=yh)
        return g.cpu(), yh.cpu()

    g_conv, yh_conv = run(conv)
    g_off, yh_off = run(four)
    assert torch.isfinite(g_off).all()
    assert torch.equal(g_conv, g_off) and torch.equal(yh_conv, yh_off)
    four.set_spectrum_penalty(0.0, fr.smoothing_kernel(ssf, torch.float32).numpy(), T, target)
    g_zero, yh_zero = run(four)
    assert torch.equal(g_zero, g_off) and torch.equal(yh_zero, yh_off)
    gt = [torch.zeros(four.num_params, device=DEV) for _ in range(2)]
    ls = [torch.zeros(1, device=DEV) for _ in range(2)]
    four.finalize_grad(_arena(four, P), g_zero.to(DEV), LAM, gt[0], ls[0])
    four.set_spectrum_penalty(0.0, None, 0, None)
    four.finalize_grad(_arena(four, P), g_off.to(DEV), LAM, gt[1], ls[1])
    assert torch.equal(gt[0], gt[1]) and torch.equal(ls[0], ls[1])


# ---- 5. determinism ------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(5008, 16, 9, 3, 2, 3, 2, 8), (108, 16, 9, 3, 2, 3, 2, 8)], ids=["many-wg", "one-wg"])
def test_loss_grad_is_bitwise_reproducible_with_the_penalty_on(case):
    T, D, W, N, Rn, Rs, C, ssf = case
    X, y, P = _inputs(case)
    plan = _plan(W, D, N, Rn, Rs, C, T, [True, False, False])
    Xd, yd = X.to(DEV), y.to(DEV)
    arena = _arena(plan, P)
    target = yd[W // 2: T - W // 2].contiguous()
    plan.set_spectrum_penalty(LAM_SP, fr.smoothing_kernel(ssf, torch.float32).numpy(), T, target)
    grads = []
    for _ in range(2):
        g = torch.full((plan.num_grads,), float("nan"), device=DEV)
        plan.loss_grad(Xd, target, None, float(target.numel()), arena, None, g)
        val, ge = plan.conv_spectrum_penalty(target)
        grads.append((g.cpu(), val.cpu(), ge.cpu()))
    assert torch.isfinite(grads[0][0]).all()
    for a, b in zip(grads[0], grads[1]):
        assert torch.equal(a, b)


# ---- 6. the plan and the ABI ---------------------------------------------------------------

def test_envelope_describe_and_call_order():
    from tensor_regression_amd import _engine, _lib
    with pytest.raises(ValueError, match="W <= 257"):
        _plan(259, 4, 2, 1, 1, 2, 600, [False] * 3)
    with pytest.raises(ValueError, match="<= 32"):
        _plan(7, 4, 2, 17, 16, 2, 600, [False] * 3)
    with pytest.raises(ValueError, match="K <= 64"):
        _plan(7, 4, 2, 8, 24, 4, 600, [False] * 3)
    plan = _plan(7, 4, 2, 1, 1, 2, 600, [False] * 3)
    assert "model=conv_fourier" in plan.describe and "path=conv-1pass-fmaf+fourier " in plan.describe
    assert plan.offsets == [0, 8, 12, 19, 33]  # Bd (4, 2) | Bo (2, 2) | Kn (7, 1) | Ks (7, 1, 2) | bias
    assert plan.num_params == 35 and plan.num_grads == 37
    with pytest.raises(ValueError, match="0..8"):
        plan.set_smoothness(0.1, 9)
    lib = _lib.load()
    ws0 = lib.tr_plan_workspace_bytes(plan.h)
    tgt = torch.randn(594, 2, device=DEV)
    g = np.ones(9, np.float32) / 9
    with pytest.raises(ValueError, match="first"):
        plan.conv_spectrum_penalty(tgt)
    with pytest.raises(ValueError, match="n_rows"):
        plan.set_spectrum_penalty(0.1, g, 500, tgt)       # n_rows > n_fft
    with pytest.raises(ValueError, match="longer"):
        plan.set_spectrum_penalty(0.1, g, 14, tgt[:10])   # n_fft / 2 + 1 < n_kernel
    plan.set_spectrum_penalty(0.1, np.ones(1025, np.float32), 4096, tgt)  # 1025 taps are accepted
    assert plan.set_spectrum_penalty(0.1, g, 600, tgt) == (293, 2)
    assert "path=conv-1pass-fmaf+fourier+spectrum-dft " in plan.describe and "n_fft=600" in plan.describe
    assert lib.tr_plan_workspace_bytes(plan.h) > ws0
    plan.set_spectrum_penalty(0.0, None, 0, None)
    assert "spectrum-dft" not in plan.describe and lib.tr_plan_workspace_bytes(plan.h) == ws0
    conv = _engine.ConvPlan(7, 4, 2, 1, 1, 2, 600, [False] * 3, None, DEV)
    ga = (ctypes.c_float * 9)(*g)
    assert lib.tr_plan_set_spectrum_penalty(conv.h, 0.1, ga, 9, 600, _lib.ptr(tgt), 594, None) == -1  # another model
    assert lib.tr_plan_set_smoothness(conv.h, 0.1, 2) == -1
    # a fresh Fourier plan: finalize needs both the L2 weights and the smoothness first
    h = ctypes.c_void_p()
    nn = (ctypes.c_int32 * 3)(0, 0, 0)
    assert lib.tr_plan_create_conv_fourier(ctypes.byref(h), 0, 7, 4, 2, 1, 1, 2, 600, nn, 50.0, 1.0) == 0
    try:
        par, grad, gtot = (torch.ones(40, device=DEV) for _ in range(3))
        m, v = torch.zeros(40, device=DEV), torch.zeros(40, device=DEV)

        def fin():
            return lib.tr_finalize_grad(h, _lib.ptr(par), _lib.ptr(grad), 0.0, _lib.ptr(gtot), None, None)

        def step():
            return lib.tr_adam_step(h, _lib.ptr(par), _lib.ptr(grad), _lib.ptr(m), _lib.ptr(v), None, 0.0, 0.01, 0.9,
                                    0.999, 1e-8, 0.0, 0, 1, None, 0, 0, 10, 0.0, None, None)

        assert fin() == -1 and b"tr_plan_set_l2_weights" in lib.tr_last_error()
        assert step() == -1 and b"tr_plan_set_l2_weights" in lib.tr_last_error()
        lam = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
        assert lib.tr_plan_set_l2_weights(h, lam, 3) == 0
        assert fin() == -1 and b"tr_plan_set_smoothness" in lib.tr_last_error()
        assert step() == -1 and b"tr_plan_set_smoothness" in lib.tr_last_error()
        assert lib.tr_plan_set_smoothness(h, 0.1, 2) == 0
        assert fin() == 0
        torch.cuda.synchronize()
    finally:
        assert lib.tr_plan_destroy(h) == 0


def test_lbfgs_verbose_lines_and_nan_stops(capsys):
    """fit's per-iteration line (verbose=2: the logged loss and the variance ratio, five significant
    digits each), its convergence line, and the NaN notice of both fits: a NaN target makes the first
    logged loss NaN and either fit stops there."""
    d = fr.load("cfs_lbfgs")
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    kw = dict(_fit_kwargs(m), lambda_L2=m["lambda_L2"], tol=0.0)
    lbfgs = dict(running_loss_logging_interval=1, LBFGS_kwargs=dict(m["lbfgs_kwargs"]))
    mod = _model_from(d)
    conv = mod.fit(X, y, **dict(kw, max_iter=2), verbose=2, **lbfgs)
    assert conv is False and len(mod.loss_running) == 2
    lines = capsys.readouterr().out.splitlines()
    for ii, loss in enumerate(mod.loss_running):
        head = f'Iter: {ii}, loss: {loss:.5}, var_ratio (y_hat/y_true): '
        assert lines[ii].startswith(head) and float(lines[ii][len(head):]) > 0, lines[ii]
    assert lines[2:] == ["Reached maximum number of iterations without convergence"]
    y[50, 1] = float("nan")
    for adam in (False, True):
        mod = _model_from(d)
        if adam:
            conv = mod.fit_Adam(X, y, **dict(kw, max_iter=3), Adam_kwargs={'lr': 0.01})
        else:
            conv = mod.fit(X, y, **dict(kw, max_iter=3), **lbfgs)
        assert conv is False and len(mod.loss_running) == 1 and np.isnan(mod.loss_running[0])
        assert capsys.readouterr().out == "Loss is NaN. Stopping.\n"
