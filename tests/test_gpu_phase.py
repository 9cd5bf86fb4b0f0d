"""GPU checks of the phase-constrained spectral convolutional model (tensor_regression_amd.
phase_constrained_spectral_convolutional_tensor_regression; kernels k_phase_kp and k_phase_finish
in csrc/tr_conv_phase.hip around k_conv and k_update_conv of csrc/tr_conv.hip).

  * fixture parity (tests/golden/pcs_*.npz, written by the reference) through the public class:
    y_hat0, loss0, every gradient (total and data term alone), the 10-step and full loss
    trajectories, the final factors, `converged`, predict
  * a shape sweep against the fp64 restatement of tests/phase_ref.py (qualified against the fixtures
    by tests/test_phase_host.py): loss 1e-5 relative, y_hat and the gradient arenas 1e-5 normwise
  * run-to-run bitwise determinism, consistency with the merged conv plan at C = 2, the smoothness
    orders at the LDS-largest shape, the ABI's order of calls

Bars: RTOL = 1e-5 as in tests/test_gpu_conv.py, unchanged.
"""
import ctypes
import functools

import numpy as np
import pytest
import torch

import phase_ref as pr

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5


def _plan(W, D, N, Rn, Rs, T, nn, softplus=None, lam_s=0.0, q=2):
    from tensor_regression_amd import _engine
    return _engine.ConvPhasePlan(W, D, N, Rn, Rs, T, nn, softplus, DEV, lam_s, q)


def _gpu_eval(plan, X, y, P, lam):
    """y_hat, (data loss, data-term gradient arena), (total loss, total gradient arena) as numpy."""
    W = plan.dims[0]
    dev = lambda a: a.detach().to(DEV, torch.float32).contiguous()  # noqa: E731
    arena = plan.pack([dev(P["Kn"]), dev(P["Ks"])], [dev(P["Bd"]), dev(P["Bo"])], dev(P["bias"]))
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
    from tensor_regression_amd.phase_constrained_spectral_convolutional_tensor_regression import \
        CP_linear_regression
    m = d["meta"]
    t = lambda a: torch.tensor(a, device=DEV).requires_grad_(True)  # noqa: E731
    return CP_linear_regression((m["T"], m["D"]), (m["T"], m["N"]), rank_normal=m["rank_normal"],
                                temporal_window=m["W"], rank_spectral=m["rank_spectral"],
                                non_negative=m["non_negative"],
                                Bcp_init=([t(d["Kn0"]), t(d["Ks0"])], [t(d["Bd0"]), t(d["Bo0"])]), device=DEV,
                                softplus_kwargs=m["softplus_kwargs"])


def _fit_kwargs(m):
    return dict(lambda_smooth=m["lambda_smooth"], smooth_diff_order=m["smooth_diff_order"], max_iter=m["max_iter"],
                tol=m["tol"], patience=m["patience"])


@pytest.mark.parametrize("name", pr.ALL_FIXTURES)
def test_fixture_first_step(name):
    d = pr.load(name)
    m = d["meta"]
    mod = _model_from(d)
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    plan = mod._plan_for(X, 0)
    plan.set_smoothness(m["lambda_smooth"], m["smooth_diff_order"])
    assert "model=conv_phase" in plan.describe and "path=conv-1pass-fmaf+phase" in plan.describe
    P = {k: torch.tensor(d[k + "0"]) for k in pr.FACTORS}
    yh, (dl, dg), (loss, g) = _gpu_eval(plan, X, y, P, pr.lam3(m))
    assert pr.rel(yh, d["y_hat0"]) < RTOL
    assert abs(dl - float(d["loss_rec0"])) < RTOL * abs(float(d["loss_rec0"]))
    assert abs(loss - float(d["loss0"])) < RTOL * abs(float(d["loss0"]))
    o = plan.offsets + [plan.num_params]
    for f, k in enumerate(pr.ARENA):
        e_d, e_g = pr.rel(dg[o[f]:o[f + 1]], d["d" + k + "0"]), pr.rel(g[o[f]:o[f + 1]], d["g" + k + "0"])
        print(f"{name} grad {k}: data {e_d:.2e} total {e_g:.2e}")
        assert e_d < RTOL and e_g < RTOL, (k, e_d, e_g)


@pytest.mark.parametrize("name", pr.ADAM_FIXTURES)
def test_fixture_fit_adam(name):
    d = pr.load(name)
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    lam = pr.lam3(m)
    kw = _fit_kwargs(m)
    m10 = _model_from(d)
    m10.fit_Adam(X, y, lambda_L2=lam, Adam_kwargs=dict(m["adam_kwargs"]), **dict(kw, max_iter=min(10, m["max_iter"])))
    np.testing.assert_allclose(m10.loss_running, d["loss_running_10"], rtol=RTOL)
    for A, k in zip(list(m10.Bcp_w) + list(m10.Bcp_n) + [m10.bias], pr.FACTORS):
        assert pr.rel(A.detach().cpu().numpy(), d[k + "_10"]) < RTOL, k
    mod = _model_from(d)
    conv = mod.fit_Adam(X, y, lambda_L2=lam, Adam_kwargs=dict(m["adam_kwargs"]), **kw)
    assert isinstance(mod.optimizer, torch.optim.Adam)
    assert bool(conv) == bool(d["converged"])
    assert len(mod.loss_running) == len(d["loss_running"])
    np.testing.assert_allclose(mod.loss_running, d["loss_running"], rtol=RTOL)
    for A, k in zip(list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias], pr.FACTORS):
        e = pr.rel(A.detach().cpu().numpy(), d[k + "_final"])
        print(f"{name} final {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    pred = mod.predict(X)
    assert isinstance(pred, torch.Tensor) and pred.device.type == "cpu" and not pred.requires_grad
    assert pred.shape == (m["T"] - m["W"] + 1, m["N"])
    assert pr.rel(pred.numpy(), d["predict_final"]) < RTOL
    # predict == the training kernel's y_hat at the final factors (same softplus_kwargs)
    plan = mod._plan_for(X, 0)
    P = {k: A.detach().cpu() for k, A in zip(pr.FACTORS, list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias])}
    yh = _gpu_eval(plan, X, y, P, lam)[0]
    assert pred.numpy().shape == yh.shape and pr.rel(pred.numpy(), yh) < 1e-6


def test_fixture_lbfgs_fit():
    """fit (LBFGS, strong Wolfe) with a scalar lambda against the reference's fp32 trajectory, final
    factors and predict, to RTOL.  The fixture's LBFGS settings (one inner iteration per step) keep
    the fit well determined: tools/gen_golden_phase.py asserts that the reference's own fp32 and
    fp64 runs agree to 1e-6 in the losses and every final factor."""
    d = pr.load("pcs_lbfgs")
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
    for A, k in zip(list(mod.Bcp_w) + list(mod.Bcp_n) + [mod.bias], pr.FACTORS):
        e = pr.rel(A.detach().cpu().numpy(), d[k + "_final"])
        print(f"pcs_lbfgs final {k}: {e:.2e}")
        assert e < RTOL, (k, e)
    assert pr.rel(mod.predict(X).numpy(), d["predict_final"]) < RTOL


def test_scalar_lambda_and_nan_stop(capsys):
    d = pr.load("pcs_base")
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    runs = []
    for lam in (0.02, [0.02], [0.02, 0.02, 0.02]):
        mod = _model_from(d)
        mod.fit_Adam(X, y, lambda_L2=lam, lambda_smooth=0.05, max_iter=3, tol=0.0, Adam_kwargs={'lr': 0.01})
        runs.append(list(mod.loss_running))
    assert runs[0] == runs[2] and runs[1] == runs[2] and len(runs[0]) == 3
    # pcs_zero: the reference's second loss is NaN and its loop stops there, not converged
    z = pr.load("pcs_zero")
    mz = z["meta"]
    mod = _model_from(z)
    conv = mod.fit_Adam(torch.tensor(z["X"], device=DEV), torch.tensor(z["y"], device=DEV), lambda_L2=pr.lam3(mz),
                        Adam_kwargs=dict(mz["adam_kwargs"]), **_fit_kwargs(mz))
    assert conv is False and len(mod.loss_running) == 2 and np.isnan(mod.loss_running[1])
    assert "Loss is NaN. Stopping." in capsys.readouterr().out


def test_verbose_prints_variance_ratio(capsys):
    d = pr.load("pcs_base")
    mod = _model_from(d)
    mod.fit_Adam(torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV), lambda_L2=pr.lam3(d["meta"]),
                 max_iter=2, tol=0.0, patience=10, verbose=2, Adam_kwargs={'lr': 0.01})
    out = capsys.readouterr().out
    assert out.count("var_ratio (y_hat/y_true)") == 2 and "Iter: 1, loss:" in out


# ---- 2. shape sweep against the fp64 restatement -------------------------------------------

SWEEP = [
    # (T, D, W, N, Rn, Rs)
    (7, 1, 7, 1, 0, 1),         # T' = 1
    (263, 3, 7, 2, 1, 1),       # T' = 257: one time past a tile
    (300, 4, 3, 2, 0, 9),       # 18 pair columns across two groups
    (300, 3, 5, 2, 0, 32),      # K = 64
    (300, 3, 5, 2, 17, 15),     # R = 32
    (520, 5, 257, 2, 1, 2),     # the largest h
    (332, 130, 33, 4, 3, 5),    # D chunks
]
LAM = [0.01, 0.02, 0.03]
LAM_S, ORDER = 0.3, 2


def _inputs(case, seed=0):
    T, D, W, N, Rn, Rs = case
    g = torch.Generator().manual_seed(2000 + seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)  # noqa: E731
    X = rn(T, D).float()
    y = rn(T, N).float()
    P = dict(Kn=rn(W, Rn) / W ** 0.5, Ks=rn(W, Rs) / W ** 0.5, Bd=rn(D, Rn + Rs) / D ** 0.5, Bo=rn(N, Rn + Rs),
             bias=0.1 * rn(N))
    P = {k: v.float() for k, v in P.items()}  # fp32-representable parameters, shared by both sides
    return X, y, P


@functools.lru_cache(maxsize=None)
def _reference(case, nn, lam_s=LAM_S, q=ORDER):
    """fp64 restatement, computed once per (case, flags, smoothness) and shared."""
    X, y, P = _inputs(case)
    out = []
    for lam in (None, LAM):
        P64 = {k: v.double().requires_grad_(True) for k, v in P.items()}
        yh, loss, g = pr.value_and_grads(X.double(), y.double(), P64, nn, lam, lam_s, q)
        out.append((yh.numpy(), loss, pr.arena_of({k: v.numpy() for k, v in g.items()})))
    return out


def _check(tag, got, want):
    yh, (dl, dg), (tl, tg) = got
    (yh_w, dl_w, dg_w), (_, tl_w, tg_w) = want
    errs = (pr.rel(yh, yh_w), abs(dl - dl_w) / abs(dl_w), pr.rel(dg, dg_w), abs(tl - tl_w) / abs(tl_w),
            pr.rel(tg, tg_w))
    print(f"{tag}: y_hat {errs[0]:.2e} data loss {errs[1]:.2e} data grads {errs[2]:.2e} total loss {errs[3]:.2e} "
          f"total grads {errs[4]:.2e}")
    assert max(errs) < RTOL, (tag, errs)


NN_CASES = [(SWEEP[i], nn) for i in range(len(SWEEP)) for nn in ((False, False, False), (True, True, True))] + \
    [(SWEEP[1], nn) for nn in ((True, False, False), (False, True, False), (False, False, True))]


@pytest.mark.parametrize("case,nn", NN_CASES,
                         ids=lambda v: "".join("ft"[b] for b in v) if isinstance(v[0], bool) else "x".join(map(str, v)))
def test_sweep_against_fp64(case, nn):
    T, D, W, N, Rn, Rs = case
    X, y, P = _inputs(case)
    plan = _plan(W, D, N, Rn, Rs, T, list(nn), None, LAM_S, ORDER)
    got = _gpu_eval(plan, X.to(DEV), y.to(DEV), P, LAM)
    assert got[0].shape == (T - W + 1, N)
    _check(f"{case} {nn}", got, _reference(case, nn))


@pytest.mark.parametrize("q", [0, 1, 8])
def test_smoothness_orders_at_the_largest_columns(q):
    """W + q rows x 32 columns of Delta^q in the update kernel's LDS (265 x 32 at q = 8)."""
    case = (300, 2, 257, 2, 16, 16)
    X, y, P = _inputs(case)
    plan = _plan(257, 2, 2, 16, 16, 300, [False] * 3, None, 1.0, q)
    got = _gpu_eval(plan, X.to(DEV), y.to(DEV), P, LAM)
    _check(f"order {q}", got, _reference(case, (False, False, False), 1.0, q))


# ---- 3. determinism ------------------------------------------------------------------------

@pytest.mark.parametrize("case", [(5008, 16, 9, 3, 2, 3), (108, 16, 9, 3, 2, 3)], ids=["many-wg", "one-wg"])
def test_loss_grad_is_bitwise_reproducible(case):
    T, D, W, N, Rn, Rs = case
    X, y, P = _inputs(case)
    plan = _plan(W, D, N, Rn, Rs, T, [True, False, False])
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


# ---- 4. consistency with the merged conv model ---------------------------------------------

@pytest.mark.parametrize("case", [(332, 130, 33, 4, 3, 5), (300, 4, 3, 2, 0, 9)], ids=lambda c: "x".join(map(str, c)))
def test_matches_conv_plan_with_the_pair_built_on_the_host(case):
    """A ConvPlan with C = 2 whose Ks is [k, H k], H k built on the host in fp64: same y_hat."""
    from tensor_regression_amd import _engine
    T, D, W, N, Rn, Rs = case
    X, y, P = _inputs(case)
    nn = [False, True, True]
    phase = _plan(W, D, N, Rn, Rs, T, nn)
    conv = _engine.ConvPlan(W, D, N, Rn, Rs, 2, T, nn, None, DEV)
    Hk = (pr.quadrature_H(W) @ P["Ks"].double()).float()
    dev = lambda a: a.to(DEV).contiguous()  # noqa: E731
    a_phase = phase.pack([dev(P["Kn"]), dev(P["Ks"])], [dev(P["Bd"]), dev(P["Bo"])], dev(P["bias"]))
    a_conv = conv.pack([dev(P["Kn"]), dev(torch.stack([P["Ks"], Hk], dim=-1))], [dev(P["Bd"]), dev(P["Bo"])],
                       dev(P["bias"]))
    yp = phase.forward(X.to(DEV), a_phase).cpu().numpy()
    yc = conv.forward(X.to(DEV), a_conv).cpu().numpy()
    e = pr.rel(yp, yc)
    print(f"{case}: phase plan from conv plan {e:.2e}")
    assert yp.shape == yc.shape == (T - W + 1, N) and e < 1e-6


# ---- 5. the plan and the ABI ---------------------------------------------------------------

def test_envelope_describe_and_call_order():
    from tensor_regression_amd import _engine, _lib
    with pytest.raises(ValueError, match="W <= 257"):
        _plan(259, 4, 2, 1, 1, 600, [False] * 3)
    with pytest.raises(ValueError, match="<= 32"):
        _plan(7, 4, 2, 17, 16, 600, [False] * 3)
    plan = _plan(7, 4, 2, 1, 1, 600, [False] * 3)
    assert "model=conv_phase" in plan.describe and "path=conv-1pass-fmaf+phase" in plan.describe
    assert plan.offsets == [0, 8, 12, 19, 26]  # Bd (4, 2) | Bo (2, 2) | Kn (7, 1) | Ks (7, 1) | bias
    assert plan.num_params == 28 and plan.num_grads == 30
    with pytest.raises(ValueError, match="0..8"):
        plan.set_smoothness(0.1, 9)
    lib = _lib.load()
    conv = _engine.ConvPlan(7, 4, 2, 1, 1, 2, 600, [False] * 3, None, DEV)
    assert lib.tr_plan_set_smoothness(conv.h, 0.1, 2) == -1  # a plan of another model
    # a fresh phase plan: finalize needs both the L2 weights and the smoothness first
    h = ctypes.c_void_p()
    nn = (ctypes.c_int32 * 3)(0, 0, 0)
    assert lib.tr_plan_create_conv_phase(ctypes.byref(h), 0, 7, 4, 2, 1, 1, 600, nn, 50.0, 1.0) == 0
    try:
        par, grad, gtot = (torch.ones(32, device=DEV) for _ in range(3))

        def fin():
            return lib.tr_finalize_grad(h, _lib.ptr(par), _lib.ptr(grad), 0.0, _lib.ptr(gtot), None, None)

        assert fin() == -1 and b"tr_plan_set_l2_weights" in lib.tr_last_error()
        lam = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
        assert lib.tr_plan_set_l2_weights(h, lam, 3) == 0
        assert fin() == -1 and b"tr_plan_set_smoothness" in lib.tr_last_error()
        assert lib.tr_plan_set_smoothness(h, 0.1, 2) == 0
        assert fin() == 0
        torch.cuda.synchronize()
    finally:
        assert lib.tr_plan_destroy(h) == 0


def test_lbfgs_verbose_lines_and_nan_stop(capsys):
    """fit's per-iteration line (verbose=2: the logged loss and the variance ratio, five significant
    digits each), its convergence line, and its NaN notice: a NaN target makes the first logged loss
    NaN and the fit stops there."""
    d = pr.load("pcs_lbfgs")
    m = d["meta"]
    X, y = torch.tensor(d["X"], device=DEV), torch.tensor(d["y"], device=DEV)
    kw = dict(lambda_L2=m["lambda_L2"], lambda_smooth=m["lambda_smooth"], smooth_diff_order=m["smooth_diff_order"],
              tol=0.0, running_loss_logging_interval=1, LBFGS_kwargs=dict(m["lbfgs_kwargs"]))
    mod = _model_from(d)
    conv = mod.fit(X, y, max_iter=2, verbose=2, **kw)
    assert conv is False and len(mod.loss_running) == 2
    lines = capsys.readouterr().out.splitlines()
    for ii, loss in enumerate(mod.loss_running):
        head = f'Iter: {ii}, loss: {loss:.5}, var_ratio (y_hat/y_true): '
        assert lines[ii].startswith(head) and float(lines[ii][len(head):]) > 0, lines[ii]
    assert lines[2:] == ["Reached maximum number of iterations without convergence"]
    y[50, 1] = float("nan")
    mod = _model_from(d)
    conv = mod.fit(X, y, max_iter=3, **kw)
    assert conv is False and len(mod.loss_running) == 1 and np.isnan(mod.loss_running[0])
    assert capsys.readouterr().out == "Loss is NaN. Stopping.\n"
