"""CPU-side checks of the convolutional Fourier model: the constructor reproduces the reference's
draws bitwise, the test-local restatement (fourier_ref: explicit DFT with integer angle indices, the
closed-form penalty gradient) against torch.fft + autograd and against every cfs_* fixture (which the
reference itself wrote), the module's own forward_model / spectral_penalty against the fixtures, the
errors the module raises in place of the reference's late failures, and the C ABI's argument
validation without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import fourier_ref as fr

BAR = 1e-5  # the project's normwise parity bar


def _mod():
    from tensor_regression_amd import convolutional_fourier_tensor_regression as M
    return M


def _model(d, device="cpu", **over):
    m = d["meta"]
    kw = dict(rank_normal=m["rank_normal"], temporal_window=m["W"], rank_spectral=m["rank_spectral"],
              non_negative=m["non_negative"], n_complex_dim=m["n_complex_dim"],
              do_spectralPenalty=m["do_spectralPenalty"], spectrum_smoothing_factor=m["spectrum_smoothing_factor"],
              softplus_kwargs=m["softplus_kwargs"], device=device)
    kw.update(over)
    torch.manual_seed(m["seed"])
    return _mod().CP_linear_regression((m["T"], m["D"]), (m["T"], m["N"]), **kw)


def test_module_is_exported():
    import tensor_regression_amd
    assert tensor_regression_amd.convolutional_fourier_tensor_regression is _mod()
    for name in ("make_BcpInit", "non_neg_fn", "gaussian", "conv", "complex_magnitude",
                 "stepwise_linear_model_multirank", "forward_model", "spectral_penalty", "L2_penalty",
                 "diff_highOrder", "smoothness_penalty", "CP_linear_regression"):
        assert hasattr(_mod(), name), name


@pytest.mark.parametrize("name", ["cfs_base", "cfs_rn0", "cfs_rs0", "cfs_c3", "cfs_nn_all", "cfs_ssf100", "cfs_off_c4"])
def test_constructor_matches_reference_draws(name):
    d = fr.load(name)
    m = d["meta"]
    mod = _model(d)
    W, D, N, Rn, Rs, C = m["W"], m["D"], m["N"], m["rank_normal"], m["rank_spectral"], m["n_complex_dim"] + 1
    assert tuple(mod.Bcp_w[0].shape) == (W, Rn) and tuple(mod.Bcp_w[1].shape) == (W, Rs, C)
    assert tuple(mod.Bcp_n[0].shape) == (D, Rn + Rs) and tuple(mod.Bcp_n[1].shape) == (N, Rn + Rs)
    assert tuple(mod.bias.shape) == (N,)
    assert np.array_equal(mod.idx_conv.numpy(), d["idx_conv"])
    for A, key in zip(list(mod.Bcp_w) + list(mod.Bcp_n), ("Kn_drawn", "Ks_drawn", "Bd_drawn", "Bo_drawn")):
        assert A.requires_grad
        assert np.array_equal(A.detach().numpy(), d[key]), key  # bitwise
    assert np.array_equal(mod.spectral_smoothing_kernel.numpy(), d["smoothing_kernel"])  # bitwise
    assert mod.weights.shape == (Rn + Rs,) and mod.loss_running == []
    assert mod.do_spectralPenalty is m["do_spectralPenalty"]
    assert torch.equal(fr.smoothing_kernel(m["spectrum_smoothing_factor"], torch.float32),
                       mod.spectral_smoothing_kernel)


@pytest.mark.parametrize("rows,n_fft,N,S", [(1, 7, 1, 1), (93, 97, 3, 5), (294, 300, 2, 9), (295, 301, 1, 9),
                                            (8, 16, 2, 9), (50, 64, 4, 3), (300, 300, 2, 21)])
def test_closed_form_penalty_gradient_is_autograd(rows, n_fft, N, S):
    """fourier_ref's explicit DFT, smoothing and closed-form gradient against torch.fft.rfft(n=n_fft) +
    the module's conv + autograd, fp64."""
    M = _mod()
    gen = torch.Generator().manual_seed(rows + n_fft)
    x = torch.randn(rows, N, generator=gen, dtype=torch.float64, requires_grad=True)
    tgt = torch.randn(rows, N, generator=gen, dtype=torch.float64)
    g = torch.rand(S, generator=gen, dtype=torch.float64) + 0.1
    My = M.conv(torch.abs(torch.fft.rfft(tgt, n=n_fft, dim=0)), g)
    assert My.shape == (n_fft // 2 + 1 - S + 1, N)
    assert torch.allclose(fr.spectrum(tgt, n_fft, g), My, rtol=1e-12, atol=1e-12)
    C, Sn, _ = fr.dft_parts(tgt, n_fft)
    Y = torch.fft.rfft(tgt, n=n_fft, dim=0)
    assert torch.allclose(C, Y.real, atol=1e-11) and torch.allclose(-Sn, Y.imag, atol=1e-11)
    pen = M.spectral_penalty(y_pred=x, y_true_fft=My, n_fft=n_fft, smoothing_kernel=g, lam=0.7)
    (gx,) = torch.autograd.grad(pen, x)
    val, grad = fr.spectrum_penalty_grad(x.detach(), n_fft, g, My, 0.7)
    assert torch.allclose(val, pen.detach(), rtol=1e-12)
    assert fr.rel(grad.numpy(), gx.numpy()) < 1e-11
    assert torch.allclose(fr.spectrum_penalty(x.detach(), n_fft, g, My, 0.7), pen.detach(), rtol=1e-12)
    assert float(M.spectral_penalty(x, passthrough=True)) == 0.0


def test_zero_bin_has_zero_gradient():
    """|Y| = 0 at a bin: torch's abs backward gives 0 there, and so does the closed form."""
    n = 8
    x = torch.zeros(n, 1, dtype=torch.float64)  # every bin is zero
    g = torch.ones(1, dtype=torch.float64)
    My = torch.ones(n // 2 + 1, 1, dtype=torch.float64)
    val, grad = fr.spectrum_penalty_grad(x, n, g, My, 1.0)
    assert torch.isfinite(grad).all() and not grad.any()
    xr = x.clone().requires_grad_(True)
    pen = _mod().spectral_penalty(y_pred=xr, y_true_fft=My, n_fft=n, smoothing_kernel=g, lam=1.0)
    (gx,) = torch.autograd.grad(pen, xr)
    assert not gx.any() and torch.allclose(val, pen.detach())


@pytest.mark.parametrize("name", fr.ALL_FIXTURES)
def test_restatement_reproduces_fixture(name):
    """fourier_ref against what the reference computed, in fp32 and in fp64: this is what lets the GPU
    tests use it as their yardstick."""
    d = fr.load(name)
    m = d["meta"]
    beta, thr = fr.softplus_of(m)
    for dtype in (torch.float32, torch.float64):
        X, y = torch.tensor(d["X"], dtype=dtype), torch.tensor(d["y"], dtype=dtype)
        spec = fr.fixture_spec(d, dtype)
        P = fr.leaf_params(d, dtype)
        yh, (rec, pen, loss), g = fr.value_and_grads(X, y, P, m["non_negative"], fr.lam3(m), m["lambda_smooth"],
                                                     m["smooth_diff_order"], beta, thr, spec)
        assert yh.shape == (m["T"] - m["W"] + 1, m["N"])
        assert fr.rel(yh.numpy(), d["y_hat0"]) < BAR
        assert abs(rec - float(d["loss_rec0"])) < BAR * abs(float(d["loss_rec0"]))
        assert abs(loss - float(d["loss0"])) < BAR * abs(float(d["loss0"]))
        for k in fr.FACTORS:
            assert fr.rel(g[k].numpy(), d["g" + k + "0"]) < BAR, (k, fr.rel(g[k].numpy(), d["g" + k + "0"]))
        P = fr.leaf_params(d, dtype)
        _, (rec, _, _), gd = fr.value_and_grads(X, y, P, m["non_negative"], None, beta=beta, thr=thr)
        assert abs(rec - float(d["loss_rec0"])) < BAR * abs(float(d["loss_rec0"]))
        for k in fr.FACTORS:
            assert fr.rel(gd[k].numpy(), d["d" + k + "0"]) < BAR, k
        if spec is not None:
            assert fr.rel(spec[2].numpy(), d["y_spectrum"]) < BAR
            assert abs(pen - float(d["loss_spectral0"])) < BAR * abs(float(d["loss_spectral0"]))
            val, grad = fr.spectrum_penalty_grad(torch.tensor(d["y_hat0"], dtype=dtype), *spec)
            assert abs(float(val) - float(d["loss_spectral0"])) < BAR * abs(float(d["loss_spectral0"]))
            assert fr.rel(grad.numpy(), d["dpen_dyhat0"]) < BAR
        else:
            assert pen == 0.0 and "y_spectrum" not in d


def test_converge_fixture_stops_before_max_iter():
    d = fr.load("cfs_converge")
    assert d["converged"] and len(d["loss_running"]) < d["meta"]["max_iter"]
    tail = d["loss_running"][-d["meta"]["patience"] + 1:]
    assert np.sum(np.abs(np.diff(tail))) < d["meta"]["tol"]


@pytest.mark.parametrize("name", ["cfs_base", "cfs_rn0", "cfs_rs0", "cfs_c3", "cfs_nn_all"])
def test_module_functions_reproduce_fixture(name):
    M = _mod()
    d = fr.load(name)
    m = d["meta"]
    t = lambda k: torch.tensor(d[k + "0"])  # noqa: E731
    yh = M.forward_model(torch.tensor(d["X"]), [t("Kn"), t("Ks")], [t("Bd"), t("Bo")], None, m["non_negative"],
                         t("bias"), m["softplus_kwargs"])
    assert fr.rel(yh.numpy(), d["y_hat0"]) < BAR
    pen = M.spectral_penalty(y_pred=yh, y_true_fft=torch.tensor(d["y_spectrum"]), n_fft=m["T"],
                             smoothing_kernel=torch.tensor(d["smoothing_kernel"]), lam=m["lambda_spectralPenalty"])
    assert abs(float(pen) - float(d["loss_spectral0"])) < BAR * abs(float(d["loss_spectral0"]))
    sm = M.smoothness_penalty([t("Kn"), t("Ks")], m["smooth_diff_order"], m["lambda_smooth"])
    assert abs(float(sm) - float(fr.smoothness(t("Kn"), t("Ks"), m["lambda_smooth"], m["smooth_diff_order"]))) < 1e-6


def test_errors_and_params_round_trip():
    CP = _mod().CP_linear_regression
    ok = dict(temporal_window=5, rank_normal=2, rank_spectral=2, n_complex_dim=1)
    with pytest.raises(ValueError, match="odd"):
        CP((50, 4), (50, 2), **{**ok, "temporal_window": 6})
    with pytest.raises(ValueError, match="2-D"):
        CP((50, 4), (50,), **ok)
    with pytest.raises(NotImplementedError):
        CP((50, 4), (50, 2), dtype=torch.float64, **ok)
    with pytest.raises(ValueError, match="reference's own forward_model fails"):
        CP((50, 4), (50, 2), **{**ok, "rank_normal": 1})
    with pytest.raises(ValueError, match="reference's own forward_model fails"):
        CP((50, 4), (50, 2), **{**ok, "n_complex_dim": 0})
    with pytest.raises(ValueError, match="reference's own forward_model fails"):
        CP((50, 4), (50, 2))  # the reference's own defaults: Rn = 1, Rs = 1, n_complex_dim = 0
    CP((50, 4), (50, 2), temporal_window=5, rank_normal=1, rank_spectral=0)  # these the reference runs
    CP((50, 4), (50, 2), temporal_window=5, rank_normal=0, rank_spectral=1, n_complex_dim=1)
    mod = CP((50, 4), (50, 2), **ok)
    X, y = torch.zeros(50, 4), torch.zeros(50, 2)
    with pytest.raises(TypeError, match="must be a mapping"):
        mod.fit(X, y, LBFGS_kwargs=None)
    with pytest.raises(NotImplementedError, match="process_group"):
        mod.fit_Adam(X, y, Adam_kwargs={'lr': 0.01}, process_group=object())
    with pytest.raises(NotImplementedError, match="verbose == 3"):
        mod.fit_Adam(X, y, Adam_kwargs={'lr': 0.01}, verbose=3)
    with pytest.raises(NotImplementedError, match="verbose == 3"):
        mod.fit(X, y, LBFGS_kwargs={'lr': 1}, verbose=3)

    class HostStream:
        pass

    with pytest.raises(NotImplementedError, match="HostStream"):
        mod.fit_Adam(HostStream(), y, Adam_kwargs={'lr': 0.01})
    with pytest.raises(NotImplementedError, match="HostStream"):
        mod.predict(HostStream())
    # F < S: 26 bins, 101 taps; refused before any device work
    sp = CP((50, 4), (50, 2), do_spectralPenalty=True, **ok)
    assert sp.do_spectralPenalty is True and sp.spectral_smoothing_kernel.shape == (101,)
    with pytest.raises(ValueError, match="bins"):
        sp.fit_Adam(X, y, Adam_kwargs={'lr': 0.01})
    with pytest.raises(ValueError, match="bins"):
        sp.fit(X, y, LBFGS_kwargs={'lr': 1})
    sp = CP((50, 4), (50, 2), do_spectralPenalty=True, spectrum_smoothing_factor=20, **ok)
    with pytest.raises(ValueError, match="n_fft"):
        sp.fit_Adam(torch.zeros(60, 4), torch.zeros(60, 2), Adam_kwargs={'lr': 0.01})
    params = sp.get_params()
    assert params['do_spectralPenalty'] is True and params['temporal_window'] == 5
    assert set(params) == {'X_shape', 'y_shape', 'dtype', 'device', 'weights', 'Bcp_n', 'Bcp_w', 'bias', 'non_negative',
                           'softplus_kwargs', 'rank', 'rank_normal', 'rank_spectral', 'idxConv',
                           'spectral_smoothing_kernel', 'temporal_window', 'do_spectralPenalty', 'loss_running'}
    other = CP((50, 4), (50, 2), **ok)
    other.set_params(params)
    assert other.do_spectralPenalty is True
    for a, b in zip(other.Bcp_w + other.Bcp_n, sp.Bcp_w + sp.Bcp_n):
        assert torch.equal(a, b.detach())
    assert torch.equal(other.spectral_smoothing_kernel, sp.spectral_smoothing_kernel)
    assert other.spectral_smoothing_kernel.shape == (21,)
    bn, bw = sp.detach_Bcp()
    assert [a.shape for a in bw] == [(5, 2), (5, 2, 2)] and [a.shape for a in bn] == [(4, 4), (2, 4)]
    fn, fw = sp.return_Bcp_final()
    assert np.array_equal(fw[1], bw[1])  # non_negative off: the factors themselves


def test_fourier_abi_rejects_bad_arguments_without_gpu():
    """The new entry points exist (they do not on a library without the Fourier model) and validate
    their arguments before any device call."""
    from tensor_regression_amd import _lib
    lib = _lib.load()
    assert lib.tr_abi_version() == 9 and _lib.TR_ABI_VERSION == 9 and _lib.TR_MODEL_CONV_FOURIER == 5
    for sym in ("tr_plan_create_conv_fourier", "tr_plan_set_spectrum_penalty", "tr_conv_spectrum",
                "tr_conv_spectrum_penalty"):
        assert sym in _lib.SIGNATURES and getattr(lib, sym) is not None
    h = ctypes.c_void_p()
    nn = (ctypes.c_int32 * 3)(0, 0, 0)

    def create(W=7, D=4, N=2, Rn=1, Rs=1, C=2, T=100, out=ctypes.byref(h)):
        return lib.tr_plan_create_conv_fourier(out, 0, W, D, N, Rn, Rs, C, T, nn, 50.0, 1.0)

    for kw, word in [(dict(W=6), b"odd"), (dict(W=0), b"window"), (dict(Rn=0, Rs=0), b"rank"),
                     (dict(Rn=17, Rs=16), b"rank"), (dict(N=65), b"n_out"), (dict(C=5), b"n_complex"),
                     (dict(C=0), b"n_complex"), (dict(out=None), b"NULL"), (dict(T=5), b"max_series_rows")]:
        assert create(**kw) == -1, kw
        assert word in lib.tr_last_error(), (kw, lib.tr_last_error())
    assert create(W=259, T=300) == -2 and b"W <= 257" in lib.tr_last_error()
    assert create(D=70000) == -2 and b"D <= 65536" in lib.tr_last_error()
    assert create(Rn=8, Rs=24, C=4) == -2 and b"K <= 64" in lib.tr_last_error()
    g = (ctypes.c_float * 3)(0.25, 0.5, 0.25)
    assert lib.tr_plan_set_spectrum_penalty(None, 0.1, g, 3, 64, None, 10, None) == -1 and b"NULL" in lib.tr_last_error()
    assert lib.tr_conv_spectrum(None, None, 10, None, None) == -1 and b"NULL" in lib.tr_last_error()
    assert lib.tr_conv_spectrum_penalty(None, None, 10, None, None, None) == -1 and b"NULL" in lib.tr_last_error()
    assert lib.tr_plan_set_smoothness(None, 0.1, 2) == -1
    if not torch.cuda.is_available():
        assert create() > 0 and lib.tr_last_error()  # a well-formed plan needs a device
