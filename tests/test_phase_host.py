"""CPU-side checks of the phase-constrained spectral convolutional model: the constructor
reproduces the reference's draws bitwise, phase_shifter against its closed form and against the
fft expression, the smoothness term against its stencil, the test-local restatement (phase_ref)
against every pcs_* fixture (which the reference itself wrote), the module's own forward_model
against the fixtures, the quirk-compatible errors, and the C ABI's argument validation without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import phase_ref as pr

BAR = 1e-5  # the project's normwise parity bar


def _mod():
    from tensor_regression_amd import phase_constrained_spectral_convolutional_tensor_regression as M
    return M


def _model(d, device="cpu", **over):
    m = d["meta"]
    kw = dict(rank_normal=m["rank_normal"], temporal_window=m["W"], rank_spectral=m["rank_spectral"],
              non_negative=m["non_negative"], softplus_kwargs=m["softplus_kwargs"], device=device)
    kw.update(over)
    torch.manual_seed(m["seed"])
    return _mod().CP_linear_regression((m["T"], m["D"]), (m["T"], m["N"]), **kw)


@pytest.mark.parametrize("name", ["pcs_base", "pcs_rn0", "pcs_rs0", "pcs_r1", "pcs_w1", "pcs_nn_all", "pcs_zero"])
def test_constructor_matches_reference_draws(name):
    d = pr.load(name)
    m = d["meta"]
    mod = _model(d)
    W, D, N, Rn, Rs = m["W"], m["D"], m["N"], m["rank_normal"], m["rank_spectral"]
    assert tuple(mod.Bcp_w[0].shape) == (W, Rn) and tuple(mod.Bcp_w[1].shape) == (W, Rs)
    assert tuple(mod.Bcp_n[0].shape) == (D, Rn + Rs) and tuple(mod.Bcp_n[1].shape) == (N, Rn + Rs)
    assert tuple(mod.bias.shape) == (N,)
    assert np.array_equal(mod.idx_conv.numpy(), d["idx_conv"])
    for A, key in zip(list(mod.Bcp_w) + list(mod.Bcp_n), ("Kn_drawn", "Ks_drawn", "Bd_drawn", "Bo_drawn")):
        assert A.requires_grad
        assert np.array_equal(A.detach().numpy(), d[key]), key  # bitwise
    assert mod.weights.shape == (Rn + Rs,) and mod.loss_running == []
    assert mod.spectral_smoothing_kernel.shape == (101,) and mod.do_spectralPenalty is False


@pytest.mark.parametrize("W", [1, 3, 7, 33, 257])
def test_phase_shifter_is_the_closed_form_map(W):
    M = _mod()
    H = pr.quadrature_H(W)
    assert torch.allclose(H.T, -H, rtol=0, atol=1e-13)  # h is odd (sums of up to 128 sines in fp64)
    assert torch.allclose(M.quadrature_matrix(W), H, rtol=0, atol=1e-13)
    sh = M.phase_shifter(W, dtype=torch.float64)
    assert sh.signal_len == W and sh.angle_mask.shape == (W,)
    assert torch.equal(sh.angle_mask, torch.cat([-torch.ones((W + 1) // 2), torch.ones(W // 2)]).double())
    g = torch.Generator().manual_seed(W)
    k = torch.randn(W, 3, generator=g, dtype=torch.float64, requires_grad=True)
    out = sh(k, shift_angle=90, deg_or_rad='deg', dim=0)
    assert torch.allclose(out, H @ k, atol=1e-14)
    assert sh(k, shift_angle=0) is k
    # the expression the linear map stands for: real(ifft(fft(k) * exp(i * mask * angle))), any angle
    for ang in (np.pi / 2, 0.3):
        f = torch.fft.fft(k.detach(), dim=0) * torch.exp(1j * sh.angle_mask[:, None] * ang)
        want = torch.real(torch.fft.ifft(f, dim=0))
        assert torch.allclose(sh(k.detach(), shift_angle=ang, deg_or_rad='rad'), want, atol=1e-12)
    # adjoint: d <g, H k> / dk = H^T g = -H g
    gout = torch.randn(W, 3, generator=g, dtype=torch.float64)
    (gk,) = torch.autograd.grad((out * gout).sum(), k)
    assert torch.allclose(gk, -(H @ gout), atol=1e-14)
    # along another axis
    assert torch.allclose(sh(k.detach().T.contiguous(), dim=1), (H @ k.detach()).T, atol=1e-14)


@pytest.mark.parametrize("q", [0, 1, 2, 3])
def test_smoothness_penalty_is_the_stencil(q):
    M = _mod()
    g = torch.Generator().manual_seed(q)
    Kn = torch.randn(9, 2, generator=g, dtype=torch.float64, requires_grad=True)
    Ks = torch.randn(9, 3, generator=g, dtype=torch.float64, requires_grad=True)
    empty = torch.zeros(9, 0, dtype=torch.float64)
    d = M.diff_highOrder(Kn, q)
    assert d.shape == (9 + q, 2)
    assert torch.allclose(d, pr.stencil_diff(Kn, q), atol=1e-13)
    pen = M.smoothness_penalty([Kn, Ks], derivative_order=q, lambda_smooth=0.7)
    assert torch.allclose(pen, pr.smoothness(Kn, Ks, 0.7, q), atol=1e-13)
    assert torch.allclose(M.smoothness_penalty([Kn, empty], q, 0.7), pr.smoothness(Kn, empty, 0.7, q))  # skipped
    # the gradient the update kernel applies: (2 lambda / ((W + q) R)) (Delta^q)^T Delta^q F
    (gK,) = torch.autograd.grad(pen, Ks)
    dd = pr.stencil_diff(Ks.detach(), q)
    want = torch.zeros_like(Ks)
    for j in range(q + 1):
        want += pr.stencil_diff(torch.eye(1, dtype=torch.float64), q)[j, 0] * dd[j:j + 9]
    assert torch.allclose(gK, 2 * 0.7 / ((9 + q) * 3) * want, atol=1e-13)


@pytest.mark.parametrize("name", pr.ALL_FIXTURES)
def test_restatement_reproduces_fixture(name):
    """phase_ref (H from the closed form, the smoothness stencil) against what the reference computed,
    in fp32 and in fp64: this is what lets the GPU sweep use it as its yardstick."""
    d = pr.load(name)
    m = d["meta"]
    beta, thr = pr.softplus_of(m)
    for dtype in (torch.float32, torch.float64):
        X, y = torch.tensor(d["X"], dtype=dtype), torch.tensor(d["y"], dtype=dtype)
        P = pr.leaf_params(d, dtype)
        yh, loss, g = pr.value_and_grads(X, y, P, m["non_negative"], pr.lam3(m), m["lambda_smooth"],
                                         m["smooth_diff_order"], beta, thr)
        assert yh.shape == (m["T"] - m["W"] + 1, m["N"])
        assert pr.rel(yh.numpy(), d["y_hat0"]) < BAR
        assert abs(loss - float(d["loss0"])) < BAR * abs(float(d["loss0"]))
        for k in pr.FACTORS:
            assert pr.rel(g[k].numpy(), d["g" + k + "0"]) < BAR, (k, pr.rel(g[k].numpy(), d["g" + k + "0"]))
        P = pr.leaf_params(d, dtype)
        _, loss_rec, gd = pr.value_and_grads(X, y, P, m["non_negative"], None, beta=beta, thr=thr)
        assert abs(loss_rec - float(d["loss_rec0"])) < BAR * abs(float(d["loss_rec0"]))
        for k in pr.FACTORS:
            assert pr.rel(gd[k].numpy(), d["d" + k + "0"]) < BAR, k


def test_zero_kernel_fixture_pins_the_gradient_at_zero():
    d = pr.load("pcs_zero")
    assert not d["Ks0"].any() and d["Ks_drawn"].any()
    assert not d["dKs0"].any()  # the data term: abs / angle / norm give 0 at zero
    assert np.isnan(d["gKs0"]).all()  # the L2 term's sqrt at zero
    assert len(d["loss_running"]) == 2 and np.isnan(d["loss_running"][1]) and not d["converged"]


@pytest.mark.parametrize("name", ["pcs_base", "pcs_r1", "pcs_rs0", "pcs_nn_all", "pcs_w1"])
def test_forward_model_reproduces_fixture(name):
    M = _mod()
    d = pr.load(name)
    m = d["meta"]
    t = lambda k: torch.tensor(d[k + "0"])  # noqa: E731
    sh = M.phase_shifter(m["W"])
    yh = M.forward_model(torch.tensor(d["X"]), [t("Kn"), t("Ks")], sh, [t("Bd"), t("Bo")], None, m["non_negative"],
                         t("bias"), m["softplus_kwargs"])
    assert pr.rel(yh.numpy(), d["y_hat0"]) < BAR
    z = M.conv(torch.tensor(d["X"]), t("Kn"))
    assert z.shape == (m["T"] - m["W"] + 1, m["D"], m["rank_normal"])


def test_quirk_compatible_errors_and_params_round_trip():
    CP = _mod().CP_linear_regression
    with pytest.raises(ValueError, match="odd"):
        CP((50, 4), (50, 2), temporal_window=6)
    with pytest.raises(ValueError, match="2-D"):
        CP((50, 4), (50,), temporal_window=5)
    with pytest.raises(NotImplementedError):
        CP((50, 4), (50, 2), temporal_window=5, dtype=torch.float64)
    mod = CP((50, 4), (50, 2), temporal_window=5)
    X, y = torch.zeros(50, 4), torch.zeros(50, 2)
    with pytest.raises(TypeError, match="must be a mapping"):
        mod.fit(X, y, LBFGS_kwargs=None)
    with pytest.raises(NotImplementedError, match="process_group"):
        mod.fit_Adam(X, y, Adam_kwargs={'lr': 0.01}, process_group=object())

    class HostStream:
        pass

    with pytest.raises(NotImplementedError, match="HostStream"):
        mod.fit_Adam(HostStream(), y, Adam_kwargs={'lr': 0.01})
    # the output-spectrum penalty: stored, round-trips, and refused before any device work
    sp = CP((50, 4), (50, 2), temporal_window=5, do_spectralPenalty=True, spectrum_smoothing_factor=20)
    assert sp.do_spectralPenalty is True and sp.spectral_smoothing_kernel.shape == (21,)
    with pytest.raises(NotImplementedError, match="do_spectralPenalty"):
        sp.fit_Adam(X, y, Adam_kwargs={'lr': 0.01})
    with pytest.raises(NotImplementedError, match="do_spectralPenalty"):
        sp.fit(X, y, LBFGS_kwargs={'lr': 1})
    params = sp.get_params()
    assert params['do_spectralPenalty'] is True and params['temporal_window'] == 5
    other = CP((50, 4), (50, 2), temporal_window=5)
    other.set_params(params)
    assert other.do_spectralPenalty is True
    for a, b in zip(other.Bcp_w + other.Bcp_n, sp.Bcp_w + sp.Bcp_n):
        assert torch.equal(a, b.detach())
    assert torch.equal(other.spectral_smoothing_kernel, sp.spectral_smoothing_kernel)
    bn, bw = sp.detach_Bcp()
    assert [a.shape for a in bw] == [(5, 1), (5, 1)] and [a.shape for a in bn] == [(4, 2), (2, 2)]
    fn, fw = sp.return_Bcp_final()
    assert np.array_equal(fw[1], bw[1])  # non_negative off: the factors themselves


def test_phase_abi_rejects_bad_arguments_without_gpu():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    assert lib.tr_abi_version() == 9 and _lib.TR_ABI_VERSION == 9 and _lib.TR_MODEL_CONV_PHASE == 4
    h = ctypes.c_void_p()
    nn = (ctypes.c_int32 * 3)(0, 0, 0)

    def create(W=7, D=4, N=2, Rn=1, Rs=1, T=100, out=ctypes.byref(h)):
        return lib.tr_plan_create_conv_phase(out, 0, W, D, N, Rn, Rs, T, nn, 50.0, 1.0)

    for kw, word in [(dict(W=6), b"odd"), (dict(W=0), b"window"), (dict(Rn=0, Rs=0), b"rank"),
                     (dict(Rn=17, Rs=16), b"rank"), (dict(N=65), b"n_out"), (dict(out=None), b"NULL")]:
        assert create(**kw) == -1, kw
        assert word in lib.tr_last_error(), (kw, lib.tr_last_error())
    # beyond the kernel's envelope: unsupported, with the reason
    assert create(W=259, T=300) == -2 and b"W <= 257" in lib.tr_last_error()
    assert create(D=70000) == -2 and b"D <= 65536" in lib.tr_last_error()
    # "K <= 64" (the conv plan's other envelope word) cannot be reached here: with Rn + Rs <= 32 the
    # pair columns Rn + 2 Rs are at most 64, so the fullest shape passes the argument checks
    rc = create(Rn=0, Rs=32)
    assert rc >= 0
    if rc == 0:
        assert lib.tr_plan_destroy(h) == 0
    assert lib.tr_plan_set_smoothness(None, 0.1, 2) == -1 and b"NULL" in lib.tr_last_error()
    lam = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    assert lib.tr_plan_set_l2_weights(None, lam, 3) == -1
    if not torch.cuda.is_available():
        assert create() > 0 and lib.tr_last_error()  # a well-formed plan needs a device
