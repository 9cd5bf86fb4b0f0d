"""CPU-side checks of the convolutional spectral model: the test-local restatement (conv_ref) is
qualified in fp32 against every cvs_* fixture (which the reference itself wrote), the class's
constructor reproduces the fixtures' initial factors bitwise, the quirk-compatible errors, and the
C ABI's argument validation without a GPU."""
import ctypes

import numpy as np
import pytest
import torch

import conv_ref as cr

BAR = 1e-5  # the project's normwise parity bar


@pytest.mark.parametrize("name", cr.ALL_FIXTURES)
def test_restatement_reproduces_fixture_fp32(name):
    d = cr.load(name)
    m = d["meta"]
    X, y = torch.tensor(d["X"]), torch.tensor(d["y"])
    beta, thr = cr.fit_softplus(m)
    P = cr.leaf_params(d, torch.float32)
    yh, loss, g = cr.value_and_grads(X, y, P, m["non_negative"], cr.lam3(m), beta, thr)
    assert yh.shape == (m["T"] - m["W"] + 1, m["N"])
    assert cr.rel(yh.numpy(), d["y_hat0"]) < BAR
    assert abs(loss - float(d["loss0"])) < BAR * abs(float(d["loss0"]))
    for k in cr.FACTORS:
        assert g[k].shape == d["g" + k + "0"].shape or g[k].numel() == d["g" + k + "0"].size
        assert cr.rel(g[k].numpy(), d["g" + k + "0"]) < BAR, k
    if m["lbfgs_kwargs"] is None:
        P = cr.leaf_params(d, torch.float32)
        losses = cr.adam_losses(X, y, P, m["non_negative"], cr.lam3(m), m["adam_kwargs"], len(d["loss_running_10"]))
        np.testing.assert_allclose(losses, d["loss_running_10"], rtol=BAR)


def _model(d, device="cpu", **over):
    from tensor_regression_amd.convolutional_spectral_tensor_regression import CP_linear_regression
    m = d["meta"]
    kw = dict(rank_normal=m["rank_normal"], temporal_window=m["W"], rank_spectral=m["rank_spectral"],
              non_negative=m["non_negative"], n_complex_dim=m["n_complex_dim"], softplus_kwargs=m["softplus_kwargs"],
              device=device)
    kw.update(over)
    torch.manual_seed(m["seed"])
    return CP_linear_regression((m["T"], m["D"]), (m["T"], m["N"]), **kw)


@pytest.mark.parametrize("name", ["cvs_base", "cvs_nn_all", "cvs_c1", "cvs_c3", "cvs_rn0", "cvs_rs0"])
def test_constructor_matches_reference_draws(name):
    d = cr.load(name)
    m = d["meta"]
    mod = _model(d)
    W, D, N, Rn, Rs, C = m["W"], m["D"], m["N"], m["rank_normal"], m["rank_spectral"], m["n_complex_dim"] + 1
    assert tuple(mod.Bcp_w[0].shape) == (W, Rn)
    assert tuple(mod.Bcp_w[1].shape) == ((W, Rs) if C == 1 else (W, Rs, C))
    assert tuple(mod.Bcp_n[0].shape) == (D, Rn + Rs) and tuple(mod.Bcp_n[1].shape) == (N, Rn + Rs)
    assert tuple(mod.bias.shape) == (N,)
    assert torch.equal(mod.idx_conv, torch.arange(W // 2, m["T"] - W // 2))
    assert np.array_equal(mod.idx_conv.numpy(), d["idx_conv"])
    for A, key in zip(list(mod.Bcp_w) + list(mod.Bcp_n), ("Kn0", "Ks0", "Bd0", "Bo0")):
        assert A.requires_grad
        assert np.array_equal(A.detach().numpy(), d[key]), key  # bitwise
    assert mod.weights.shape == (Rn + Rs,) and mod.loss_running == []


def test_quirk_compatible_errors():
    from tensor_regression_amd.convolutional_spectral_tensor_regression import CP_linear_regression
    with pytest.raises(ValueError, match="odd"):
        CP_linear_regression((50, 4), (50, 2), temporal_window=6)
    with pytest.raises(ValueError, match="2-D"):
        CP_linear_regression((50, 4), (50,), temporal_window=5)
    with pytest.raises(NotImplementedError):
        CP_linear_regression((50, 4), (50, 2), temporal_window=5, dtype=torch.float64)
    mod = CP_linear_regression((50, 4), (50, 2), temporal_window=5)
    X, y = torch.zeros(50, 4), torch.zeros(50, 2)
    with pytest.raises(TypeError):  # lambda_L2[0] on a float, as in the reference
        mod.fit_Adam(X, y, lambda_L2=0.01, Adam_kwargs={'lr': 0.01})
    with pytest.raises(TypeError, match="must be a mapping"):
        mod.fit_Adam(X, y, lambda_L2=[0.01] * 3, Adam_kwargs=None)
    with pytest.raises(NotImplementedError):
        mod.fit_Adam(X, y, lambda_L2=[0.01] * 3, Adam_kwargs={'lr': 0.01}, process_group=object())


def test_l2_penalty_and_torch_helpers():
    from tensor_regression_amd import convolutional_spectral_tensor_regression as C
    g = torch.Generator().manual_seed(0)
    A, B = torch.randn(5, 3, generator=g), torch.randn(4, 3, generator=g)
    want = 0.5 * A.norm() + 2.0 * B.norm()
    assert torch.allclose(C.L2_penalty([A, B], [0.5, 2.0]), want)
    X = torch.randn(20, 3, generator=g)
    K = torch.randn(5, 2, 2, generator=g)
    z = C.conv(X, K)
    assert z.shape == (16, 3, 2, 2)
    assert torch.allclose(z[4, 1, 1, 0], (X[4:9, 1] * K[:, 1, 0]).sum(), atol=1e-5)
    assert torch.equal(C.complex_magnitude(z[..., :1]), z[..., 0])
    assert torch.allclose(C.complex_magnitude(z), z.pow(2).sum(-1).sqrt())


def test_conv_abi_rejects_bad_arguments_without_gpu():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    assert lib.tr_abi_version() == 9 and _lib.TR_ABI_VERSION == 9
    h = ctypes.c_void_p()
    nn = (ctypes.c_int32 * 3)(0, 0, 0)

    def create(W=7, D=4, N=2, Rn=1, Rs=1, C=2, T=100, out=ctypes.byref(h)):
        return lib.tr_plan_create_conv(out, 0, W, D, N, Rn, Rs, C, T, nn, 50.0, 1.0)

    for kw, word in [(dict(W=6), b"odd"), (dict(W=0), b"window"), (dict(Rn=0, Rs=0), b"rank"),
                     (dict(Rn=17, Rs=16), b"rank"), (dict(C=5), b"n_complex"), (dict(N=65), b"n_out"),
                     (dict(out=None), b"NULL")]:
        assert create(**kw) == -1, kw
        assert word in lib.tr_last_error(), (kw, lib.tr_last_error())
    # beyond the kernel's envelope: unsupported, with the reason
    assert create(W=259, T=300) == -2 and b"W <= 257" in lib.tr_last_error()
    assert create(Rn=4, Rs=16, C=4) == -2 and b"K <= 64" in lib.tr_last_error()
    lam = (ctypes.c_float * 3)(0.1, 0.2, 0.3)
    assert lib.tr_plan_set_l2_weights(None, lam, 3) == -1
    if not torch.cuda.is_available():
        assert create() > 0 and lib.tr_last_error()  # a well-formed plan needs a device
