"""CPU-side checks of the hierarchical multinomial module (multinomial_tensor_regression_hierarchical):
the fixtures against the test-local torch restatement (tests/hier_ref.py, bitwise in fp32), the
constructor's RNG draws, the reference's crash quirks (all raised before any device work),
`group_lr` validation, the helpers, and the C entry of the grouped update step."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import hier_ref

GOLDEN = hier_ref.GOLDEN


def _module():
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    return H


def _tiny(ndim=3, **kw):
    H = _module()
    shape = {2: (6, 4), 3: (6, 4, 3), 4: (6, 4, 3, 2)}[ndim]
    X = np.arange(np.prod(shape), dtype=np.float32).reshape(shape) / 10
    y = np.arange(6) % 2
    torch.manual_seed(0)
    return H.CP_logistic_regression(X, y, rank=2, **kw)


def test_module_surface_and_export():
    import tensor_regression_amd
    H = _module()
    assert tensor_regression_amd.multinomial_tensor_regression_hierarchical is H
    for name in ("squeeze_integers", "confusion_matrix", "idx_to_oneHot", "make_BcpInit", "non_neg_fn", "model",
                 "L2_penalty", "CP_logistic_regression"):
        assert hasattr(H, name), name
    import inspect
    C = H.CP_logistic_regression
    assert list(inspect.signature(C.__init__).parameters) == [
        "self", "X", "y", "rank", "non_negative", "weights", "Bcp_init", "Bcp_init_scale", "device",
        "softplus_kwargs"]
    assert list(inspect.signature(C.fit).parameters) == [
        "self", "lambda_L2", "max_iter", "tol", "patience", "verbose", "running_loss_logging_interval",
        "LBFGS_kwargs"]
    assert list(inspect.signature(C.fit_Adam).parameters) == [
        "self", "lambda_L2", "max_iter", "tol", "patience", "verbose", "Adam_kwargs", "group_lr"]
    assert list(inspect.signature(C.predict).parameters) == ["self", "X", "y_true", "Bcp", "device", "plot_pref"]
    d = {k: v.default for k, v in inspect.signature(C.__init__).parameters.items()}
    assert d["rank"] == 5 and d["non_negative"] is False and d["weights"] is None and d["device"] == "cpu"
    for name in ("return_Bcp_final", "make_confusion_matrix", "detach_Bcp", "get_params", "set_params",
                 "display_params", "plot_outputs"):
        assert callable(getattr(C, name))


@pytest.mark.parametrize("name", hier_ref.ADAM_FIXTURES)
def test_restatement_reproduces_fixture_bitwise(name):
    d = hier_ref.load(name)
    m = d["meta"]
    r0 = hier_ref.loss_grad(d["X_f32"], d["y"], d["Bcp0_list"], d["cp_weights"], m["non_negative"], m["lambda_L2"],
                            m["softplus_kwargs"])
    assert np.array_equal(r0["probs"], d["probs0"])
    assert r0["loss"] == float(d["loss0"])
    for g, w in zip(r0["grads"], d["grads0_list"]):
        assert np.array_equal(g, w)
    r10 = hier_ref.fit_from_fixture(d, max_iter=min(10, m["max_iter"]))
    assert np.array_equal(np.asarray(r10["loss_running"]), d["loss_running_10"])
    for a, b in zip(r10["Bcp"], d["Bcp_10_list"]):
        assert np.array_equal(a, b)
    r = hier_ref.fit_from_fixture(d)
    assert np.array_equal(np.asarray(r["loss_running"]), d["loss_running"])
    assert int(r["converged"]) == int(d["converged"])
    for a, b in zip(r["Bcp"], d["Bcp_final_list"]):
        assert np.array_equal(a, b)
    # the recorded fp32-to-fp64 distance of the reference is this restatement's too
    r64 = hier_ref.fit_from_fixture(d, dtype=torch.float64)
    n = min(len(r["loss_running"]), len(r64["loss_running"]))
    a, b = np.asarray(r["loss_running"][:n]), np.asarray(r64["loss_running"][:n])
    assert np.max(np.abs(a - b) / np.abs(b)) == pytest.approx(float(d["drift_loss"]), rel=1e-6)
    assert hier_ref.normwise_rel(r["Bcp"], r64["Bcp"]) == pytest.approx(float(d["drift_factors"]), rel=1e-6)


def test_fixture_properties():
    """What each fixture is there for."""
    kim = hier_ref.load("hier_kim")
    assert kim["X_f32"].shape == (227, 8, 12) and kim["X_f32"].dtype == np.float32
    assert kim["meta"]["n_classes"] == 4 and kim["meta"]["rank"] == 6 and kim["meta"]["non_negative"] == [True] * 3
    assert kim["meta"]["adam_kwargs"] == {"lr": 0.05, "amsgrad": True} and kim["meta"]["lambda_L2"] == 0.005
    assert np.abs(kim["X_f32"].mean(axis=1)).max() < 1e-6 and len(kim["loss_running"]) == 150
    conv = hier_ref.load("hier_converge")
    assert int(conv["converged"]) == 1
    assert conv["meta"]["patience"] + 2 < len(conv["loss_running"]) < conv["meta"]["max_iter"]
    d4 = hier_ref.load("hier_4d")
    assert len(d4["Bcp0_list"]) == 4
    assert np.array_equal(d4["Bcp_final_list"][3], d4["Bcp0_list"][3])  # the class factor is never stepped
    assert np.abs(d4["grads0_list"][3]).max() > 0  # ... but has a gradient
    assert not np.array_equal(d4["Bcp_final_list"][2], d4["Bcp0_list"][2])
    glr = hier_ref.load("hier_group_lr")
    assert glr["meta"]["group_lr"][2][0] == [0, 0.0]
    assert np.array_equal(glr["Bcp_10_list"][2], glr["Bcp0_list"][2])  # lr 0 for the first stretch
    assert not np.array_equal(glr["Bcp_final_list"][2], glr["Bcp0_list"][2])
    assert not np.allclose(hier_ref.load("hier_cpw")["cp_weights"], 1.0)
    assert hier_ref.load("hier_wd")["meta"]["adam_kwargs"]["weight_decay"] > 0
    for f in os.listdir(GOLDEN):
        if f.startswith("hier_"):
            assert os.path.getsize(os.path.join(GOLDEN, f)) < 256 * 1024, f


def test_constructor_rng_parity_bitwise():
    H = _module()
    d = dict(np.load(os.path.join(GOLDEN, "hier_init_rng.npz")))
    cases = json.loads(str(d["meta"]))["cases"]
    assert len(cases) == 3
    for k, c in enumerate(cases):
        y = np.arange(c["shape"][0]) % c["n_classes"]
        torch.manual_seed(c["seed"])
        m = H.CP_logistic_regression(np.zeros(c["shape"], np.float32), y, rank=c["rank"],
                                     non_negative=c["non_negative"], Bcp_init_scale=c["scale"])
        assert [list(A.shape) for A in m.Bcp] == c["factor_shapes"]
        got = np.concatenate([A.detach().numpy().reshape(-1) for A in m.Bcp])
        assert np.array_equal(got, d[f"Bcp_{k}"])
        assert np.array_equal(torch.rand(4).numpy(), d[f"after_{k}"])  # no draw more, none less
        assert all(A.requires_grad for A in m.Bcp)
        assert m.weights.tolist() == c["weights"] and m.softplus_kwargs == c["softplus_kwargs"]
        assert m.n_classes == c["n_classes"] and m.loss_running == []


def test_constructor_weights_are_component_weights():
    m = _tiny(weights=np.array([0.5, 2.0], dtype=np.float32))
    assert m.weights.tolist() == [0.5, 2.0]
    assert _tiny().weights.tolist() == [1.0, 1.0]


def test_quirk_errors_come_before_device_work(monkeypatch):
    """Every one is raised although the model's device is 'cpu' and no plan can exist."""
    from tensor_regression_amd import _engine
    def no_device(*a, **k):
        raise AssertionError("device work before the reference's own error")
    monkeypatch.setattr(_engine, "compute_device", no_device)
    monkeypatch.setattr(_engine, "Plan", no_device)
    with pytest.raises(TypeError):
        _tiny().fit_Adam(Adam_kwargs=None)
    with pytest.raises(TypeError):
        _tiny().fit_Adam()
    with pytest.raises(TypeError):
        _tiny().fit(LBFGS_kwargs=None)
    with pytest.raises(TypeError):
        _tiny().fit()
    with pytest.raises(KeyError):
        _tiny().fit_Adam(Adam_kwargs={"amsgrad": True})
    with pytest.raises(IndexError):
        _tiny(ndim=2).fit_Adam(Adam_kwargs={"lr": 0.01})
    with pytest.raises(TypeError):  # no `weights` argument on either fit
        _tiny().fit_Adam(Adam_kwargs={"lr": 0.01}, weights=np.ones(2))
    with pytest.raises(TypeError):
        _tiny().fit(LBFGS_kwargs={"lr": 1}, weights=np.ones(2))
    with pytest.raises(TypeError):  # torch.optim.Adam's own check of an unknown keyword
        _tiny().fit_Adam(Adam_kwargs={"lr": 0.01, "bogus": 1})
    for kw in ("process_group", "dtype"):
        with pytest.raises(TypeError):
            _tiny().fit_Adam(Adam_kwargs={"lr": 0.01}, **{kw: None})


def test_quirk_get_params_display_params_plot_outputs(monkeypatch, capsys):
    m = _tiny()
    with pytest.raises(AttributeError, match="bias"):
        m.get_params()
    with pytest.raises(AttributeError, match="bias"):
        m.display_params()
    assert "Bcp:" in capsys.readouterr().out  # everything before the bias line was printed
    params = dict(X=m.X, y=m.y, weights=m.weights, Bcp=m.Bcp, non_negative=m.non_negative,
                  softplus_kwargs=m.softplus_kwargs, rank=2, device="cpu", loss_running=[1.0])
    with pytest.raises(KeyError):
        m.set_params(params)
    m.set_params(dict(params, bias=torch.zeros(1)))
    assert m.loss_running == [1.0] and m.get_params()["bias"].tolist() == [0.0]
    # plot_outputs unpacks four values from predict's two
    import sys
    import types
    from unittest import mock
    mpl = types.ModuleType("matplotlib")
    mpl.pyplot = mock.MagicMock()  # no figure is needed to reach the unpack
    monkeypatch.setitem(sys.modules, "matplotlib", mpl)
    monkeypatch.setitem(sys.modules, "matplotlib.pyplot", mpl.pyplot)
    monkeypatch.setattr(type(m), "predict", lambda self, *a, **k: (np.zeros((6, 2)), np.zeros(6, dtype=np.int64)))
    with pytest.raises(ValueError, match="unpack"):
        m.plot_outputs()


def test_group_lr_validation_before_device_work(monkeypatch):
    from tensor_regression_amd import _engine
    H = _module()
    def no_device(*a, **k):
        raise AssertionError("device work before group_lr was validated")
    monkeypatch.setattr(_engine, "compute_device", no_device)
    bad = [0.01,                                   # not a sequence
           [0.01, 0.01],                           # two entries
           [0.01] * 4,                             # four entries
           [0.01, 0.01, -0.01],                    # negative
           [0.01, 0.01, float("nan")],
           [0.01, 0.01, "0.01"],
           [0.01, 0.01, True],
           [0.01, 0.01, []],                       # empty schedule
           [0.01, 0.01, [(1, 0.01)]],              # does not start at 0
           [0.01, 0.01, [(0, 0.01), (0, 0.02)]],   # starts do not strictly increase
           [0.01, 0.01, [(0, 0.01), (5, 0.02), (3, 0.01)]],
           [0.01, 0.01, [(0, 0.01), (2.5, 0.02)]],  # a fractional iteration
           [0.01, 0.01, [(0, 0.01, 1)]],           # not a pair
           [0.01, 0.01, [(0, -1.0)]],
           {0: 0.01, 1: 0.01, 2: 0.01},
           "abc"]
    for g in bad:
        with pytest.raises(ValueError):
            H.resolve_group_lr(g, 0.01)
        with pytest.raises(ValueError):
            _tiny().fit_Adam(Adam_kwargs={"lr": 0.01}, group_lr=g)
    sched = H.resolve_group_lr([0.5, [(0, 0.0), (30, 0.03), (70, 0.002)], np.float32(0.25)], 0.01)
    assert H.lr_in_force(sched, 0) == [0.5, 0.0, 0.25]
    assert H.lr_in_force(sched, 29) == [0.5, 0.0, 0.25]
    assert H.lr_in_force(sched, 30) == [0.5, 0.03, 0.25]
    assert H.lr_in_force(sched, 69) == [0.5, 0.03, 0.25]
    assert H.lr_in_force(sched, 70) == [0.5, 0.002, 0.25]
    assert H.lr_in_force(sched, 10 ** 6) == [0.5, 0.002, 0.25]
    assert H.lr_in_force(H.resolve_group_lr(None, 0.05), 7) == [0.05] * 3
    # the restatement's schedule is the same rule
    glr = hier_ref.load("hier_group_lr")["meta"]["group_lr"]
    sched = H.resolve_group_lr(glr, 0.03)
    ref = hier_ref.lr_schedule(glr, 0.03)
    for ii in range(100):
        want = [[lr for s, lr in ref[g] if s <= ii][-1] for g in range(3)]
        assert H.lr_in_force(sched, ii) == want


def test_predict_arity_and_confusion_helpers_against_fixture():
    H = _module()
    d = hier_ref.load("hier_lbfgs")
    assert int(d["n_predict_outputs"]) == 2  # the reference's predict returns (probs, pred)
    y = d["y"]
    cm = H.confusion_matrix(d["pred_final"], y)
    assert np.array_equal(cm, d["confusion"])
    assert np.sum(np.diag(cm)) / np.sum(cm) == float(d["accuracy"])
    assert np.array_equal(H.confusion_matrix(H.idx_to_oneHot(d["pred_final"], 4), y), d["confusion"])
    assert np.array_equal(np.argmax(d["probs_final"], axis=1), d["pred_final"])
    assert np.array_equal(H.squeeze_integers(np.array([7, 2, 7, 4, 1])), [3, 1, 3, 2, 0])
    # make_confusion_matrix with given predictions needs no device
    m = H.CP_logistic_regression(d["X_f32"], y, rank=3, Bcp_init=[torch.tensor(a) for a in d["Bcp_final_list"]])
    cm2, acc2 = m.make_confusion_matrix(prob_or_pred="pred", pred=d["pred_final"])
    assert np.array_equal(cm2, d["confusion"]) and acc2 == float(d["accuracy"])
    assert [a.shape for a in m.detach_Bcp()] == [(6, 3), (5, 3), (4, 3)]
    A = [torch.tensor(a) for a in d["Bcp0_list"]]
    assert torch.equal(H.L2_penalty(A), hier_ref.l2_penalty(A))


def test_abi_exports_grouped_step_and_rejects_bad_arguments_without_gpu():
    from tensor_regression_amd import _lib
    lib = _lib.load()
    assert "tr_adam_step_groups" in _lib.SIGNATURES and hasattr(lib, "tr_adam_step_groups")
    lr = (ctypes.c_double * 3)(0.01, 0.01, 0.01)
    assert lib.tr_adam_step_groups(None, None, None, None, None, None, 0.0, lr, 3, 7, 0.9, 0.999, 1e-8, 0.0, 0, 1,
                                   None, 0, 0, 0, 0.0, None, None) == -1
    assert b"NULL" in lib.tr_last_error()


def test_resident_envelope_admits_the_notebook_shape_without_gpu():
    """The LDS carve is host arithmetic: (227, 8, 12), C 4, R 6 fits one CU's 160 KiB; C or R past 16 never."""
    from tensor_regression_amd import _lib
    lib = _lib.load()
    for s in ("tr_mnl_resident_max_rows", "tr_plan_set_resident", "tr_fit_adam_resident"):
        assert s in _lib.SIGNATURES and hasattr(lib, s)
    nmax = lib.tr_mnl_resident_max_rows(8, 12, 4, 6)
    assert 227 <= nmax
    # X at the odd pitch 97, Z at pitch 5 and the labels grow with N: 103 words a sample; everything
    # else (B, G and its split partials, seven parameter-sized arrays) is under 4096 words here
    words = 160 * 1024 // 4
    assert (words - 4096) // 103 <= nmax <= words // 103
    assert lib.tr_mnl_resident_max_rows(8, 12, 17, 6) == 0 and lib.tr_mnl_resident_max_rows(8, 12, 4, 17) == 0
    assert lib.tr_mnl_resident_max_rows(0, 12, 4, 6) == 0
    assert lib.tr_plan_set_resident(None, 1) == -1
    assert lib.tr_fit_adam_resident(None, None, 1, None, None, None, None, None, None, 0.0, None, 0.9, 0.999, 1e-8,
                                    0.0, 0, 1, 1, None, 0, 0, 0, 0.0, None, None) == -1
