"""The table pair that the many-model routes share (_engine.table_buffers), across routes and sizes in
one process: a resident fit of 2 models, a scoring call on those 2, a shared-X linear fit of 5 models
(whose table is larger: the pair grows), then the resident fit again in the pair grown for the linear
route.  Rows of three different sizes pass through the same two buffers.

The yardstick is each model's own single route, as in the routes' own tests: fit_Adam for a resident
member, score_many on the one model for a scoring entry, and a group of one for a linear member (a
member's bits do not depend on its neighbours: test_gpu_linear_many).  All bit for bit."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
AK = {"lr": 0.01}


def hier_models():
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    out = []
    for seed in (1, 2):
        rng = np.random.default_rng(seed)
        X = rng.standard_normal((12, 3, 4)).astype(np.float32)
        y = np.arange(12) % 3
        B0 = [torch.tensor((rng.random((k, 2)) - 0.5).astype(np.float32), device=DEV) for k in (3, 4, 3)]
        out.append(H.CP_logistic_regression(X, y, rank=2, Bcp_init=B0, device=DEV))
    return out


def linear_models():
    from tensor_regression_amd import CP_linear_regression
    g = torch.Generator().manual_seed(7)
    return [CP_linear_regression((16, 4, 4), rank=2, device=DEV,
                                 Bcp_init=[(torch.randn(4, 2, generator=g) * 0.3).to(DEV) for _ in range(2)])
            for _ in range(5)]


def fit_bits(m):
    return ([np.asarray(m.loss_running).view(np.int64)] + [A.detach().cpu().numpy().view(np.int32) for A in m.Bcp]
            + ([m.bias.detach().cpu().numpy().view(np.int32)] if hasattr(m, "bias") else []))


def same(a, b):
    return len(a) == len(b) and all(x.shape == y.shape and np.array_equal(x, y) for x, y in zip(a, b))


def score_bits(s):
    return [np.float64(s["loss"]).reshape(1).view(np.int64), np.float64(s["acc"]).reshape(1).view(np.int64),
            s["counts"]]


def test_one_table_pair_serves_every_route_in_turn():
    from tensor_regression_amd import _engine
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    from tensor_regression_amd import standard_tensor_regression as S
    g = torch.Generator().manual_seed(3)
    X = torch.randn(16, 4, 4, generator=g).to(DEV)
    y = torch.randn(16, generator=g).to(DEV)
    lams = [0.01 * (1 + j) for j in range(5)]
    hier_kw = dict(lambda_L2=[0.01, 0.02], max_iter=5, tol=0.0, Adam_kwargs=AK)

    hm, report = hier_models(), {}
    H.fit_Adam_many(hm, report=report, **hier_kw)
    assert report["batched"] == [0, 1]
    scores = H.score_many(hm, report=report)
    assert report["batched"] == [0, 1]
    lm = linear_models()
    S.fit_Adam_many(lm, X, y, lambda_L2=lams, max_iter=5, tol=0.0, Adam_kwargs=AK, min_batch=1, report=report)
    assert report["batched"] == [0, 1, 2, 3, 4] and report["groups"] == 1
    pair = _engine.table_buffers(0, 1)[0].data_ptr()
    hm2 = hier_models()
    H.fit_Adam_many(hm2, report=report, **hier_kw)
    assert report["batched"] == [0, 1]
    assert _engine.table_buffers(0, 1)[0].data_ptr() == pair  # the pair grown for the linear table, reused

    for j, (a, b) in enumerate(zip(hm, hm2)):
        assert len(a.loss_running) == 5 and same(fit_bits(a), fit_bits(b)), f"resident member {j}: second fit"
    for j, (alone, lam) in enumerate(zip(hier_models(), hier_kw["lambda_L2"])):
        alone.fit_Adam(lambda_L2=lam, max_iter=5, tol=0.0, Adam_kwargs=AK)
        assert "fit=resident" in alone._plan.describe
        assert same(fit_bits(hm[j]), fit_bits(alone)), f"resident member {j}: alone"
        assert same(score_bits(scores[j]), score_bits(H.score_many([alone])[0])), f"scoring entry {j}: alone"
    for j, (alone, lam) in enumerate(zip(linear_models(), lams)):
        S.fit_Adam_many([alone], X, y, lambda_L2=lam, max_iter=5, tol=0.0, Adam_kwargs=AK, min_batch=1)
        assert len(lm[j].loss_running) == 5 and same(fit_bits(lm[j]), fit_bits(alone)), f"linear member {j}: alone"
