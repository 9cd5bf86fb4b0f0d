"""Scoring the linear sweep on the GPU: standard_tensor_regression.predict_many / score_many and
tr_linear_many_score against the CPU oracle (oracle/cp_oracle.py), the models' own predict and the fit's
tr_linear_many_loss_grad.

Data, seeds and bars are test_gpu_linear_many.py's: randn X and y, factors 0.3 * randn, weights in
0.5..1.5, alternating non_negative, seeds from crc32 of the case; RTOL = 1e-5.  Shapes: SHAPES of that
file, plus

  (1, 8, 4)         one row: the variances are 0 / 0
  (257, 33, 36)     P = 1188: two feature slices, the second with a 4-feature tail
  (37, 4, 3, 8)     three feature modes, ragged rows
  (130, 8, 4, 8)    three feature modes, two forward workgroups
"""
import types

import numpy as np
import pytest
import torch

from golden_util import normwise_rel
from test_gpu_linear_many import DEV, RANKS, RTOL, SHAPES, _seed, build_model, evaluate, make_specs, make_x, same_bits

pytestmark = pytest.mark.gpu

EXTRA = {"row1": (1, 8, 4), "tail1188": (257, 33, 36), "modes3": (37, 4, 3, 8), "modes3b": (130, 8, 4, 8)}


def case_x(name):
    """(X on the device, the same X contiguous on the host, N, shape)."""
    if name in SHAPES:
        Xd, Xh, N = make_x(name)
        return Xd, Xh, N, tuple(Xh.shape)
    shape = EXTRA[name]
    Xh = torch.randn(*shape, generator=torch.Generator().manual_seed(_seed("x", name)))
    return Xh.to(DEV), Xh, shape[0], shape


def case_specs(name, M):
    """make_specs' recipe; for the extra shapes restated with one factor per feature mode."""
    if name in SHAPES:
        return make_specs(name, M)
    shape = EXTRA[name]
    N, dims = shape[0], shape[1:]
    y_shared = torch.randn(N, generator=torch.Generator().manual_seed(_seed("y", name)))
    specs = []
    for j in range(M):
        gj = torch.Generator().manual_seed(_seed("m", name, j, 0))
        R = RANKS[j % 4]
        specs.append(types.SimpleNamespace(
            rank=R, nn=[bool((j + f) % 2) for f in range(1, len(dims) + 1)],
            Bcp0=[torch.randn(d, R, generator=gj) * 0.3 for d in dims], w=torch.rand(R, generator=gj) + 0.5,
            bias=0.25 - 0.1 * j, sp=None if j % 4 else {"beta": 20, "threshold": 2},
            y=(torch.randn(N, generator=gj) if j % 2 else y_shared)))
    return specs


def oracle_yhat(Xh, s, dtype):
    from oracle import cp_oracle
    out = cp_oracle.lin_model(Xh.to(dtype), [A.to(dtype) for A in s.Bcp0], s.w.to(dtype), s.nn,
                              torch.tensor([s.bias], dtype=torch.float32).to(dtype), s.sp)
    return out.detach().reshape(-1).numpy()


def metrics64(yh, y):
    """The three metrics from a float64 y_hat, with the plain formulas."""
    yh, y = np.asarray(yh, np.float64), np.asarray(y, np.float64)
    with np.errstate(all="ignore"):
        return {"loss": np.mean((yh - y) ** 2),
                "var_ratio": (np.sum((yh - yh.mean()) ** 2) / (len(y) - 1)) / (np.sum((y - y.mean()) ** 2) / (len(y) - 1)),
                "r2": 1.0 - np.sum((yh - y) ** 2) / np.sum((y - y.mean()) ** 2)}


def rel(a, b):
    return abs(a - b) / abs(b)


def S():
    from tensor_regression_amd import standard_tensor_regression
    return standard_tensor_regression


def bits_equal(a, b):
    return same_bits([np.asarray(a)], [np.asarray(b)])


def same_scores(a, b):
    return all(np.float64(a[k]).tobytes() == np.float64(b[k]).tobytes() for k in ("loss", "var_ratio", "r2"))


# ---- 1. against the oracle ---------------------------------------------------------------------------

@pytest.mark.parametrize("name,M", [(n, 5) for n in list(SHAPES) + list(EXTRA)]
                         + [("ragged37", 1), ("ragged37", 2), ("plain130", 16)])
def test_predict_and_score_against_the_oracle(name, M):
    """predict_many within RTOL normwise of cp_oracle.lin_model in fp32; loss, var_ratio and 1 - r2 within
    1e-5 relative of the same quantities from the oracle's float64 y_hat.  All grouped (min_batch = 1)."""
    Xd, Xh, N, shape = case_x(name)
    specs = case_specs(name, M)
    models = [build_model(s, shape) for s in specs]
    rep = {}
    yh = S().predict_many(models, Xd, report=rep, min_batch=1)
    assert rep == {"batched": list(range(M)), "alone": [], "groups": 1, "x_passes": 1}
    sc = S().score_many(models, Xd, [s.y for s in specs], report=rep, min_batch=1)
    assert rep == {"batched": list(range(M)), "alone": [], "groups": 1, "x_passes": 1}
    for j, s in enumerate(specs):
        ref32, ref64 = oracle_yhat(Xh, s, torch.float32), oracle_yhat(Xh, s, torch.float64)
        assert yh[j].dtype == np.float32 and yh[j].shape == (N,)
        err = normwise_rel(yh[j], ref32)
        want = metrics64(ref64, s.y.numpy())
        print(f"{name} M={M} member {j} rank {s.rank}: y_hat {err:.3g} (oracle fp32 vs fp64 "
              f"{normwise_rel(ref32, ref64):.3g}), score {sc[j]} vs {want}")
        assert err <= RTOL, (j, err)
        assert set(sc[j]) == {"loss", "var_ratio", "r2"}
        assert rel(sc[j]["loss"], want["loss"]) <= 1e-5, (j, sc[j]["loss"], want["loss"])
        if N == 1:
            assert np.isnan(sc[j]["var_ratio"]) and sc[j]["r2"] == -np.inf == want["r2"]
            continue
        assert rel(sc[j]["var_ratio"], want["var_ratio"]) <= 1e-5, (j, sc[j]["var_ratio"], want["var_ratio"])
        assert rel(1.0 - sc[j]["r2"], 1.0 - want["r2"]) <= 1e-5, (j, sc[j]["r2"], want["r2"])


# ---- 2. the C entry, driven directly -----------------------------------------------------------------

@pytest.mark.parametrize("name", ["ragged37", "ragged257", "c2row"])
def test_entry_bits_against_predict_many_and_the_fit(name):
    """One call of tr_linear_many_score with y, yhat and sums: y_hat carries predict_many's bits, and the
    data loss formed from sums[0] as k_lm_fold forms it, float(sum e^2 * (1 / N)), carries the bits of
    tr_linear_many_loss_grad's data-loss slot for the same members."""
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    Xd, Xh, N, shape = case_x(name)
    I, J = shape[1:]
    M = 5
    specs = make_specs(name, M)
    members, _, _, _ = evaluate(Xd, specs)  # the fit's evaluation: arena, w, y on the device, grad filled
    yhat = torch.zeros(M, N, device=DEV)
    sums = torch.zeros(M, 5, dtype=torch.float64, device=DEV)
    arr, rec = _engine.member_records(_lib.LinearScoreMember, M)
    for j, (r, mb) in enumerate(zip(arr, members)):
        r.params, r.weights, r.y = mb.arena.data_ptr(), mb.w.data_ptr(), mb.y.data_ptr()
        r.yhat, r.sums = yhat[j].data_ptr(), sums[j].data_ptr()
        r.rank, r.softplus_beta, r.softplus_threshold = mb.rank, mb.beta, mb.thr
        r.nonneg[0], r.nonneg[1] = int(mb.nonneg[0]), int(mb.nonneg[1])
    bufs = _engine.LinearScoreBuffers(0, N, (I, J), 1)
    th, td = bufs.tables(0)
    xld = Xd.stride(0) if N > 1 else I * J
    _lib.check(lib.tr_linear_many_score(0, _lib.ptr(Xd), N, xld, 2, bufs.dims, arr, M, _lib.ptr(bufs.ws), bufs.ws_bytes,
                                        _lib.ptr(th), _lib.ptr(td), bufs.table_bytes, _engine.stream_handle(0)),
               "tr_linear_many_score")
    torch.cuda.synchronize()
    models = [build_model(s, shape) for s in specs]
    via = S().predict_many(models, Xd, min_batch=1)
    yhat_h, sums_h = yhat.cpu().numpy(), sums.cpu().numpy()
    for j, mb in enumerate(members):
        assert bits_equal(yhat_h[j], via[j]), j
        n = mb.arena.numel()
        fit_loss = mb.grad[n].cpu().numpy()
        mine = np.float32(sums_h[j, 0] * (1.0 / float(N)))
        print(f"{name} member {j}: data loss {mine!r} vs the fit's {fit_loss!r}")
        assert mine.tobytes() == fit_loss.tobytes(), (j, mine, fit_loss)


# ---- 3. groups, positions and neighbours ---------------------------------------------------------------

def test_nineteen_models_two_groups_and_position_independence():
    name = "plain130"
    Xd, Xh, N, shape = case_x(name)
    specs = make_specs(name, 19)
    models = [build_model(s, shape) for s in specs]
    ys = [s.y for s in specs]
    rep = {}
    yh = S().predict_many(models, Xd, report=rep)
    assert rep == {"batched": list(range(19)), "alone": [], "groups": 2, "x_passes": 2}
    sc = S().score_many(models, Xd, ys, report=rep)
    assert rep == {"batched": list(range(19)), "alone": [], "groups": 2, "x_passes": 2}
    size = max(S().LINEAR_SCORE_MIN_BATCH, 2)
    for j in range(19):
        others = [(j + 7 + k) % 19 for k in range(size - 1)]  # other neighbours than in the big call
        at = j % size                                         # ... and another position
        idx = others[:at] + [j] + others[at:]
        yh2 = S().predict_many([models[i] for i in idx], Xd, report=rep)
        assert rep["batched"] == list(range(size)) and rep["groups"] == 1
        sc2 = S().score_many([models[i] for i in idx], Xd, [ys[i] for i in idx])
        assert bits_equal(yh[j], yh2[at]), j
        assert same_scores(sc[j], sc2[at]), (j, sc[j], sc2[at])
    # the same object twice: the same bits twice
    twice = [models[3], models[5], models[3], models[5], models[3]]
    yh3 = S().predict_many(twice, Xd, report=rep, min_batch=1)
    assert rep["batched"] == [0, 1, 2, 3, 4]
    assert bits_equal(yh3[0], yh3[2]) and bits_equal(yh3[0], yh3[4]) and bits_equal(yh3[1], yh3[3])
    assert bits_equal(yh3[0], yh[3]) and bits_equal(yh3[1], yh[5])
    sc3 = S().score_many(twice, Xd, ys[3], min_batch=1)
    assert same_scores(sc3[0], sc3[2]) and same_scores(sc3[0], sc3[4]) and same_scores(sc3[1], sc3[3])


# ---- 4. a target far from zero ---------------------------------------------------------------------------

def test_large_mean_target_keeps_the_variances():
    """y with mean 1e4 and unit variance: var_ratio and r2 within 1e-6 relative of float64 arithmetic on
    the same fp32 y_hat and y (the sums are shifted by y[0], so nothing cancels)."""
    name = "ragged257"
    Xd, Xh, N, shape = case_x(name)
    specs = make_specs(name, 5)
    models = [build_model(s, shape) for s in specs]
    y = (1e4 + torch.randn(N, generator=torch.Generator().manual_seed(_seed("big", name)))).float()
    yh = S().predict_many(models, Xd, min_batch=1)
    sc = S().score_many(models, Xd, y, min_batch=1)
    for j in range(5):
        want = metrics64(yh[j], y.numpy())
        print(f"member {j}: {sc[j]} vs {want}")
        assert rel(sc[j]["var_ratio"], want["var_ratio"]) <= 1e-6, (j, sc[j], want)
        assert rel(sc[j]["r2"], want["r2"]) <= 1e-6, (j, sc[j], want)


# ---- 5. routing on the device ---------------------------------------------------------------------------

def _alone_equals_predict(models, X, y, rep_alone, **kw):
    rep = {}
    yh = S().predict_many(models, X, report=rep, **kw)
    assert rep["alone"] == rep_alone, rep
    sc = S().score_many(models, X, y, report=rep, **kw)
    assert rep["alone"] == rep_alone, rep
    for j in rep_alone:
        own = models[j].predict(X)
        assert bits_equal(yh[j], own), j
        assert same_scores(sc[j], S()._host_metrics(own, y)), j
    return yh, sc


def test_routing_on_the_device(monkeypatch):
    from tensor_regression_amd import CP_linear_regression
    name = "plain130"
    Xd, Xh, N, shape = case_x(name)
    specs = make_specs(name, 4)
    models = [build_model(s, shape) for s in specs]
    y = specs[0].y
    # a rank-33 model goes alone, its neighbours stay grouped
    g = torch.Generator().manual_seed(_seed("r33"))
    big = CP_linear_regression(shape, rank=33, device=DEV, bias_init=0.1,
                               Bcp_init=[(torch.randn(d, 33, generator=g) * 0.3).to(DEV) for d in shape[1:]])
    mixed = [models[0], big, models[1], models[2]]
    rep = {}
    yh, sc = _alone_equals_predict(mixed, Xd, y, [1], min_batch=1)
    S().predict_many(mixed, Xd, report=rep, min_batch=1)
    assert rep == {"batched": [0, 2, 3], "alone": [1], "groups": 1, "x_passes": 1}
    # float64 models over a float64 X go alone
    m64 = [CP_linear_regression(shape, dtype=torch.float64, rank=s.rank, non_negative=list(s.nn), weights=s.w.numpy(),
                                device=DEV, Bcp_init=[b.double().to(DEV) for b in s.Bcp0], bias_init=s.bias,
                                softplus_kwargs=s.sp) for s in specs[:2]]
    _alone_equals_predict(m64, Xd.double(), y, [0, 1], min_batch=1)
    # P = 6 is no multiple of 4
    X6 = torch.randn(20, 2, 3, generator=torch.Generator().manual_seed(_seed("x6"))).to(DEV)
    m6 = [CP_linear_regression((20, 2, 3), rank=2, device=DEV,
                               Bcp_init=[(torch.randn(d, 2, generator=g) * 0.3).to(DEV) for d in (2, 3)])
          for _ in range(2)]
    _alone_equals_predict(m6, X6, torch.randn(20, generator=g), [0, 1], min_batch=1)
    # a group below min_batch
    _alone_equals_predict(models, Xd, y, [0, 1, 2, 3], min_batch=5)
    # a Bcp override is honoured, and the caller's list is converted in place as predict does
    over = [(specs[1].Bcp0[0] * 0.5).numpy().copy(), (specs[1].Bcp0[1] + 0.1).numpy().copy()]
    over_own = [a.copy() for a in over]
    out = S().predict_many(models, Xd, Bcp=[None, over, None, None], report=rep, min_batch=1)
    assert rep["batched"] == [0, 1, 2, 3]
    assert all(isinstance(a, torch.Tensor) and a.dtype == torch.float32 and a.device.type == "cuda" for a in over)
    own = models[1].predict(Xd, Bcp=over_own)
    assert normwise_rel(out[1], own) <= RTOL and not bits_equal(out[1], yh_of(models[1], Xd))
    assert bits_equal(out[0], S().predict_many(models, Xd, min_batch=1)[0])
    # the switch sends everything alone
    monkeypatch.setenv("TR_LINEAR_MANY", "0")
    _alone_equals_predict(models, Xd, y, [0, 1, 2, 3], min_batch=1)


def yh_of(model, X):
    return model.predict(X)


# ---- 6. after a fit, on views of one buffer ----------------------------------------------------------------

def test_score_after_fit_on_views_of_one_buffer(monkeypatch):
    from oracle import cp_oracle
    from tensor_regression_amd import _engine
    name = "plain130"
    (N, I, J), _ = SHAPES[name]
    n_all = N + 70
    g = torch.Generator().manual_seed(_seed("x", "views"))
    Xh = torch.randn(n_all, I, J, generator=g)
    yh_all = torch.randn(n_all, generator=g)
    Xd = Xh.to(DEV)
    specs = make_specs(name, 4, y_list=False)
    models = [build_model(s, (N, I, J)) for s in specs]
    S().fit_Adam_many(models, Xd[:N], yh_all[:N], lambda_L2=[s.lam for s in specs], max_iter=20, tol=0.0,
                      Adam_kwargs=[s.ak for s in specs], min_batch=1)
    seen = []
    real = _engine.run_linear_score

    def spy(dev, X, members, want, trace=None):
        seen.append((X.data_ptr(), tuple(X.shape), X.stride(0)))
        return real(dev, X, members, want, trace)
    monkeypatch.setattr(_engine, "run_linear_score", spy)
    rep = {}
    held = S().score_many(models, Xd[N:], yh_all[N:], report=rep, min_batch=1)
    train = S().score_many(models, Xd[:N], yh_all[:N], report=rep, min_batch=1)
    assert rep == {"batched": [0, 1, 2, 3], "alone": [], "groups": 1, "x_passes": 1}
    assert seen == [(Xd.data_ptr() + 4 * N * I * J, (n_all - N, I, J), I * J), (Xd.data_ptr(), (N, I, J), I * J)]
    for j, (s, m) in enumerate(zip(specs, models)):
        fitted = [A.detach().cpu().double() for A in m.Bcp]
        bias = m.bias.detach().cpu().double()
        for part, Xp, yp in ((train, Xh[:N], yh_all[:N]), (held, Xh[N:], yh_all[N:])):
            ref = cp_oracle.lin_model(Xp.double(), fitted, s.w.double(), s.nn, bias, s.sp).numpy()
            want = metrics64(ref, yp.numpy())
            print(f"member {j}: {part[j]} vs {want}")
            assert rel(part[j]["loss"], want["loss"]) <= 1e-5, (j, part[j], want)
