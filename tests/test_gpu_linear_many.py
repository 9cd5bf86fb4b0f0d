"""The shared-X linear sweep on the GPU: standard_tensor_regression.fit_Adam_many and the
tr_linear_many_* entries against the CPU oracle (oracle/cp_oracle.py), the golden fixtures and the
single-model route.

Data as in test_linear_sweep_vs_oracle: randn X and y, factors 0.3 * randn, weights in 0.5..1.5,
alternating non_negative, seeds from crc32 of the case.  Bars: RTOL = 1e-5 and the bias-gradient bar
of tests/test_gpu_parity.py::test_linear_golden, unchanged.  Shapes (N, I, J), each the smallest at
which a kernel of the sweep takes another path:

  (3, 8, 4)       fewer rows than one 16-row tile
  (37, 8, 12)     ragged row tile; P = 96 is no multiple of the 32-feature step (zero-filled tail)
  (130, 16, 16)   plain; more than one forward workgroup of 128 rows, ragged gradient chunk
  (257, 24, 20)   ragged tile at a larger P; two epilogue workgroups, two gradient chunks
  (48, 256, 128)  config 2's row: the 512-feature fold inside a slice, 32 feature slices, 128 gradient waves
  (292, 9, 12)    util.windowed_view of a (300, 12) series: row stride 12 < P = 108
  (130, 16, 16)+4 rows cut from a buffer with row stride P + 4
"""
import types
import zlib

import numpy as np
import pytest
import torch

from golden_util import load, normwise_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5
RANKS = (1, 3, 8, 32)
SHAPES = {
    "rows3": ((3, 8, 4), "plain"),
    "ragged37": ((37, 8, 12), "plain"),
    "plain130": ((130, 16, 16), "plain"),
    "ragged257": ((257, 24, 20), "plain"),
    "c2row": ((48, 256, 128), "plain"),
    "windowed": ((292, 9, 12), "windowed"),
    "padded": ((130, 16, 16), "padded"),
}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 2**31


def make_x(name):
    """(X on the device in the case's layout, the same X contiguous on the host, N)."""
    shape, kind = SHAPES[name]
    N, I, J = shape
    P = I * J
    g = torch.Generator().manual_seed(_seed("x", name))
    if kind == "windowed":
        from tensor_regression_amd.util import windowed_view
        series = torch.randn(N + I - 1, J, generator=g)
        Xd, _ = windowed_view(series.to(DEV), torch.zeros(N + I - 1, device=DEV), (0, I))
        Xh, _ = windowed_view(series, torch.zeros(N + I - 1), (0, I))
        assert tuple(Xd.shape) == shape and Xd.stride(0) == J < P
        return Xd, Xh.contiguous(), N
    if kind == "padded":
        base = torch.randn(N * (P + 4), generator=g)
        Xh = torch.as_strided(base, shape, (P + 4, J, 1))
        Xd = torch.as_strided(base.to(DEV), shape, (P + 4, J, 1))
        return Xd, Xh.contiguous(), N
    Xh = torch.randn(*shape, generator=g)
    return Xh.to(DEV), Xh, N


def make_specs(name, M, y_list=True, vary=0):
    """M member descriptions over the case's shape: ranks, lambda, lr, amsgrad, weight decay, softplus
    settings and targets mixed.  `vary` reseeds the initial factors and shifts lambda (test 4)."""
    (N, I, J), _ = SHAPES[name]
    g = torch.Generator().manual_seed(_seed("y", name))
    y_shared = torch.randn(N, generator=g)
    specs = []
    for j in range(M):
        gj = torch.Generator().manual_seed(_seed("m", name, j, vary))
        R = RANKS[j % 4]
        ak = {"lr": 0.01 * (1 + j % 3)}
        if j % 2:
            ak["amsgrad"] = True
        if j % 3 == 2:
            ak.update(weight_decay=0.01, betas=(0.8, 0.99), eps=1e-6)
        specs.append(types.SimpleNamespace(
            rank=R, nn=[bool(j % 2), bool((j + 1) % 2)],
            Bcp0=[torch.randn(I, R, generator=gj) * 0.3, torch.randn(J, R, generator=gj) * 0.3],
            w=torch.rand(R, generator=gj) + 0.5, bias=0.25 - 0.1 * j,
            lam=0.01 * (1 + j) + 0.003 * vary, ak=ak,
            sp=None if j % 4 else {"beta": 20, "threshold": 2},
            y=(torch.randn(N, generator=gj) if (y_list and j % 2) else y_shared)))
    return specs


def build_model(s, shape):
    from tensor_regression_amd import CP_linear_regression
    return CP_linear_regression(shape, rank=s.rank, non_negative=list(s.nn), weights=s.w.numpy(), device=DEV,
                                Bcp_init=[b.clone().to(DEV) for b in s.Bcp0], bias_init=s.bias,
                                softplus_kwargs=s.sp)


def oracle_fit(Xh, s, max_iter, tol=0.0, patience=10, dtype=torch.float32):
    from oracle import cp_oracle
    return cp_oracle.fit_adam_linear(Xh, s.y, s.Bcp0, np.array([s.bias], np.float32), s.w, s.nn, s.lam, max_iter,
                                     tol, patience, s.ak, s.sp, dtype=dtype)


def bits(model):
    return [A.detach().cpu().numpy().copy() for A in model.Bcp] + [model.bias.detach().cpu().numpy().copy(),
                                                                    np.array(model.loss_running)]


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- the C entries, driven directly (tests 1 and 6) ---------------------------------------------------

def evaluate(Xd, specs):
    """tr_linear_many_loss_grad on the group: returns the members (with arena, grad, ...) and buffers."""
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    N, I, J = (int(d) for d in Xd.shape)
    members = []
    for s in specs:
        n = (I + J) * s.rank + 1
        _, beta, thr = _engine.nonlin_key(s.nn, s.sp, 2)
        members.append(types.SimpleNamespace(
            arena=torch.cat([s.Bcp0[0].reshape(-1), s.Bcp0[1].reshape(-1), torch.tensor([s.bias])]).to(DEV),
            w=s.w.to(DEV), y=s.y.to(DEV), grad=torch.zeros(n + 2, device=DEV), m=torch.zeros(n, device=DEV),
            v=torch.zeros(n, device=DEV), vmax=torch.zeros(n, device=DEV) if s.ak.get("amsgrad") else None,
            hist=torch.zeros(8, dtype=torch.float64, device=DEV), stop=torch.zeros(1, dtype=torch.int32, device=DEV),
            rank=s.rank, nonneg=s.nn, beta=beta, thr=thr, lambda_L2=s.lam, hp=_engine.adam_hparams(s.ak),
            patience=10, tol=0.0, hist_base=0))
    bufs = _engine.LinearManyBuffers(0, N, I, J, len(members))
    arr, rec = _engine.linear_member_array(members)
    xld = Xd.stride(0) if N > 1 else I * J
    _lib.check(lib.tr_linear_many_loss_grad(0, _lib.ptr(Xd), N, xld, I, J, arr, len(members), _lib.ptr(bufs.ws),
                                            bufs.ws_bytes, _lib.ptr(bufs.table_host), _lib.ptr(bufs.table_dev),
                                            bufs.table_bytes, _engine.stream_handle(0)), "tr_linear_many_loss_grad")
    torch.cuda.synchronize()
    return members, bufs, arr, rec


@pytest.mark.parametrize("name,M", [(n, 5) for n in SHAPES] + [("ragged37", 1), ("ragged37", 2), ("plain130", 16)])
def test_one_evaluation(name, M):
    """tr_linear_many_loss_grad per member against cp_oracle.linear_loss_grad: data loss and total loss
    within 1e-5 relative, every factor gradient within 1e-5 normwise, the bias gradient under
    test_linear_golden's bar.  The L2 term is added by the member's own plan (tr_finalize_grad), which
    also reads the arena in tr_loss_grad's layout."""
    from oracle import cp_oracle
    Xd, Xh, N = make_x(name)
    specs = make_specs(name, M)
    members, _, _, _ = evaluate(Xd, specs)
    for j, (s, mb) in enumerate(zip(specs, members)):
        ref = cp_oracle.linear_loss_grad(Xh, s.y, s.Bcp0, torch.tensor([s.bias]), s.w, s.nn, s.lam, s.sp)
        model = build_model(s, Xh.shape)
        plan = model._get_plan(Xd, N)
        n = plan.num_params
        assert mb.grad.numel() == plan.num_grads and mb.grad[n + 1].item() == 0.0
        gtot, loss = torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
        plan.finalize_grad(mb.arena, mb.grad, s.lam, gtot, loss)
        dl = mb.grad[n].item()
        print(f"{name} M={M} member {j} rank {s.rank}: data loss {dl:.8g} vs {ref['data_loss']:.8g}, "
              f"grads {[normwise_rel(a.cpu().numpy(), b) for a, b in zip(plan.factor_views(gtot), ref['grads'])]}")
        assert abs(dl - ref["data_loss"]) <= RTOL * abs(ref["data_loss"]), (j, dl, ref["data_loss"])
        assert abs(loss.item() - ref["loss"]) <= RTOL * abs(ref["loss"]), (j, loss.item(), ref["loss"])
        for a, b in zip(plan.factor_views(gtot), ref["grads"]):
            assert normwise_rel(a.cpu().numpy(), b) <= RTOL, (j, normwise_rel(a.cpu().numpy(), b))
        np.testing.assert_allclose(gtot[-1:].cpu().numpy(), ref["bias_grad"], rtol=1e-4,
                                   atol=1e-6 * max(1.0, abs(float(ref["bias_grad"][0]))))


@pytest.mark.parametrize("j", [0, 1, 2])
def test_update_equivalence(j):
    """On one member's gradient arena, tr_linear_many_step and the plan's adam_step (k_update) give
    bitwise equal parameters, m, v, vmax and loss record.  Members 0, 1, 2: Adam, AMSGrad, AMSGrad with
    weight decay and other betas."""
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    name = "ragged37"
    Xd, Xh, N = make_x(name)
    specs = make_specs(name, 3)
    members, bufs, arr, rec = evaluate(Xd, specs)
    mb, s = members[j], specs[j]
    plan = build_model(s, Xh.shape)._get_plan(Xd, N)
    a2, m2, v2 = mb.arena.clone(), torch.zeros_like(mb.m), torch.zeros_like(mb.v)
    x2 = torch.zeros_like(mb.vmax) if mb.vmax is not None else None
    h2, stop2 = torch.zeros_like(mb.hist), torch.zeros_like(mb.stop)
    step, it = 3, 2  # a step whose bias corrections are not those of step 1
    plan.adam_step(a2, mb.grad, m2, v2, x2, s.lam, mb.hp, step, h2, 0, it, 10, 0.0, stop2)
    rec["n_iters"], rec["step"], rec["iter"] = 1, step, it
    I, J = int(Xd.shape[1]), int(Xd.shape[2])
    _lib.check(lib.tr_linear_many_step(0, I, J, arr, len(members), _lib.ptr(bufs.table_host),
                                       _lib.ptr(bufs.table_dev), bufs.table_bytes, _engine.stream_handle(0)),
               "tr_linear_many_step")
    torch.cuda.synchronize()
    pairs = [(mb.arena, a2), (mb.m, m2), (mb.v, v2), (mb.hist, h2)] + ([(mb.vmax, x2)] if x2 is not None else [])
    for got, want in pairs:
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8))
    init = torch.cat([s.Bcp0[0].reshape(-1), s.Bcp0[1].reshape(-1), torch.tensor([s.bias])])
    assert mb.hist[it].item() != 0.0 and not torch.equal(mb.arena.cpu(), init)  # a step was taken


# ---- fit_Adam_many against the oracle and the goldens (test 2) ----------------------------------------

def assert_fit_matches(model, s, Xh, max_iter, tol=0.0, patience=10):
    from test_gpu_parity import _assert_as_accurate_as_reference
    r32 = oracle_fit(Xh, s, max_iter, tol, patience)
    assert len(model.loss_running) == len(r32["loss_running"])
    np.testing.assert_allclose(model.loss_running, r32["loss_running"], rtol=RTOL)
    r64 = oracle_fit(Xh, s, max_iter, tol, patience, dtype=torch.float64)
    _assert_as_accurate_as_reference(model.Bcp, r32["Bcp"], r64["Bcp"])


def run_many(Xd, specs, shape, **kw):
    from tensor_regression_amd.standard_tensor_regression import fit_Adam_many
    models = [build_model(s, shape) for s in specs]
    ys = [s.y.to(DEV) for s in specs]
    y = ys[0] if all(s.y is specs[0].y for s in specs) else ys
    report = {}
    kw.setdefault("max_iter", 10)
    kw.setdefault("tol", 0.0)
    conv = fit_Adam_many(models, Xd, y, lambda_L2=[s.lam for s in specs], Adam_kwargs=[s.ak for s in specs],
                         min_batch=1, report=report, **kw)
    return models, conv, report


@pytest.mark.parametrize("name,M", [(n, 5) for n in SHAPES] + [("ragged37", 1), ("ragged37", 2), ("plain130", 16),
                                                              ("ragged37", 17)])
def test_ten_iterations(name, M):
    Xd, Xh, N = make_x(name)
    specs = make_specs(name, M, y_list=(M != 2))  # M = 2: one shared y
    models, conv, report = run_many(Xd, specs, Xh.shape)
    assert conv == [False] * M
    assert report["batched"] == list(range(M)) and report["alone"] == [] and report["groups"] == -(-M // 16)
    assert report["x_passes"] == 2 * 10 * report["groups"]  # two passes per iteration and group, whatever M
    for model, s in zip(models, specs):
        assert model._plan is None
        assert_fit_matches(model, s, Xh, 10)


@pytest.mark.parametrize("gname", ["lin_fused_shape", "lin_cfg1_amsgrad", "lin_nonneg_amsgrad_wd"])
def test_golden_replayed_as_member_0(gname):
    """Member 0 is a golden fixture on its own X and y, against its loss_running_10 and Bcp_10; the
    other members vary lambda and rank on the same data."""
    from test_gpu_parity import _assert_factors, _lin_model_from
    from tensor_regression_amd.standard_tensor_regression import fit_Adam_many
    d = load(gname)
    m = d["meta"]
    X, y = d["X"].to(DEV), torch.tensor(d["y"], device=DEV)
    N, I, J = d["X"].shape
    models = [_lin_model_from(d)]
    lams, aks = [m["lambda_L2"]], [m["adam_kwargs"]]
    others = []
    for j in range(1, 4):
        g = torch.Generator().manual_seed(_seed(gname, j))
        s = types.SimpleNamespace(rank=RANKS[j], nn=[False, bool(j % 2)], w=torch.rand(RANKS[j], generator=g) + 0.5,
                                  Bcp0=[torch.randn(I, RANKS[j], generator=g) * 0.3,
                                        torch.randn(J, RANKS[j], generator=g) * 0.3],
                                  bias=0.1 * j, lam=0.02 * j, ak={"lr": 0.01}, sp=None, y=torch.tensor(d["y"]))
        others.append(s)
        models.append(build_model(s, d["X"].shape))
        lams.append(s.lam)
        aks.append(s.ak)
    report = {}
    fit_Adam_many(models, X, y, lambda_L2=lams, max_iter=min(10, m["max_iter"]), tol=m["tol"],
                  patience=m["patience"], Adam_kwargs=aks, min_batch=1, report=report)
    assert report["batched"] == [0, 1, 2, 3]
    np.testing.assert_allclose(models[0].loss_running, d["loss_running_10"], rtol=RTOL)
    _assert_factors(models[0].Bcp, d["Bcp_10_list"])
    for model, s in zip(models[1:], others):
        assert_fit_matches(model, s, d["X"], 10, m["tol"], m["patience"])


# ---- stops (test 3) ---------------------------------------------------------------------------------

def test_stops_and_second_fit():
    from test_gpu_parity import _assert_factors, _lin_model_from
    from tensor_regression_amd.standard_tensor_regression import fit_Adam_many
    d = load("lin_converge")
    m = d["meta"]
    X, y = d["X"].to(DEV), torch.tensor(d["y"], device=DEV)
    N, I, J = d["X"].shape
    specs = make_specs("rows3", 4, y_list=False)  # only ranks and settings are taken from these
    others = []
    for j, s in enumerate(specs):
        g = torch.Generator().manual_seed(_seed("stops", j))
        s.Bcp0 = [torch.randn(I, s.rank, generator=g) * 0.3, torch.randn(J, s.rank, generator=g) * 0.3]
        s.y = torch.tensor(d["y"])
        others.append(s)
    models = [_lin_model_from(d)] + [build_model(s, d["X"].shape) for s in others]
    patience = [m["patience"], 10, 3, 10, 10]
    tols = [m["tol"], 0.0, 1e30, 0.0, 0.0]
    iters = [m["max_iter"], 12, 40, 70, 5]  # 70: past one chunk of 64 iterations
    lams = [m["lambda_L2"]] + [s.lam for s in others]
    aks = [m["adam_kwargs"]] + [s.ak for s in others]
    conv = fit_Adam_many(models, X, y, lambda_L2=lams, max_iter=iters, tol=tols, patience=patience,
                         Adam_kwargs=aks, min_batch=1)
    assert int(conv[0]) == int(d["converged"]) and len(models[0].loss_running) == len(d["loss_running"])
    np.testing.assert_allclose(models[0].loss_running, d["loss_running"], rtol=RTOL)
    # every member's length: its own max_iter, or its stop
    assert [len(mm.loss_running) for mm in models[1:]] == [12, 3 + 2, 70, 5]
    assert conv[1:] == [False, True, False, False]
    # the tol = 1e30 member stops at the first plateau test, loop index ii = patience + 1 (the
    # reference's `ii > patience`): patience + 2 iterations, the length its own fit_Adam gives.  Its
    # factors are then those of a fit of exactly that length, bit for bit, while the others went on.
    lone = build_model(others[1], d["X"].shape)
    assert lone.fit_Adam(X, y, lambda_L2=lams[2], max_iter=40, tol=1e30, patience=3, Adam_kwargs=aks[2])
    assert len(lone.loss_running) == len(models[2].loss_running) == 5
    np.testing.assert_allclose(models[2].loss_running, lone.loss_running, rtol=RTOL)
    many5 = build_model(others[1], d["X"].shape)
    fit_Adam_many([many5], X, y, lambda_L2=lams[2], max_iter=5, tol=0.0, patience=3, Adam_kwargs=aks[2], min_batch=1)
    assert same_bits(bits(models[2]), bits(many5))
    for k in (1, 3, 4):
        assert_fit_matches(models[k], others[k - 1], d["X"], iters[k])
    # a second call continues loss_running (the plateau test reads the earlier losses)
    fit_Adam_many(models[:2], X, y, lambda_L2=lams[:2], max_iter=[m["second_fit"], 4], tol=[m["tol"], 0.0],
                  patience=[m["patience"], 10], Adam_kwargs=aks[:2], min_batch=1)
    assert len(models[0].loss_running) == len(d["loss_running2"])
    np.testing.assert_allclose(models[0].loss_running, d["loss_running2"], rtol=RTOL)
    _assert_factors(models[0].Bcp, d["Bcp_final2_list"])
    assert len(models[1].loss_running) == 16


# ---- independence and reproducibility (test 4) --------------------------------------------------------

@pytest.mark.parametrize("name", ["ragged257", "c2row"])
def test_independence_and_reproducibility(name):
    Xd, Xh, N = make_x(name)
    specs = make_specs(name, 5)
    a, _, _ = run_many(Xd, specs, Xh.shape, max_iter=6)
    b, _, _ = run_many(Xd, specs, Xh.shape, max_iter=6)
    for x, y in zip(a, b):
        assert same_bits(bits(x), bits(y))  # the same group twice
    other = make_specs(name, 5, vary=1)  # other initial factors and lambda for the other four
    other[2] = specs[2]
    c, _, _ = run_many(Xd, other, Xh.shape, max_iter=6)
    assert same_bits(bits(a[2]), bits(c[2]))
    assert not same_bits(bits(a[1]), bits(c[1]))
    moved = [specs[2], specs[0], specs[1], specs[3], specs[4]]  # member 2 at position 0
    e, _, _ = run_many(Xd, moved, Xh.shape, max_iter=6)
    assert same_bits(bits(a[2]), bits(e[0]))


# ---- routing (test 5) ---------------------------------------------------------------------------------

def _alone_twin(s, shape, Xd, max_iter=4):
    twin = build_model(s, shape)
    twin.fit_Adam(Xd, s.y.to(DEV), lambda_L2=s.lam, max_iter=max_iter, tol=0.0, Adam_kwargs=s.ak)
    return twin


def test_routing(monkeypatch):
    from tensor_regression_amd import CP_linear_regression
    from tensor_regression_amd import standard_tensor_regression as S
    name = "ragged37"
    Xd, Xh, N = make_x(name)
    specs = make_specs(name, 3)
    big = make_specs(name, 1)[0]
    g = torch.Generator().manual_seed(_seed("r33"))
    big.rank, big.w = 33, torch.rand(33, generator=g) + 0.5
    big.Bcp0 = [torch.randn(8, 33, generator=g) * 0.3, torch.randn(12, 33, generator=g) * 0.3]
    mixed = specs + [big]
    models, conv, report = run_many(Xd, mixed, Xh.shape, max_iter=4)
    assert report == {"batched": [0, 1, 2], "alone": [3], "groups": 1, "x_passes": 8}
    assert same_bits(bits(models[3]), bits(_alone_twin(big, Xh.shape, Xd)))
    # x_passes does not grow with M inside one group
    _, _, r1 = run_many(Xd, specs[:1], Xh.shape, max_iter=4)
    assert r1["x_passes"] == report["x_passes"] == 8
    # the route switched off, and a default min_batch above the group size: everything alone
    monkeypatch.setenv("TR_LINEAR_MANY", "0")
    off, _, r_off = run_many(Xd, specs, Xh.shape, max_iter=4)
    monkeypatch.delenv("TR_LINEAR_MANY")
    assert r_off == {"batched": [], "alone": [0, 1, 2], "groups": 0, "x_passes": 0}
    monkeypatch.setattr(S, "LINEAR_MANY_MIN_BATCH", 4)
    ms = [build_model(s, Xh.shape) for s in specs]
    r_min = {}
    S.fit_Adam_many(ms, Xd, [s.y.to(DEV) for s in specs], lambda_L2=[s.lam for s in specs], max_iter=4, tol=0.0,
                    Adam_kwargs=[s.ak for s in specs], report=r_min)
    assert r_min == r_off
    for k, s in enumerate(specs):
        twin = bits(_alone_twin(s, Xh.shape, Xd))
        assert same_bits(bits(off[k]), twin) and same_bits(bits(ms[k]), twin)
    # P % 4 != 0 and a 4-D X: alone, bit for bit the model's own fit
    for shape in ((20, 3, 3), (12, 4, 2, 4)):
        gs = torch.Generator().manual_seed(_seed("alone", shape))
        X = torch.randn(*shape, generator=gs).to(DEV)
        y = torch.randn(shape[0], generator=gs).to(DEV)
        B0 = [torch.randn(dd, 2, generator=gs) * 0.3 for dd in shape[1:]]
        mk = lambda: CP_linear_regression(shape, rank=2, device=DEV, Bcp_init=[b.clone().to(DEV) for b in B0])
        a, b = mk(), mk()
        rep = {}
        S.fit_Adam_many([a], X, y, max_iter=4, tol=0.0, Adam_kwargs={"lr": 0.01}, min_batch=1, report=rep)
        b.fit_Adam(X, y, max_iter=4, tol=0.0, Adam_kwargs={"lr": 0.01})
        assert rep == {"batched": [], "alone": [0], "groups": 0, "x_passes": 0}
        assert same_bits(bits(a), bits(b))
