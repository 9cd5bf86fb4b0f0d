"""The shared-X multinomial sweep on the GPU: multinomial_tensor_regression.fit_Adam_many and the
tr_mnl_many_* entries against the CPU oracle (oracle/cp_oracle.py), the golden fixtures and the
single-model route.

Data as in test_gpu_linear_many.py: randn X, factors 0.3 * randn, CP weights in 0.5..1.5, alternating
non_negative, ranks from (1, 3, 8, 32), Adam settings mixed, class weights and labels of their own on
every other member, seeds from crc32 of the case.  Bars: those of tests/test_gpu_parity.py's multinomial
tests, unchanged: losses within RTOL = 1e-5, factors after 10 iterations within 1e-5 normwise (or as
accurate as the oracle's own fp32 run), factor gradients of one evaluation against the fp64 closed form
beside the oracle's own fp32: e32 <= max(1e-5, 2 e_ref) and e <= 2 e_ref + 1e-7.  Shapes (N, I, J) with
the members' class counts, each the smallest at which a kernel takes another path:

  (3, 8, 4)       C = 2 x 2        fewer rows than a 16-row tile
  (37, 8, 12)     C = 5 x 12       ragged row tile, zero-filled 32-feature tail, 60 columns in four tiles
                                   (the last partly filled), members straddling tile boundaries
  (130, 16, 16)   C = 3 x 5, x 6   15 columns in one tile, 18 in two; two forward workgroups
  (257, 24, 20)   C = 10 x 6       two epilogue workgroups, several gradient chunks
  (64, 16, 8)     C = 16 x 4       exactly 64 columns
  (64, 16, 8)     C = 2,5,16,3,7   mixed class counts
  (48, 256, 128)  C = 5 x 3        the 512-feature fold inside a slice, many slices and gradient waves
  (292, 9, 12)    C = 4 x 4        util.windowed_view, row stride 12 < P = 108
  (130, 16, 16)+4 C = 3 x 5        rows cut from a buffer with row stride P + 4
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
CASES = {
    "rows3": ((3, 8, 4), "plain", [2, 2]),
    "ragged37": ((37, 8, 12), "plain", [5] * 12),
    "tile1": ((130, 16, 16), "plain", [3] * 5),
    "tile2": ((130, 16, 16), "plain", [3] * 6),
    "c10": ((257, 24, 20), "plain", [10] * 6),
    "full64": ((64, 16, 8), "plain", [16] * 4),
    "mixed": ((64, 16, 8), "plain", [2, 5, 16, 3, 7]),
    "c2row": ((48, 256, 128), "plain", [5] * 3),
    "windowed": ((292, 9, 12), "windowed", [4] * 4),
    "padded": ((130, 16, 16), "padded", [3] * 5),
}


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 2**31


_X = {}


def make_x(name):
    """(X on the device in the case's layout, the same X contiguous on the host); made once per case."""
    if name in _X:
        return _X[name]
    shape, kind, _ = CASES[name]
    N, I, J = shape
    P = I * J
    g = torch.Generator().manual_seed(_seed("x", shape, kind))
    if kind == "windowed":
        from tensor_regression_amd.util import windowed_view
        series = torch.randn(N + I - 1, J, generator=g)
        Xd, _ = windowed_view(series.to(DEV), torch.zeros(N + I - 1, device=DEV), (0, I))
        Xh, _ = windowed_view(series, torch.zeros(N + I - 1), (0, I))
        assert tuple(Xd.shape) == shape and Xd.stride(0) == J < P
        out = (Xd, Xh.contiguous())
    elif kind == "padded":
        base = torch.randn(N * (P + 4), generator=g)
        out = (torch.as_strided(base.to(DEV), shape, (P + 4, J, 1)),
               torch.as_strided(base, shape, (P + 4, J, 1)).contiguous())
    else:
        Xh = torch.randn(*shape, generator=g)
        out = (Xh.to(DEV), Xh)
    _X[name] = out
    return out


def labels(N, C, g):
    y = torch.randint(0, C, (N,), generator=g)
    k = min(N, C)
    y[:k] = torch.arange(k)  # (with N < C the class count comes from Bcp_init)
    return y


def make_specs(name, Cs=None, vary=0):
    """One member description per class count: ranks, lambda, lr, amsgrad, weight decay, softplus
    settings mixed; class weights and labels of its own on every other member.  `vary` reseeds."""
    (N, I, J), _, cs = CASES[name]
    Cs = cs if Cs is None else Cs
    specs = []
    for j, C in enumerate(Cs):
        gj = torch.Generator().manual_seed(_seed("m", name, j, C, vary))
        gy = torch.Generator().manual_seed(_seed("y", name, C, j if j % 2 else "shared"))
        R = RANKS[j % 4]
        ak = {"lr": 0.01 * (1 + j % 3)}
        if j % 2:
            ak["amsgrad"] = True
        if j % 3 == 2:
            ak.update(weight_decay=0.01, betas=(0.8, 0.99), eps=1e-6)
        specs.append(types.SimpleNamespace(
            C=C, rank=R, nn=[bool(j % 2), bool((j + 1) % 2), bool(j % 3 == 0)],
            Bcp0=[torch.randn(d, R, generator=gj) * 0.3 for d in (I, J, C)],
            w=torch.rand(R, generator=gj) + 0.5, lam=0.01 * (1 + j) + 0.003 * vary, ak=ak,
            sp=None if j % 4 else {"beta": 20, "threshold": 2},
            cw=((torch.rand(C, generator=gj) + 0.5).numpy() if j % 2 else np.ones(C, np.float32)),
            y=labels(N, C, gy)))
    return specs


def build_model(s, Xd):
    from tensor_regression_amd import CP_logistic_regression
    return CP_logistic_regression(Xd, s.y, rank=s.rank, non_negative=list(s.nn), weights=s.w.numpy(), device=DEV,
                                  Bcp_init=[b.clone().to(DEV) for b in s.Bcp0], softplus_kwargs=s.sp)


_ORACLE = {}


def oracle_fit(key, Xh, s, max_iter, tol=0.0, patience=10, dtype=torch.float32):
    from oracle import cp_oracle
    key = (key, max_iter, tol, patience, dtype)
    if key not in _ORACLE:
        _ORACLE[key] = cp_oracle.fit_adam_mnl(Xh, s.y, s.Bcp0, s.w, s.nn, s.cw, s.lam, max_iter, tol, patience, s.ak,
                                              s.sp, dtype=dtype)
    return _ORACLE[key]


def bits(model):
    return [A.detach().cpu().numpy().copy() for A in model.Bcp] + [np.array(model.loss_running)]


def same_bits(a, b):
    return all(x.shape == y.shape and np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


# ---- the C entries, driven directly (cases 1 and 2) ---------------------------------------------------

def device_members(Xd, specs, hist_len=8):
    """The group's members with their own device state, the buffers and the tr_mnl_many_member array."""
    from tensor_regression_amd import _engine
    N, I, J = (int(d) for d in Xd.shape)
    members = []
    for s in specs:
        n = (I + J + s.C) * s.rank
        _, beta, thr = _engine.nonlin_key(s.nn, s.sp, 3)
        cw = torch.as_tensor(s.cw, dtype=torch.float32)
        members.append(types.SimpleNamespace(
            arena=torch.cat([b.reshape(-1) for b in s.Bcp0]).to(DEV), w=s.w.to(DEV), y=s.y.to(DEV), cw=cw.to(DEV),
            W=float(cw.double()[s.y].sum()), grad=torch.zeros(n + 2, device=DEV), m=torch.zeros(n, device=DEV),
            v=torch.zeros(n, device=DEV), vmax=torch.zeros(n, device=DEV) if s.ak.get("amsgrad") else None,
            hist=torch.zeros(hist_len, dtype=torch.float64, device=DEV),
            stop=torch.zeros(1, dtype=torch.int32, device=DEV), n_classes=s.C, rank=s.rank, nonneg=s.nn, beta=beta,
            thr=thr, lambda_L2=s.lam, hp=_engine.adam_hparams(s.ak), patience=10, tol=0.0, hist_base=0))
    bufs = _engine.MnlManyBuffers(0, N, I, J, len(members))
    arr, rec = _engine.mnl_many_member_array(members)
    return members, bufs, arr, rec


def evaluate(Xd, specs):
    """tr_mnl_many_loss_grad on the group: returns the members (with arena, grad, ...) and buffers."""
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    N, I, J = (int(d) for d in Xd.shape)
    members, bufs, arr, rec = device_members(Xd, specs)
    xld = Xd.stride(0) if N > 1 else I * J
    _lib.check(lib.tr_mnl_many_loss_grad(0, _lib.ptr(Xd), N, xld, I, J, arr, len(members), _lib.ptr(bufs.ws),
                                         bufs.ws_bytes, _lib.ptr(bufs.table_host), _lib.ptr(bufs.table_dev),
                                         bufs.table_bytes, _engine.stream_handle(0)), "tr_mnl_many_loss_grad")
    torch.cuda.synchronize()
    return members, bufs, arr, rec


@pytest.mark.parametrize("name", list(CASES))
def test_one_evaluation(name):
    """tr_mnl_many_loss_grad per member against cp_oracle.mnl_loss_grad and closed_form_mnl.  The L2
    term is added by the member's own plan (tr_finalize_grad), which reads the arena in tr_loss_grad's
    layout."""
    from oracle import cp_oracle
    Xd, Xh = make_x(name)
    N = Xh.shape[0]
    specs = make_specs(name)
    members, _, _, _ = evaluate(Xd, specs)
    for j, (s, mb) in enumerate(zip(specs, members)):
        ref = cp_oracle.mnl_loss_grad(Xh, s.y, s.Bcp0, s.w, s.nn, s.cw, s.lam, s.sp)
        c64 = cp_oracle.closed_form_mnl(Xh.double().numpy(), s.y.numpy(), [b.double().numpy() for b in s.Bcp0],
                                        s.w.double().numpy(), s.nn, s.cw, s.lam, s.sp)
        plan = build_model(s, Xd)._get_plan(Xd, N)
        n = plan.num_params
        assert mb.grad.numel() == plan.num_grads and mb.grad[n + 1].item() == 0.0
        gtot, loss = torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
        plan.finalize_grad(mb.arena, mb.grad, s.lam, gtot, loss)
        dl = mb.grad[n].item()
        errs = []
        for a, o, w in zip(plan.factor_views(gtot), ref["grads"], c64["grads"]):
            a = a.cpu().numpy()
            errs.append((normwise_rel(a, o), normwise_rel(a, w), normwise_rel(o, w)))
        print(f"{name} member {j} C {s.C} rank {s.rank}: data loss {dl:.8g} vs {ref['data_loss']:.8g}, "
              f"(e32, e, e_ref) per factor {errs}")
        assert abs(dl - ref["data_loss"]) <= RTOL * abs(ref["data_loss"]), (j, dl, ref["data_loss"])
        assert abs(loss.item() - ref["loss"]) <= RTOL * abs(ref["loss"]), (j, loss.item(), ref["loss"])
        for e32, e, e_ref in errs:
            assert e32 <= max(1e-5, 2 * e_ref), (j, e32, e_ref)
            assert e <= 2 * e_ref + 1e-7, (j, e, e_ref)


@pytest.mark.parametrize("j", [0, 1, 2])
def test_update_equivalence(j):
    """On one member's gradient arena, tr_mnl_many_step and the plan's adam_step (k_update) give bitwise
    equal parameters, m, v, vmax and loss record.  Members 0, 1, 2: Adam, AMSGrad, AMSGrad with weight
    decay and other betas."""
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    name = "ragged37"
    Xd, Xh = make_x(name)
    specs = make_specs(name)[:3]
    members, bufs, arr, rec = evaluate(Xd, specs)
    mb, s = members[j], specs[j]
    plan = build_model(s, Xd)._get_plan(Xd, Xh.shape[0])
    a2, m2, v2 = mb.arena.clone(), torch.zeros_like(mb.m), torch.zeros_like(mb.v)
    x2 = torch.zeros_like(mb.vmax) if mb.vmax is not None else None
    h2, stop2 = torch.zeros_like(mb.hist), torch.zeros_like(mb.stop)
    step, it = 3, 2  # a step whose bias corrections are not those of step 1
    plan.adam_step(a2, mb.grad, m2, v2, x2, s.lam, mb.hp, step, h2, 0, it, 10, 0.0, stop2)
    rec["n_iters"], rec["step"], rec["iter"] = 1, step, it
    I, J = int(Xd.shape[1]), int(Xd.shape[2])
    _lib.check(lib.tr_mnl_many_step(0, I, J, arr, len(members), _lib.ptr(bufs.table_host),
                                    _lib.ptr(bufs.table_dev), bufs.table_bytes, _engine.stream_handle(0)),
               "tr_mnl_many_step")
    torch.cuda.synchronize()
    pairs = [(mb.arena, a2), (mb.m, m2), (mb.v, v2), (mb.hist, h2)] + ([(mb.vmax, x2)] if x2 is not None else [])
    for got, want in pairs:
        assert np.array_equal(got.cpu().numpy().view(np.uint8), want.cpu().numpy().view(np.uint8))
    init = torch.cat([b.reshape(-1) for b in s.Bcp0])
    assert mb.hist[it].item() != 0.0 and not torch.equal(mb.arena.cpu(), init)  # a step was taken


# ---- fit_Adam_many against the oracle and the goldens (cases 3, 4, 5) ---------------------------------

def assert_fit_matches(key, model, s, Xh, max_iter, tol=0.0, patience=10):
    from test_gpu_parity import _assert_as_accurate_as_reference
    r32 = oracle_fit(key, Xh, s, max_iter, tol, patience)
    assert len(model.loss_running) == len(r32["loss_running"])
    np.testing.assert_allclose(model.loss_running, r32["loss_running"], rtol=RTOL)
    if all(normwise_rel(a.detach().cpu().numpy(), b) <= RTOL for a, b in zip(model.Bcp, r32["Bcp"])):
        return
    r64 = oracle_fit(key, Xh, s, max_iter, tol, patience, dtype=torch.float64)
    _assert_as_accurate_as_reference(model.Bcp, r32["Bcp"], r64["Bcp"])


def run_many(Xd, specs, **kw):
    from tensor_regression_amd.multinomial_tensor_regression import fit_Adam_many
    models = [build_model(s, Xd) for s in specs]
    report = {}
    kw.setdefault("max_iter", 10)
    kw.setdefault("tol", 0.0)
    kw.setdefault("min_batch", 1)
    conv = fit_Adam_many(models, lambda_L2=[s.lam for s in specs], weights=[s.cw for s in specs],
                         Adam_kwargs=[s.ak for s in specs], report=report, **kw)
    return models, conv, report


@pytest.mark.parametrize("name", list(CASES))
def test_ten_iterations(name):
    Xd, Xh = make_x(name)
    specs = make_specs(name)
    M = len(specs)
    models, conv, report = run_many(Xd, specs)
    assert conv == [False] * M
    assert report == {"batched": list(range(M)), "alone": [], "groups": 1, "x_passes": 20}
    for j, (model, s) in enumerate(zip(models, specs)):
        assert model._plan is None
        assert_fit_matches((name, j), model, s, Xh, 10)


def _mnl_model_from(d):
    from tensor_regression_amd import CP_logistic_regression
    m = d["meta"]
    return CP_logistic_regression(d["X"].to(DEV), d["y"], rank=m["rank"], non_negative=m["non_negative"],
                                  Bcp_init=[torch.tensor(a, device=DEV) for a in d["Bcp0_list"]], device=DEV,
                                  softplus_kwargs=m["softplus_kwargs"])


def _golden_group(gname, n_others=3):
    """The fixture's model and `n_others` drawn members on the same device X."""
    d = load(gname)
    first = _mnl_model_from(d)
    Xd = first.X
    N, I, J = d["X"].shape
    others = []
    for j in range(1, n_others + 1):
        g = torch.Generator().manual_seed(_seed(gname, j))
        C, R = (3, 5, 7)[j % 3], RANKS[j % 4]
        others.append(types.SimpleNamespace(
            C=C, rank=R, nn=[False, bool(j % 2), False], w=torch.rand(R, generator=g) + 0.5,
            Bcp0=[torch.randn(dd, R, generator=g) * 0.3 for dd in (I, J, C)], lam=0.02 * j, ak={"lr": 0.01}, sp=None,
            cw=np.ones(C, np.float32), y=labels(N, C, g)))
    return d, first, Xd, others


@pytest.mark.parametrize("gname", ["mnl_basic", "mnl_converge", "mnl_c10", "mnl_duo_shape"])
def test_golden_replayed_as_member_0(gname):
    """Member 0 is a golden fixture, the other members are drawn on the same X.  One evaluation against
    loss0 and grads0_list, ten iterations against loss_running_10 and Bcp_10_list, the full horizon
    against loss_running and converged; mnl_converge stops at its own iteration while the others run on."""
    from test_gpu_parity import _assert_factors
    from tensor_regression_amd.multinomial_tensor_regression import fit_Adam_many
    d, first, Xd, others = _golden_group(gname)
    m = d["meta"]
    cw0 = np.array(m["class_weights"], np.float32)
    s0 = types.SimpleNamespace(C=m["n_classes"], rank=m["rank"], nn=m["non_negative"], w=torch.ones(m["rank"]),
                               Bcp0=[torch.tensor(a) for a in d["Bcp0_list"]], lam=m["lambda_L2"],
                               ak=m["adam_kwargs"], sp=m["softplus_kwargs"], cw=cw0, y=torch.as_tensor(d["y"]))
    members, _, _, _ = evaluate(Xd, [s0] + others)
    plan = first._get_plan(Xd, Xd.shape[0])
    n = plan.num_params
    gtot, loss = torch.zeros(n, device=DEV), torch.zeros(1, device=DEV)
    plan.finalize_grad(members[0].arena, members[0].grad, m["lambda_L2"], gtot, loss)
    assert abs(loss.item() - d["loss0"]) <= RTOL * abs(d["loss0"])
    _assert_factors(plan.factor_views(gtot), d["grads0_list"])
    first._plan = None

    def fit(models, iters0):
        K = len(models) - 1
        return fit_Adam_many(models, lambda_L2=[m["lambda_L2"]] + [s.lam for s in others],
                             max_iter=[iters0] + [12] * K, tol=[m["tol"]] + [0.0] * K,
                             patience=[m["patience"]] + [10] * K, weights=[cw0] + [s.cw for s in others],
                             Adam_kwargs=[m["adam_kwargs"]] + [s.ak for s in others], min_batch=1)
    ten = [_mnl_model_from(d)] + [build_model(s, Xd) for s in others]
    ten[0].X = Xd
    fit(ten, min(10, m["max_iter"]))
    np.testing.assert_allclose(ten[0].loss_running, d["loss_running_10"], rtol=RTOL)
    _assert_factors(ten[0].Bcp, d["Bcp_10_list"])
    models = [first] + [build_model(s, Xd) for s in others]
    conv = fit(models, m["max_iter"])
    assert int(conv[0]) == int(d["converged"]) and len(first.loss_running) == len(d["loss_running"])
    np.testing.assert_allclose(first.loss_running, d["loss_running"], rtol=RTOL)
    assert [len(mm.loss_running) for mm in models[1:]] == [12] * len(others)
    for j, (model, s) in enumerate(zip(models[1:], others)):
        assert_fit_matches((gname, j), model, s, d["X"], 12)
    if d["converged"]:
        # stopped after len(loss_running) iterations while the others ran to 12: its factors are those
        # of a fit of exactly that length, bit for bit
        stop_at = len(d["loss_running"])
        assert stop_at < 12
        lone = _mnl_model_from(d)
        lone.X = Xd
        fit_Adam_many([lone], lambda_L2=m["lambda_L2"], max_iter=stop_at, tol=0.0, patience=m["patience"],
                      weights=cw0, Adam_kwargs=m["adam_kwargs"], min_batch=1)
        assert same_bits(bits(first)[:-1], bits(lone)[:-1])
        np.testing.assert_array_equal(first.loss_running, lone.loss_running)
    else:
        from oracle import cp_oracle
        from test_gpu_parity import _assert_as_accurate_as_reference
        r64 = cp_oracle.fit_adam_mnl(d["X"], d["y"], d["Bcp0_list"], np.ones(m["rank"]), m["non_negative"],
                                     m["class_weights"], m["lambda_L2"], m["max_iter"], m["tol"], m["patience"],
                                     m["adam_kwargs"], m["softplus_kwargs"], dtype=torch.float64)
        _assert_as_accurate_as_reference(first.Bcp, d["Bcp_final_list"], r64["Bcp"])


def test_stopped_member_is_left_untouched():
    """mnl_converge as member 0 of tr_mnl_many_fit calls of 4 iterations each: it stops at its own
    iteration (7) inside the second call; after that its parameters, Adam state and loss history no
    longer change while the other members go on."""
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    d, first, Xd, others = _golden_group("mnl_converge", 2)
    m = d["meta"]
    s0 = types.SimpleNamespace(C=m["n_classes"], rank=m["rank"], nn=m["non_negative"], w=torch.ones(m["rank"]),
                               Bcp0=[torch.tensor(a) for a in d["Bcp0_list"]], lam=m["lambda_L2"],
                               ak=m["adam_kwargs"], sp=m["softplus_kwargs"],
                               cw=np.array(m["class_weights"], np.float32), y=torch.as_tensor(d["y"]))
    members, bufs, arr, rec = device_members(Xd, [s0] + others, hist_len=32)
    rec["tol"], rec["patience"] = [m["tol"], 0.0, 0.0], [m["patience"], 10, 10]
    N, I, J = (int(x) for x in Xd.shape)
    snaps = []
    for ii in (0, 4, 8, 12):
        rec["n_iters"], rec["step"], rec["iter"] = 4, ii + 1, ii
        _lib.check(lib.tr_mnl_many_fit(0, _lib.ptr(Xd), N, Xd.stride(0), I, J, arr, len(members), _lib.ptr(bufs.ws),
                                       bufs.ws_bytes, _lib.ptr(bufs.table_host), _lib.ptr(bufs.table_dev),
                                       bufs.table_bytes, _engine.stream_handle(0)), "tr_mnl_many_fit")
        torch.cuda.synchronize()
        snaps.append([(mb.arena.clone(), mb.m.clone(), mb.v.clone(), mb.hist.clone(), int(mb.stop.item()))
                      for mb in members])
    assert [sn[0][4] for sn in snaps] == [0, 7, 7, 7] and len(d["loss_running"]) == 7
    assert all(sn[k][4] == 0 for sn in snaps for k in (1, 2))
    for t in range(4):  # parameters, m, v, history
        assert torch.equal(snaps[1][0][t], snaps[2][0][t]) and torch.equal(snaps[2][0][t], snaps[3][0][t])
        assert not torch.equal(snaps[2][1][t], snaps[3][1][t])  # the others went on
    assert not torch.equal(snaps[0][0][0], snaps[1][0][0])
    np.testing.assert_allclose(snaps[3][0][3][:7].cpu().numpy(), d["loss_running"], rtol=RTOL)
    assert (snaps[3][0][3][7:] == 0).all()


def test_second_fit_extends_loss_running():
    """A second fit_Adam_many on the same models continues loss_running exactly as a second fit_Adam
    does on a twin model (Adam restarts, the plateau test reads the earlier losses)."""
    name = "tile2"
    Xd, Xh = make_x(name)
    specs = make_specs(name)
    models, _, _ = run_many(Xd, specs, max_iter=6)
    from tensor_regression_amd.multinomial_tensor_regression import fit_Adam_many
    conv = fit_Adam_many(models, lambda_L2=[s.lam for s in specs], max_iter=5, tol=[0.0, 1e30] + [0.0] * 4,
                         patience=[10, 2] + [10] * 4, weights=[s.cw for s in specs],
                         Adam_kwargs=[s.ak for s in specs], min_batch=1)
    for j, (model, s) in enumerate(zip(models, specs)):
        twin = build_model(s, Xd)
        twin.fit_Adam(lambda_L2=s.lam, max_iter=6, tol=0.0, weights=s.cw, Adam_kwargs=s.ak)
        c2 = twin.fit_Adam(lambda_L2=s.lam, max_iter=5, tol=1e30 if j == 1 else 0.0, patience=2 if j == 1 else 10,
                           weights=s.cw, Adam_kwargs=s.ak)
        assert bool(conv[j]) == bool(c2) == (j == 1)
        assert len(model.loss_running) == len(twin.loss_running) == (6 + 4 if j == 1 else 11)
        np.testing.assert_allclose(model.loss_running, twin.loss_running, rtol=RTOL)
        for a, b in zip(model.Bcp, twin.Bcp):
            assert normwise_rel(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= RTOL


# ---- independence and reproducibility (case 6) --------------------------------------------------------

@pytest.mark.parametrize("name", ["ragged37", "c10"])
def test_independence_and_reproducibility(name):
    from tensor_regression_amd import _engine
    Xd, Xh = make_x(name)
    specs = make_specs(name)
    k = 3  # the member under test: at C = 5 its columns 15..19 straddle the first tile boundary
    a, _, _ = run_many(Xd, specs, max_iter=20)
    b, _, _ = run_many(Xd, specs, max_iter=20)
    for x, y in zip(a, b):
        assert same_bits(bits(x), bits(y))  # the same group twice
    want = bits(a[k])
    alone, _, rep = run_many(Xd, [specs[k]], max_iter=20)  # a group of one: one tile
    assert rep["batched"] == [0] and same_bits(want, bits(alone[0]))
    rest = specs[:k] + specs[k + 1:]
    first, _, _ = run_many(Xd, [specs[k]] + rest, max_iter=20)
    assert same_bits(want, bits(first[0]))
    last, _, _ = run_many(Xd, rest + [specs[k]], max_iter=20)
    assert same_bits(want, bits(last[-1]))
    perm = rest[::-1][:2] + [specs[k]] + rest[::-1][2:]  # other columns, other straddle
    moved, _, _ = run_many(Xd, perm, max_iter=20)
    assert same_bits(want, bits(moved[2]))
    other = make_specs(name, vary=1)  # other neighbours
    other[k] = specs[k]
    c, _, _ = run_many(Xd, other, max_iter=20)
    assert same_bits(want, bits(c[k])) and not same_bits(bits(a[1]), bits(c[1]))
    # the fit cut into chunks of 7 iterations instead of 64
    real = _engine.run_mnl_many
    _engine.run_mnl_many = lambda dev, X, mbs, **kw: real(dev, X, mbs, sync_every=7)
    try:
        cut, _, _ = run_many(Xd, specs, max_iter=20)
    finally:
        _engine.run_mnl_many = real
    for x, y in zip(a, cut):
        assert same_bits(bits(x), bits(y))


# ---- routing (case 7) ---------------------------------------------------------------------------------

def test_routing_on_the_device():
    """Two different X tensors, one model outside the envelope and 13 same-X models of C = 5: 12 + 1 on
    the first X, a group of 2 on the second, the outsider alone; every model within the bars of its own
    twin fitted by fit_Adam."""
    from tensor_regression_amd.multinomial_tensor_regression import fit_Adam_many
    Xa, _ = make_x("ragged37")
    Xb, _ = make_x("tile1")
    specs_a = make_specs("ragged37", [5] * 13)
    specs_b = make_specs("tile1", [3, 4])
    g = torch.Generator().manual_seed(_seed("outside"))
    Xo = torch.randn(40, 6, 5, generator=g).to(DEV)  # P = 30 is no multiple of 4
    so = types.SimpleNamespace(C=3, rank=2, nn=[False, True, False], w=torch.rand(2, generator=g) + 0.5,
                               Bcp0=[torch.randn(dd, 2, generator=g) * 0.3 for dd in (6, 5, 3)], lam=0.02,
                               ak={"lr": 0.01}, sp=None, cw=np.ones(3, np.float32), y=labels(40, 3, g))
    order = [(specs_a[0], Xa), (specs_b[0], Xb), (so, Xo)] + [(s, Xa) for s in specs_a[1:]] + [(specs_b[1], Xb)]
    models = [build_model(s, X) for s, X in order]
    report = {}
    fit_Adam_many(models, lambda_L2=[s.lam for s, _ in order], max_iter=4, tol=0.0, weights=[s.cw for s, _ in order],
                  Adam_kwargs=[s.ak for s, _ in order], min_batch=2, report=report)
    on_a = [0] + list(range(3, 15))
    assert report == {"batched": sorted(on_a[:12] + [1, 15]), "alone": [2, on_a[12]], "groups": 2, "x_passes": 16}
    for j, (model, (s, X)) in enumerate(zip(models, order)):
        twin = build_model(s, X)
        twin.fit_Adam(lambda_L2=s.lam, max_iter=4, tol=0.0, weights=s.cw, Adam_kwargs=s.ak)
        if j in report["alone"]:
            assert same_bits(bits(model), bits(twin))
            continue
        np.testing.assert_allclose(model.loss_running, twin.loss_running, rtol=RTOL)
        for a, b in zip(model.Bcp, twin.Bcp):
            assert normwise_rel(a.detach().cpu().numpy(), b.detach().cpu().numpy()) <= RTOL, j
