"""GPU checks of the hierarchical multinomial module (multinomial_tensor_regression_hierarchical) and of
the grouped update step tr_adam_step_groups (k_update<true>).

  * every hier_* Adam fixture: probabilities, one loss + gradient and the 10-iteration factors at
    1e-5; the full trajectory: losses at 1e-5 with the same length and convergence flag, factors at
    1e-5 or no further from the fp64 restatement (tests/hier_ref.py) than twice the reference's own
    fp32 run
  * the LBFGS fixture, checked as tests/test_gpu_parity.py checks the multinomial one
  * hier_4d: the class factor comes back bitwise equal to its initial value
  * group_lr=None on a 3-D X: losses and factors bitwise those of the multinomial module's
    fit_Adam(weights=np.ones(C)) from the same start
  * the resident route: two runs bitwise equal; one iteration per launch bitwise equal to 64 per
    launch; a shape sweep (N 1 and 65, P odd and a multiple of 64, C 2 and 16, R 1 and 16, mixed
    non_negative, the largest N that fits) against the fp64 closed form; one sample past the
    envelope takes the streamed route
  * tr_adam_step_groups on synthetic arenas on both sides of the 1024-thread stride and of the
    2048-element trip (factor boundaries inside a trip, at 2048 + 1 and in the tail): three distinct
    learning rates, one group at lr 0, one factor outside the mask; steps 1 and 1000, with and
    without AMSGrad and weight decay; against fp64 torch.optim.Adam with param groups at the bar of
    tests/test_gpu_update.py (e <= 2 e_torch32 + 2^-22, e the measure of update_ref.err)
"""
import functools

import numpy as np
import pytest
import torch

import hier_ref
import update_ref as ur

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5
FLOOR32 = 2.0 ** -22


def _H():
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    return H


@functools.lru_cache(maxsize=None)
def fixture(name):
    return hier_ref.load(name)


@functools.lru_cache(maxsize=None)
def ref64(name):
    """The fp64 restatement of a fixture's full fit (computed once, shared, never modified)."""
    return hier_ref.fit_from_fixture(fixture(name), dtype=torch.float64)


def new_model(d):
    m = d["meta"]
    Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in d["Bcp0_list"]]
    return _H().CP_logistic_regression(d["X_f32"], d["y"], rank=m["rank"], non_negative=m["non_negative"],
                                       weights=d["cp_weights"], Bcp_init=Bcp, device=DEV,
                                       softplus_kwargs=m["softplus_kwargs"])


def set_route(monkeypatch, route):
    """'streamed': TR_MNL_RESIDENT=0 (the multinomial plan + tr_adam_step_groups); 'resident': the default."""
    if route == "streamed":
        monkeypatch.setenv("TR_MNL_RESIDENT", "0")
    else:
        monkeypatch.delenv("TR_MNL_RESIDENT", raising=False)


def route_of(mm):
    return "resident" if "fit=resident" in mm._plan.describe else "streamed"


def expected_route(d, route):
    """Three feature modes (hier_4d) are outside the resident envelope: streamed whatever the switch says."""
    return "streamed" if len(d["Bcp0_list"]) != 3 else route


ROUTES = ["resident", "streamed"]


def run_fit(d, max_iter=None, **kw):
    m = d["meta"]
    mm = new_model(d)
    conv = mm.fit_Adam(lambda_L2=m["lambda_L2"], max_iter=m["max_iter"] if max_iter is None else max_iter,
                       tol=m["tol"], patience=m["patience"], Adam_kwargs=dict(m["adam_kwargs"]),
                       group_lr=m["group_lr"], **kw)
    return mm, conv


def factors(mm):
    return [A.detach().cpu().numpy() for A in mm.Bcp]


def assert_factors(got, want, tol=RTOL):
    for a, b in zip(got, want):
        a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
        e = hier_ref.normwise_rel(a, b)
        assert e <= tol, (e, np.shape(a))


def assert_streamed(mm):
    assert "resident" not in mm._plan.describe, mm._plan.describe


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", hier_ref.ADAM_FIXTURES)
def test_fixture_one_step_and_ten_iterations(name, route, monkeypatch):
    set_route(monkeypatch, route)
    d = fixture(name)
    m = d["meta"]
    mm = new_model(d)
    probs, pred = mm.predict()
    assert probs.shape == d["probs0"].shape
    assert np.max(np.abs(probs - d["probs0"])) <= RTOL * np.max(np.abs(d["probs0"]))
    assert pred.shape == (d["X_f32"].shape[0],)
    # one loss + gradient of every factor (the frozen ones included) at the initial point
    dev, Xd, yd = mm._device_data()
    plan = mm._get_plan(Xd, Xd.shape[0])
    cw, W = mm._class_weights(mm._ones(), dev, yd)
    assert W == d["X_f32"].shape[0]
    arena = plan.pack(mm.Bcp)
    grad = torch.zeros(plan.num_grads, device=DEV)
    gtot = torch.zeros(plan.num_params, device=DEV)
    loss = torch.zeros(1, device=DEV)
    plan.loss_grad(Xd, yd, cw, W, arena, mm.weights.to(DEV), grad)
    plan.finalize_grad(arena, grad, m["lambda_L2"], gtot, loss)
    print(f"{name}: loss {loss.item():.9g} want {float(d['loss0']):.9g}")
    assert abs(loss.item() - float(d["loss0"])) <= RTOL * abs(float(d["loss0"]))
    assert_factors(plan.factor_views(gtot), d["grads0_list"])
    m10, _ = run_fit(d, max_iter=min(10, m["max_iter"]))
    assert route_of(m10) == expected_route(d, route), m10._plan.describe
    assert np.allclose(m10.loss_running, d["loss_running_10"], rtol=RTOL, atol=0)
    assert_factors(factors(m10), d["Bcp_10_list"])


@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("name", hier_ref.ADAM_FIXTURES)
def test_fixture_full_trajectory(name, route, monkeypatch):
    set_route(monkeypatch, route)
    d = fixture(name)
    mm, conv = run_fit(d)
    assert route_of(mm) == expected_route(d, route), mm._plan.describe
    assert len(mm.loss_running) == len(d["loss_running"])
    assert int(conv) == int(d["converged"])
    ours = np.asarray(mm.loss_running)
    e_loss = np.max(np.abs(ours - d["loss_running"]) / np.abs(d["loss_running"]))
    r64 = ref64(name)
    e32 = hier_ref.normwise_rel(factors(mm), d["Bcp_final_list"])
    e64 = hier_ref.normwise_rel(factors(mm), r64["Bcp"])
    print(f"{name} {route}: loss {e_loss:.2e}  factors vs fp32 {e32:.2e}  vs fp64 {e64:.2e}  "
          f"reference fp32 vs fp64 {float(d['drift_factors']):.2e}")
    assert e_loss <= RTOL
    for a, b, c in zip(factors(mm), d["Bcp_final_list"], r64["Bcp"]):
        if hier_ref.normwise_rel(a, b) <= RTOL:
            continue
        assert hier_ref.normwise_rel(a, c) <= 2.0 * hier_ref.normwise_rel(b, c), (name, a.shape)


def test_4d_class_factor_is_frozen_bitwise():
    d = fixture("hier_4d")
    mm, _ = run_fit(d)
    assert_streamed(mm)  # three feature modes: outside the resident envelope
    got = factors(mm)
    assert np.array_equal(got[3].view(np.int32), d["Bcp0_list"][3].view(np.int32))
    for f in range(3):
        assert not np.array_equal(got[f], d["Bcp0_list"][f])
    # the frozen factor's norm is in the recorded loss: lambda * ||Bcp[3]|| is far above the bar
    lam = d["meta"]["lambda_L2"]
    assert lam * np.linalg.norm(d["Bcp0_list"][3]) > 100 * RTOL * mm.loss_running[0]


@pytest.mark.parametrize("name", ["hier_kim", "hier_signed", "hier_wd", "hier_converge"])
def test_streamed_route_is_bitwise_the_multinomial_module(name, monkeypatch):
    """group_lr=None on a 3-D X: the new module must not fork the math."""
    from tensor_regression_amd import multinomial_tensor_regression as M
    set_route(monkeypatch, "streamed")
    d = fixture(name)
    m = d["meta"]
    iters = min(m["max_iter"], 200)
    mm = new_model(d)
    conv = mm.fit_Adam(lambda_L2=m["lambda_L2"], max_iter=iters, tol=m["tol"], patience=m["patience"],
                       Adam_kwargs=dict(m["adam_kwargs"]))
    assert_streamed(mm)
    Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in d["Bcp0_list"]]
    mr = M.CP_logistic_regression(d["X_f32"], d["y"], rank=m["rank"], non_negative=m["non_negative"],
                                  weights=d["cp_weights"], Bcp_init=Bcp, device=DEV,
                                  softplus_kwargs=m["softplus_kwargs"])
    convr = mr.fit_Adam(lambda_L2=m["lambda_L2"], max_iter=iters, tol=m["tol"], patience=m["patience"],
                        weights=np.ones(m["n_classes"]), Adam_kwargs=dict(m["adam_kwargs"]))
    assert conv == convr and len(mm.loss_running) == len(mr.loss_running)
    assert np.array_equal(np.asarray(mm.loss_running).view(np.int64), np.asarray(mr.loss_running).view(np.int64))
    for a, b in zip(factors(mm), factors(mr)):
        assert np.array_equal(a.view(np.int32), b.view(np.int32))


@pytest.mark.parametrize("route", ROUTES)
def test_second_fit_continues_the_loss_history(route, monkeypatch):
    """loss_running carries over into a second fit_Adam (the plateau slice reads the earlier entries)."""
    set_route(monkeypatch, route)
    d = fixture("hier_signed")
    m = d["meta"]
    mm, _ = run_fit(d, max_iter=7)
    mm.fit_Adam(lambda_L2=m["lambda_L2"], max_iter=5, tol=0.0, patience=3, Adam_kwargs=dict(m["adam_kwargs"]))
    assert len(mm.loss_running) == 12 and route_of(mm) == route
    r = hier_ref.fit_from_fixture(d, max_iter=7)
    r2 = hier_ref.fit_adam(d["X_f32"], d["y"], r["Bcp"], d["cp_weights"], m["non_negative"], m["lambda_L2"], 5, 0.0, 3,
                           m["adam_kwargs"], softplus_kwargs=m["softplus_kwargs"], loss_running=r["loss_running"])
    assert np.allclose(mm.loss_running, r2["loss_running"], rtol=RTOL, atol=0)
    assert_factors(factors(mm), r2["Bcp"])


def test_lbfgs_fixture():
    """CP_logistic_regression.fit (hierarchical…py:292-381) optimises every factor; checked as
    tests/test_gpu_parity.py::test_multinomial_lbfgs_golden checks the multinomial module's: the first
    logged loss at 1e-5, every later one within 1e-5 of the reference's fp32 run or no further from the
    fp64 run than the reference's fp32 run has been up to that step (x2)."""
    from oracle import cp_oracle
    H = _H()
    d = fixture("hier_lbfgs")
    m = d["meta"]
    Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in d["Bcp0_list"]]
    mm = H.CP_logistic_regression(d["X_f32"], d["y"], rank=m["rank"], Bcp_init=Bcp, device=DEV)
    conv = mm.fit(lambda_L2=m["lambda_L2"], max_iter=m["max_iter"], tol=0.0, patience=100,
                  running_loss_logging_interval=m["logging_interval"], LBFGS_kwargs=m["lbfgs_kwargs"])
    assert int(conv) == int(d["converged"])
    assert len(mm.loss_running) == len(d["loss_running"])
    r64 = cp_oracle.fit_lbfgs_mnl(d["X_f32"], d["y"], d["Bcp0_list"], np.ones(m["rank"]), m["non_negative"],
                                  np.ones(m["n_classes"]), m["lambda_L2"], m["max_iter"], 0.0, 100,
                                  m["logging_interval"], m["lbfgs_kwargs"], dtype=torch.float64)
    ours, r32, r64l = (np.asarray(v, np.float64) for v in (mm.loss_running, d["loss_running"], r64["loss_running"]))
    assert abs(ours[0] - r32[0]) <= RTOL * abs(r32[0])
    spread = np.maximum.accumulate(np.abs(r32 - r64l))
    ok = (np.abs(ours - r32) <= RTOL * np.abs(r32)) | (np.abs(ours - r64l) <= 2 * spread + RTOL * np.abs(r64l))
    assert ok.all(), (ours, r32, r64l)
    assert not np.array_equal(factors(mm)[2], d["Bcp0_list"][2])  # the class factor moved
    probs, pred = mm.predict()
    assert probs.shape == (96, 4) and pred.shape == (96,)
    cm, acc = mm.make_confusion_matrix()
    assert cm.shape == (4, 4) and 0.0 <= acc <= 1.0


# ---- tr_adam_step_groups on synthetic arenas ---------------------------------------------------

# name -> (feature dims, classes, rank, intended num_params)
ARENAS = {
    "g3_1023": ((20, 10), 3, 31, 1023),    # one element short of the stride
    "g3_1054": ((20, 10), 4, 31, 1054),    # thread 0..29 take a second element
    "g3_2180": ((64, 40), 5, 20, 2180),    # three trips
    "g4_126": ((6, 5, 4), 3, 7, 126),
    "g4_1105": ((30, 20, 10), 5, 17, 1105),
    # 3 * 1024 + 5 elements: the step takes two elements per trip (t, t + 1024), so one full trip
    # [0, 2048), a second trip for threads 0..4 (2048 + t, 3072 + t) and a one-element tail for the
    # rest.  The middle factor is the one the "masked" groups leave out.
    #   boundaries 5 (inside a trip: threads 0..4 hold f0 and f1) and 2049 = 2048 + 1 (thread 0's
    #   second trip holds 2048 of the masked f1 and 3072 of f2)
    "g3_3077": ((5, 2044), 1028, 1, 3077),
    #   boundaries 7 (inside a trip) and 2600 (in the one-element tail)
    "g3_3077t": ((7, 2593), 477, 1, 3077),
}
HP = {
    "plain": ur.hparams(),
    "ams_wd": ur.hparams(beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.01, amsgrad=True),
}
LAM = 0.03
# name -> (learning rates of the first three factors, factors in a param group)
GROUPS = {
    "distinct": ((0.02, 0.005, 0.0007), None),
    "lr0": ((0.02, 0.0, 0.003), None),
    "masked": ((0.02, 0.005, 0.0007), "drop_last"),
}


class Arena:
    def __init__(self, name):
        from tensor_regression_amd import _engine, _lib
        dims, ncls, rank, total = ARENAS[name]
        self.name = name
        self.plan = _engine.Plan(_lib.TR_MODEL_MULTINOMIAL, dims, ncls, rank, 1, [False] * (len(dims) + 1), None, DEV)
        self.shapes = [tuple(s) for s in self.plan.factor_shapes()]
        self.nf = len(self.shapes)
        self.off = list(self.plan.offsets[:self.nf + 1])
        self.np = self.plan.num_params
        assert self.np == total == self.off[self.nf] and self.plan.num_grads == total + 2


@functools.lru_cache(maxsize=None)
def arena_of(name):
    return Arena(name)


def _mag(rng, n):
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n)


def make_inputs(a, rng, zero_state, hp):
    P = a.np
    params = (0.5 * rng.standard_normal(P)).astype(np.float32)
    grad = np.zeros(P + 2, np.float32)
    grad[:P] = _mag(rng, P).astype(np.float32)
    grad[P] = np.float32(rng.uniform(0.5, 2.0))
    if zero_state:
        m, v, vmax = (np.zeros(P, np.float32) for _ in range(3))
    else:
        m = _mag(rng, P).astype(np.float32)
        v = (_mag(rng, P) ** 2).astype(np.float32)
        g64, _ = ur.total_grad(params, grad[:P], float(grad[P]), ur.make_penalty("l2", a.off, a.shapes, LAM))
        g64 = g64 + hp["weight_decay"] * params.astype(np.float64)
        vnew = hp["beta2"] * v.astype(np.float64) + (1.0 - hp["beta2"]) * g64 * g64
        vmax = (vnew * np.where(rng.random(P) < 0.5, 1.5, 0.5)).astype(np.float32)
    return dict(params=params, grad=grad, m=m, v=v, vmax=vmax)


def torch_groups_step(a, inp, hp, t, lrs, stepped, dtype):
    """torch.optim.Adam (CPU, foreach=False) with one param group per stepped factor, the state
    preloaded as after step t - 1; the unstepped factors are leaves the optimizer never sees.
    Returns (params, m, v, vmax, total gradient, total loss) as flat numpy arrays in `dtype`."""
    leaves = [torch.tensor(inp["params"][a.off[f]:a.off[f + 1]].reshape(a.shapes[f]), dtype=dtype,
                           requires_grad=True) for f in range(a.nf)]
    opt = torch.optim.Adam([{"params": leaves[f], "lr": lrs[f]} for f in stepped], lr=1.0,
                           betas=(hp["beta1"], hp["beta2"]), eps=hp["eps"], weight_decay=hp["weight_decay"],
                           amsgrad=hp["amsgrad"], foreach=False)
    for f in stepped:
        sl = slice(a.off[f], a.off[f + 1])
        st = {"step": torch.tensor(float(t - 1)),
              "exp_avg": torch.tensor(inp["m"][sl].reshape(a.shapes[f]), dtype=dtype).clone(),
              "exp_avg_sq": torch.tensor(inp["v"][sl].reshape(a.shapes[f]), dtype=dtype).clone()}
        if hp["amsgrad"]:
            st["max_exp_avg_sq"] = torch.tensor(inp["vmax"][sl].reshape(a.shapes[f]), dtype=dtype).clone()
        opt.state[leaves[f]] = st
    pen = 0
    for A in leaves:
        pen = pen + torch.sqrt(torch.sum(A ** 2))
    (LAM * pen).backward()
    total = torch.tensor(float(inp["grad"][a.np]), dtype=dtype) + LAM * pen.detach()
    for f, A in enumerate(leaves):
        A.grad = A.grad + torch.tensor(inp["grad"][a.off[f]:a.off[f + 1]].reshape(a.shapes[f]), dtype=dtype)
    gtot = np.concatenate([A.grad.numpy().reshape(-1).copy() for A in leaves])
    opt.step()
    out = {k: np.asarray(inp[k], dtype=np.float64 if dtype == torch.float64 else np.float32).copy()
           for k in ("params", "m", "v", "vmax")}
    for f in stepped:
        sl = slice(a.off[f], a.off[f + 1])
        st = opt.state[leaves[f]]
        out["params"][sl] = leaves[f].detach().numpy().reshape(-1)
        out["m"][sl] = st["exp_avg"].numpy().reshape(-1)
        out["v"][sl] = st["exp_avg_sq"].numpy().reshape(-1)
        if hp["amsgrad"]:
            out["vmax"][sl] = st["max_exp_avg_sq"].numpy().reshape(-1)
    out["gtot"], out["total"] = gtot, float(total)
    return out


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.int32).copy()


@pytest.mark.parametrize("t", [1, 1000])
@pytest.mark.parametrize("hpname", list(HP))
@pytest.mark.parametrize("gname", list(GROUPS))
@pytest.mark.parametrize("aname", list(ARENAS))
def test_adam_step_groups_against_fp64_param_groups(aname, gname, hpname, t):
    a, hp = arena_of(aname), HP[hpname]
    lrs3, mask = GROUPS[gname]
    # factors past the third are never in a group; "masked" also leaves the last of the plan's out
    stepped = [f for f in range(min(3, a.nf))]
    if mask == "drop_last" and a.nf == 3:
        stepped = [0, 2]  # a factor in the middle of the arena outside the mask
    lrs = list(lrs3) + [0.0] * (a.nf - 3)
    rng = np.random.default_rng(sum(map(ord, aname + gname + hpname)) + t)
    inp = make_inputs(a, rng, zero_state=(t == 1), hp=hp)
    ref = torch_groups_step(a, inp, hp, t, lrs, stepped, torch.float64)
    yard = torch_groups_step(a, inp, hp, t, lrs, stepped, torch.float32)
    d = {k: torch.tensor(x, device=DEV) for k, x in inp.items()}
    hist = torch.full((8,), -1234.5, dtype=torch.float64, device=DEV)
    stop = torch.zeros(1, dtype=torch.int32, device=DEV)
    a.plan.adam_step_groups(d["params"], d["grad"], d["m"], d["v"], d["vmax"] if hp["amsgrad"] else None, LAM, hp,
                            lrs, stepped, t, hist, 2, 3, 10, 0.0, stop)
    got = {k: d[k].cpu().numpy() for k in ("params", "m", "v", "vmax")}
    keys = ["params", "m", "v"] + (["vmax"] if hp["amsgrad"] else [])
    bad = []
    for k in keys:
        e, ey = ur.err(got[k], ref[k]), ur.err(yard[k], ref[k])
        bound = 2.0 * ey + FLOOR32
        print(f"{aname} {gname} {hpname} t={t} {k}: e {e:.3e} e_torch {ey:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((k, e, ey, bound))
    assert not bad, bad
    # bookkeeping: the loss record in its slot only, the gradient arena and the stop flag untouched
    h = hist.cpu().numpy()
    assert float(np.float32(h[5])) == h[5]
    assert abs(h[5] - ref["total"]) <= 4 * float(np.spacing(np.float32(abs(ref["total"]))))
    assert (np.delete(h, 5) == -1234.5).all() and int(stop.item()) == 0
    assert np.array_equal(bits(d["grad"]), bits(inp["grad"]))
    if not hp["amsgrad"]:
        assert np.array_equal(bits(d["vmax"]), bits(inp["vmax"]))
    # a factor outside the mask: parameters and state bitwise untouched, its L2 term in the loss
    # (the total above holds every factor's norm) and in finalize_grad's total gradient
    for f in range(a.nf):
        sl = slice(a.off[f], a.off[f + 1])
        if f not in stepped:
            for k in ("params", "m", "v", "vmax"):
                assert np.array_equal(bits(got[k][sl]), bits(inp[k][sl])), (f, k)
            assert LAM * np.linalg.norm(inp["params"][sl]) > 1e3 * np.spacing(np.float32(ref["total"]))
        elif lrs[f] == 0.0:  # lr 0: the moments advance, the parameters do not move
            assert np.array_equal(bits(got["params"][sl]), bits(inp["params"][sl]))
            assert not np.array_equal(bits(got["m"][sl]), bits(inp["m"][sl]))
            assert not np.array_equal(bits(got["v"][sl]), bits(inp["v"][sl]))
        else:
            assert not np.array_equal(bits(got["params"][sl]), bits(inp["params"][sl]))
    gt = torch.zeros(a.np, device=DEV)
    lo = torch.zeros(1, device=DEV)
    a.plan.finalize_grad(torch.tensor(inp["params"], device=DEV), d["grad"], LAM, gt, lo)
    assert ur.err(gt.cpu().numpy(), ref["gtot"]) <= 2.0 * ur.err(yard["gtot"], ref["gtot"]) + FLOOR32


@pytest.mark.parametrize("aname", ["g3_1054", "g4_1105", "g3_3077", "g3_3077t"])
def test_adam_step_groups_one_lr_is_bitwise_adam_step(aname):
    a = arena_of(aname)
    if a.nf != 3:
        stepped = range(a.nf)  # every factor in a group (not the module's use, the kernel's general form)
    else:
        stepped = range(3)
    hp = dict(HP["ams_wd"], lr=0.013)
    inp = make_inputs(a, np.random.default_rng(5), zero_state=False, hp=hp)
    outs = []
    for grouped in (False, True):
        d = {k: torch.tensor(x, device=DEV) for k, x in inp.items()}
        hist = torch.zeros(4, dtype=torch.float64, device=DEV)
        stop = torch.zeros(1, dtype=torch.int32, device=DEV)
        if grouped:
            a.plan.adam_step_groups(d["params"], d["grad"], d["m"], d["v"], d["vmax"], LAM, hp, [0.013] * a.nf,
                                    stepped, 7, hist, 0, 1, 10, 0.0, stop)
        else:
            a.plan.adam_step(d["params"], d["grad"], d["m"], d["v"], d["vmax"], LAM, hp, 7, hist, 0, 1, 10, 0.0, stop)
        outs.append([bits(d[k]) for k in ("params", "m", "v", "vmax")] + [hist.cpu().numpy().view(np.int64)])
    for x, y in zip(*outs):
        assert np.array_equal(x, y)


def test_adam_step_groups_stop_rules_and_arguments():
    a = arena_of("g3_1054")
    hp = HP["plain"]
    inp = make_inputs(a, np.random.default_rng(9), zero_state=False, hp=hp)

    def step(stop_value=0, status=0.0, **kw):
        x = dict(inp)
        x["grad"] = inp["grad"].copy()
        x["grad"][a.np + 1] = status
        d = {k: torch.tensor(v, device=DEV) for k, v in x.items()}
        hist = torch.full((4,), -1234.5, dtype=torch.float64, device=DEV)
        stop = torch.full((1,), stop_value, dtype=torch.int32, device=DEV)
        a.plan.adam_step_groups(d["params"], d["grad"], d["m"], d["v"], None, LAM, hp, kw.get("lrs", [0.01] * 3),
                                kw.get("stepped", range(3)), 3, hist, 0, 2, 10, 0.0, stop)
        return d, hist.cpu().numpy(), int(stop.item())

    from tensor_regression_amd import _lib
    for d, h, s, want in [step(stop_value=5) + (5,), step(status=1.0) + (_lib.TR_STOP_DEVICE_ERROR - 2,)]:
        assert s == want and (h == -1234.5).all()
        for k in ("params", "m", "v"):
            assert np.array_equal(bits(d[k]), bits(inp[k]))
    for kw in (dict(lrs=[0.01, -0.01, 0.01]), dict(lrs=[0.01, float("nan"), 0.01]), dict(stepped=[0, 3])):
        with pytest.raises(ValueError):
            step(**kw)
    # a plateau: the grouped step launches the same k_converge
    d = {k: torch.tensor(v, device=DEV) for k, v in inp.items()}
    hist = torch.full((16,), float(inp["grad"][a.np]), dtype=torch.float64, device=DEV)
    stop = torch.zeros(1, dtype=torch.int32, device=DEV)
    a.plan.adam_step_groups(d["params"], d["grad"], d["m"], d["v"], None, 0.0, hp, [0.0] * 3, range(3), 9, hist, 0, 8,
                            3, 1e-3, stop)
    assert int(stop.item()) == 9


# ---- the resident route ------------------------------------------------------------------------

def bits_of_fit(mm):
    return [np.asarray(mm.loss_running).view(np.int64)] + [a.view(np.int32) for a in factors(mm)]


def test_resident_two_runs_are_bitwise_equal():
    d = fixture("hier_kim")
    a, _ = run_fit(d)
    b, _ = run_fit(d)
    assert route_of(a) == route_of(b) == "resident"
    for x, y in zip(bits_of_fit(a), bits_of_fit(b)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["hier_kim", "hier_converge", "hier_group_lr"])
def test_resident_one_iteration_per_launch_is_bitwise_sixty_four(name, capsys):
    """verbose=2 cuts the fit into one-iteration launches; the default is 64 per launch (cut at the
    group_lr breakpoints); a plateau stop falls inside a launch in one and at its end in the other."""
    d = fixture(name)
    a, ca = run_fit(d)
    b, cb = run_fit(d, verbose=2)
    out = capsys.readouterr().out
    assert out.count("Iteration:") == len(d["loss_running"])
    assert route_of(a) == route_of(b) == "resident" and ca == cb
    for x, y in zip(bits_of_fit(a), bits_of_fit(b)):
        assert np.array_equal(x, y)


def sweep_case(N, dims, C, R, nn, seed):
    rng = np.random.default_rng(seed)
    X = rng.standard_normal((N,) + dims).astype(np.float32)
    y = rng.integers(0, C, size=N).astype(np.int64)
    y[:min(N, C)] = np.arange(min(N, C))
    B0 = [(rng.random((k, R)) - (0.0 if nn[f] else 0.5)).astype(np.float32) for f, k in enumerate(dims + (C,))]
    w = (0.5 + rng.random(R)).astype(np.float32)
    return X, y, B0, w


def max_rows(dims, C, R):
    from tensor_regression_amd import _lib
    return int(_lib.load().tr_mnl_resident_max_rows(dims[0], dims[1], C, R))


NMAX_KIM = ("nmax", (8, 12), 4, 6)
SWEEP = [
    (1, (8, 12), 4, 6, [True] * 3),            # a single sample
    (65, (8, 12), 4, 6, [True] * 3),           # one sample past a wave
    (33, (5, 7), 3, 2, [False] * 3),           # P odd (the X pitch is P itself)
    (40, (8, 16), 3, 4, [True, False, True]),  # P a multiple of 64, mixed non_negative
    (50, (4, 6), 2, 3, [False, True, False]),  # C = 2
    # C = 16 (the widest sample row in registers).  96 samples, not fewer: at 37 (two a class) the fp32
    # CPU restatement itself, with only the sample order permuted, ends 1.3e-5 from fp64 on the class
    # factor after 10 iterations (an entry whose gradient is all rounding gets Adam's full step);
    # at 96 it stays within 2e-7
    (96, (6, 5), 16, 5, [True] * 3),
    (45, (7, 4), 3, 1, [True, True, False]),   # R = 1
    (29, (9, 8), 4, 16, [False] * 3),          # R = 16
    NMAX_KIM,                                  # the largest N that fits the notebook's features
]
LAM_SWEEP = 0.01


@pytest.mark.parametrize("case", SWEEP, ids=lambda c: "-".join(map(str, c[:4])).replace(" ", ""))
def test_resident_shape_sweep_against_fp64(case):
    """One loss + gradient at 1e-5 against the fp64 closed form, then 10 iterations against the fp64
    restatement.  The gradient is read from the kernel's own state: one resident iteration from zero
    Adam state with beta1 = 0 leaves exp_avg = the total gradient (data + L2), bitwise."""
    from tensor_regression_amd import _engine, _lib
    H = _H()
    if case[0] == "nmax":
        _, dims, C, R = case
        N, nn = max_rows(dims, C, R), [True] * 3
        assert 227 <= N < 65536  # the notebook's 227 samples are inside the envelope
    else:
        N, dims, C, R, nn = case
    X, y, B0, w = sweep_case(N, dims, C, R, nn, seed=N + 7 * C + R)
    ref = hier_ref.loss_grad(X, y, B0, w, nn, LAM_SWEEP, dtype=torch.float64)
    plan = _engine.Plan(_lib.TR_MODEL_MULTINOMIAL, dims, C, R, N, nn, None, DEV)
    assert plan.set_resident(True), plan.describe
    Xd, yd = torch.tensor(X, device=DEV), torch.tensor(y, device=DEV)
    arena = plan.pack([torch.tensor(a) for a in B0])
    m, v = torch.zeros_like(arena), torch.zeros_like(arena)
    hist = torch.zeros(2, dtype=torch.float64, device=DEV)
    stop = torch.zeros(1, dtype=torch.int32, device=DEV)
    hp = ur.hparams(lr=0.0, beta1=0.0)
    plan.fit_resident(Xd, yd, arena, torch.tensor(w, device=DEV), m, v, None, LAM_SWEEP, hp, [0.0] * 3, 1, 1, hist, 0,
                      0, 10, 0.0, stop)
    loss = float(hist[0].item())
    print(f"N {N} dims {dims} C {C} R {R}: loss {loss:.9g} fp64 {ref['loss']:.9g}")
    assert abs(loss - ref["loss"]) <= RTOL * abs(ref["loss"])
    assert_factors(plan.factor_views(m), ref["grads"])
    assert np.array_equal(arena.cpu().numpy(), np.concatenate([a.reshape(-1) for a in B0]))  # lr 0
    # 10 iterations through the module
    ak = {"lr": 0.01, "amsgrad": True}
    Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in B0]
    mm = H.CP_logistic_regression(X, y, rank=R, non_negative=nn, weights=w, Bcp_init=Bcp, device=DEV)
    mm.fit_Adam(lambda_L2=LAM_SWEEP, max_iter=10, tol=0.0, patience=10, Adam_kwargs=dict(ak))
    assert route_of(mm) == "resident"
    r64 = hier_ref.fit_adam(X, y, B0, w, nn, LAM_SWEEP, 10, 0.0, 10, ak, dtype=torch.float64)
    assert np.allclose(mm.loss_running, r64["loss_running"], rtol=RTOL, atol=0)
    assert_factors(factors(mm), r64["Bcp"])


def test_one_sample_past_the_envelope_takes_the_streamed_route():
    H = _H()
    _, dims, C, R = NMAX_KIM
    N = max_rows(dims, C, R) + 1
    nn = [True] * 3
    X, y, B0, w = sweep_case(N, dims, C, R, nn, seed=3)
    Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in B0]
    mm = H.CP_logistic_regression(X, y, rank=R, non_negative=nn, weights=w, Bcp_init=Bcp, device=DEV)
    ak = {"lr": 0.01, "amsgrad": True}
    mm.fit_Adam(lambda_L2=LAM_SWEEP, max_iter=10, tol=0.0, patience=10, Adam_kwargs=dict(ak))
    assert route_of(mm) == "streamed", mm._plan.describe
    r64 = hier_ref.fit_adam(X, y, B0, w, nn, LAM_SWEEP, 10, 0.0, 10, ak, dtype=torch.float64)
    assert np.allclose(mm.loss_running, r64["loss_running"], rtol=RTOL, atol=0)
    assert_factors(factors(mm), r64["Bcp"])


def test_resident_envelope_and_arguments():
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    assert lib.tr_mnl_resident_max_rows(8, 12, 17, 6) == 0 and lib.tr_mnl_resident_max_rows(8, 12, 4, 17) == 0
    assert lib.tr_mnl_resident_max_rows(8, 12, 16, 16) > 0
    assert lib.tr_mnl_resident_max_rows(400, 400, 4, 6) == 0  # B and G alone exceed the LDS
    # three feature modes, or a linear plan: the call succeeds and the plan stays streamed
    p3 = _engine.Plan(_lib.TR_MODEL_MULTINOMIAL, (3, 4, 5), 3, 2, 40, [False] * 4, None, DEV)
    assert p3.set_resident(True) is False
    pl = _engine.Plan(_lib.TR_MODEL_LINEAR, (8, 12), 1, 2, 40, [False] * 2, None, DEV)
    assert pl.set_resident(True) is False
    p = _engine.Plan(_lib.TR_MODEL_MULTINOMIAL, (8, 12), 4, 6, 40, [True] * 3, None, DEV)
    assert p.set_resident(True) is True and p.set_resident(False) is False and "resident" not in p.describe
    z = torch.zeros(p.num_params, device=DEV)
    X = torch.zeros(40, 8, 12, device=DEV)
    y = torch.zeros(40, dtype=torch.int64, device=DEV)
    hist = torch.zeros(4, dtype=torch.float64, device=DEV)
    stop = torch.zeros(1, dtype=torch.int32, device=DEV)
    w = torch.ones(6, device=DEV)
    hp = ur.hparams()
    with pytest.raises(ValueError):  # not on the resident route
        p.fit_resident(X, y, z, w, z.clone(), z.clone(), None, 0.0, hp, [0.01] * 3, 1, 1, hist, 0, 0, 10, 0.0, stop)
    assert p.set_resident(True)
    for kw in (dict(n=0), dict(n=65), dict(step=0), dict(lr=[0.01, -1.0, 0.01])):
        with pytest.raises(ValueError):
            p.fit_resident(X, y, z, w, z.clone(), z.clone(), None, 0.0, hp, kw.get("lr", [0.01] * 3), kw.get("step", 1),
                           kw.get("n", 1), hist, 0, 0, 10, 0.0, stop)
    with pytest.raises(ValueError):  # more rows than the plan was made for
        p.fit_resident(torch.zeros(41, 8, 12, device=DEV), y, z, w, z.clone(), z.clone(), None, 0.0, hp, [0.01] * 3, 1,
                       1, hist, 0, 0, 10, 0.0, stop)


def test_verbose_lines_of_both_fits(capsys):
    """verbose=2 of fit and fit_Adam: 'Iteration: i, Loss: l' per logged iteration with the logged
    loss, then the convergence line."""
    d = fixture("hier_lbfgs")
    m = d["meta"]
    for adam in (False, True):
        mm = new_model(d)
        if adam:
            conv = mm.fit_Adam(lambda_L2=m["lambda_L2"], max_iter=2, tol=0.0, verbose=2, Adam_kwargs={'lr': 0.01})
        else:
            conv = mm.fit(lambda_L2=m["lambda_L2"], max_iter=2, tol=0.0, verbose=2, running_loss_logging_interval=1,
                          LBFGS_kwargs=m["lbfgs_kwargs"])
        assert conv is False and len(mm.loss_running) == 2
        assert capsys.readouterr().out.splitlines() == [
            f'Iteration: {ii}, Loss: {loss}' for ii, loss in enumerate(mm.loss_running)] + [
            "Reached maximum number of iterations without convergence"]
