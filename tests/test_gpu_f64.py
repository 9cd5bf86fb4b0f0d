"""GPU checks of the float64 X pass (csrc/tr_fp64.hip behind tr_plan_create_f64 / tr_forward_f64 /
tr_loss_grad_f64): k64_prep, k64_dense, both instantiations of k64_rows, k64_cols, k64_reduce and k64_mttkrp,
with k64_update's closure mode (tr_finalize_grad_f64) behind them.  tests/test_gpu_update.py covers k64_update.

Every case is one loss_grad + finalize_grad + forward through CP_linear_regression(dtype=torch.float64)'s plan
on the draws of tests/f64_ref.py.  Per compared array (y_hat from forward and from loss_grad, the data loss,
the total loss, every factor's total gradient, the bias gradient),
    e = max_i |got_i - ref_i| / (|ref_i| + rms(ref))
against the closed form in numpy.longdouble must satisfy
    e <= 2 * e_yard + 2^-50    and    e <= 2^-40
where e_yard is the same measure of the closed form in float64 with every reduction one left-to-right chain.
The factor 2 needs no more room because no chain of the kernels is longer than the sequential one (k64_rows
P / 64 terms per lane, k64_cols rows_per_chunk / 2 per chain, k64_reduce at most 1024 slabs); 2^-40 is about
8000 fp64 ulps, above any order effect at these lengths and five decimal orders below what one fp32-rounded
operand or scalar leaves (2^-24).  tests/test_f64_ref_host.py shows on the CPU that the rule lets two correct
fp64 evaluations through and rejects an fp32-rounded softplus parameter or dense B in every case.

The plan's max_slabs is min(1024, floor(2097152 / P)) at these sizes (16 MiB of slabs; the 2 % of X term is
smaller); tr_loss_grad_f64 takes nchunks = min(max_slabs, N), rows_per_chunk = ceil(N / nchunks), then
nchunks = ceil(N / rows_per_chunk).  test_cases_sit_on_their_branches asserts the arithmetic below.

   #  X shape                        rank  what it reaches
   1  (1, 8, 4)                         2  N = 1; P = 32 < 64, idle lanes; three of four waves own no row
   2  (7, 5, 3)                         1  P = 15, rank 1, N not a multiple of 4
 3-12 (37, P), P = 63 64 65 127 128     2  one feature mode (nf == 1 in k64_dense / k64_mttkrp); every edge of
      129 192 193 256 257                  k64_rows' 128-stride loop and tail; the 256-column block edge of
                                           k64_cols / k64_reduce
  13  (1027, 6, 7)                      4  max_slabs 1024: 2 rows per chunk, 514 chunks, the last of one row
                                           (odd tail); nd = 1028 > 256 partials in k64_reduce
  14  (2500, 5, 4, 3)                   5  3 rows per chunk, 834 chunks, the last of one row; three modes, a
                                           middle mode in the MTTKRP decode
  15  (4096, 3, 3)                      2  exactly one row per wave at the wave cap; 4 rows per chunk
  16  (4099, 3, 3)                      2  k64_rows' grid-stride (three waves take two rows); 5 rows per chunk,
                                           820 chunks, the last of 4
  17  (600, 41, 100)                    3  P = 4100: max_slabs 511 < N, 2 rows per chunk, 300 chunks; 17 column
                                           blocks, the last of 4 columns
  18  (7, 800, 700)                    50  nfelem 75000: k64_prep wraps its 65536-thread grid; P = 560000:
                                           k64_dense wraps its 524288-thread grid, max_slabs 3 (chunks of 3, 3,
                                           1); rank tiles 32 + 18
  19  (64, 10, 10)                     32  one full rank tile
  20  (64, 10, 10)                     33  a tile of 32 and a tile of 1
  21  (90, 10, 10)                     65  three tiles
  22  (257, 6, 7, 8, 3)                 5  four modes, `nother` 168 .. 336 on both sides of the 256 threads
  23  (20, 2, 3, 2, 3, 2, 3, 2, 3)      3  eight modes (TR_MAXF)
All run with softplus {'beta': 0.7, 'threshold': 1.3} (neither an fp32 number; the plan keeps an fp32 copy
beside the fp64 one), non_negative alternating over the modes; 1, 11, 12 and 17 also with the default
arguments (12 has no flagged factor: there the two runs must agree, and do).

Around the sweep: X as an overlapping / padded strided view (bitwise the contiguous result, and stride 0
restores the plan), bitwise reproducibility across runs and plans, the stop flag, the empty shard, two shards
summed under a common norm on a plan larger than either, argument errors, and one 25-step AMSGrad fit against
the oracle's fp64 fit_adam_linear (F64_RTOL, the bars of test_float64_golden) with its strided twin.

Largest measured e and the e_yard of the same array (MI355X; every case prints its own with -s):
                  largest e / its e_yard (case)            nearest its bound: e / e_yard (case), e / bound
  y_hat           7.17e-16 / 4.36e-15 (17, default softplus)  3.97e-16 / 2.42e-16 (13, stride P + 5)   0.29
  data loss       2.92e-16 / 7.15e-17 (1, default softplus)   the same                                 0.28
  total loss      2.60e-16 / 6.44e-17 (1, default softplus)   the same                                 0.26
  factor grads    1.54e-15 / 3.91e-16 (13, factor 0)          the same                                 0.92
  bias gradient   1.49e-15 / 7.34e-16 (21)                    the same                                 0.63
The kernels are as accurate as numpy's pairwise / BLAS order on the host and mostly better than the
sequential chain.  Where e exceeds e_yard it stays inside the 2^-50 floor's room: the scalars of case 1 are
two roundings of a one-term sum, and case 13's first factor gradient passes through k64_reduce's chain of 514
slabs, half as long as the yardstick's 1027-term chain, whose error on that factor happens to be small
(3.9e-16 where it has 1.3e-15 on the other factor).  Case 18, the largest, sits at 9.0e-16 / 3.2e-15 on its
first factor's gradient (0.13 of the bound).  No case needs more than the factor 2.  The whole
module takes 5 s, its longest test (the three fits) 1.6 s, the largest sweep case (18, 31 MB of X) 0.4 s.

No kernel defect was found with this module: every test passes on tr_fp64.hip / tr_api.hip as they were.
That the module would notice one was checked once with six deliberately wrong builds of tr_fp64.hip, each
of which fails it: softplus parameters rounded to fp32 (every case with a flagged factor at (0.7, 1.3)),
k64_rows' tail dropping its last column (P = 32, 15, 63, 64, 129, 192, 257, ... and not 65, 127, 128, 193, 256),
k64_reduce's partial loop not wrapping (the cases with N > 256), k64_dense ignoring modes past the third
(cases 22 and 23 alone), k64_cols dropping the odd tail row of the last chunk, and k64_mttkrp losing the
fourth wave's partial beyond the first rank tile (case 18 alone).
"""
import numpy as np
import pytest
import torch

import f64_ref as fr
from golden_util import normwise_rel

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F64_RTOL = 1e-10  # test_gpu_parity.py's bar for the float64 path
SENT = -1234.5
TR_E_ARG = -1  # include/tensor_regression_hip.h
CASE_IDS = [f"case{c}-{s}" for c, s in fr.SWEEP]

# case -> (max_slabs, rows per chunk, chunks, rows of the last chunk)
CHUNKS = {1: (1024, 1, 1, 1), 2: (1024, 1, 7, 1), 13: (1024, 2, 514, 1), 14: (1024, 3, 834, 1),
          15: (1024, 4, 1024, 4), 16: (1024, 5, 820, 4), 17: (511, 2, 300, 2), 18: (3, 3, 3, 1)}


def dev(a, dtype=torch.float64):
    return torch.tensor(np.asarray(a), dtype=dtype, device=DEV)


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return np.ascontiguousarray(x).view(np.int64 if x.dtype.itemsize == 8 else np.int32).copy()


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def strided_view(base_dev, shape, row_stride):
    return torch.as_strided(base_dev, tuple(shape), (row_stride,) + tuple(torch.empty(shape[1:]).stride()))


class Session:
    """A model and its float64 plan for one draw, and one evaluation of everything the plan writes."""

    def __init__(self, inp, max_rows=None, fresh_factors=False):
        from tensor_regression_amd import CP_linear_regression
        self.inp = inp
        Bcp = [dev(A).requires_grad_(fresh_factors) for A in inp["Bcp"]]
        self.model = CP_linear_regression(inp["shape"], dtype=torch.float64, rank=inp["rank"],
                                          non_negative=list(inp["nn"]), weights=inp["w"], Bcp_init=Bcp,
                                          bias_init=inp["bias"], device=DEV, softplus_kwargs=dict(inp["sp"]))
        self.X = dev(inp["X"])
        self.y = dev(inp["y"])
        self.N = inp["shape"][0]
        self.plan = self.model._get_plan(self.X, self.N if max_rows is None else max_rows)
        assert "float64" in self.plan.describe and "path=2pass-f64-valu" in self.plan.describe, self.plan.describe
        self.arena = self.plan.pack(self.model.Bcp, self.model.bias)
        self.w = self.model.weights

    def loss_grad(self, X=None, y=None, norm=None, stop=None, fill=float("nan")):
        """(gradient arena, yhat) of one loss_grad, both prefilled with `fill`."""
        X = self.X if X is None else X
        y = self.y if y is None else y
        p = self.plan
        grad = torch.full((p.num_grads,), fill, dtype=torch.float64, device=DEV)
        yhat = torch.full((X.shape[0],), fill, dtype=torch.float64, device=DEV)
        p.loss_grad(X, y, None, float(self.N if norm is None else norm), self.arena, self.w, grad, yhat=yhat, stop=stop)
        return grad, yhat

    def run(self, X=None):
        """loss_grad + finalize_grad + forward; `raw`: every device array written, for bitwise comparisons."""
        X = self.X if X is None else X
        p = self.plan
        grad, yhat = self.loss_grad(X)
        gtot = torch.full((p.num_params,), float("nan"), dtype=torch.float64, device=DEV)
        loss = torch.full((1,), float("nan"), dtype=torch.float64, device=DEV)
        p.finalize_grad(self.arena, grad, self.inp["lam"], gtot, loss)
        fwd = p.forward(X, self.arena, self.w)
        torch.cuda.synchronize()
        g = grad.cpu().numpy()
        got = {"y_hat": fwd.cpu().numpy(), "y_hat_loss_grad": yhat.cpu().numpy(), "data_loss": g[p.num_params],
               "loss": loss.cpu().numpy()[0], "grads": [v.cpu().numpy() for v in p.factor_views(gtot)],
               "bias_grad": gtot.cpu().numpy()[-1], "status": g[p.num_params + 1],
               "data_grads": [v.cpu().numpy() for v in p.factor_views(grad[:p.num_params])],
               "data_bias_grad": g[p.num_params - 1]}
        raw = {"grad": grad, "yhat": yhat, "gtot": gtot, "loss": loss, "fwd": fwd}
        return got, raw


@pytest.fixture
def session():
    """Session factory: every plan made through it is destroyed when the test ends, passed or failed."""
    made = []

    def make(*args, **kwargs):
        made.append(Session(*args, **kwargs))
        return made[-1]

    yield make
    for s in made:
        for plan in (s.plan, s.model._plan):  # (a fit may have replaced the model's plan; destroy is idempotent)
            if plan is not None:
                plan.destroy()


def assert_rule(tag, got, ref, yard, shape):
    bad, _ = fr.check(tag, got, ref, yard, shape)
    b2, _ = fr.check(tag + " (loss_grad)", dict(got, y_hat=got["y_hat_loss_grad"]), ref, yard, shape, keys=("y_hat",))
    assert not bad + b2, (tag, bad + b2)
    assert got["status"] == 0.0                                  # the status slot, exactly
    assert same_bits(got["y_hat"], got["y_hat_loss_grad"])        # one instruction sequence in both k64_rows


def test_cases_sit_on_their_branches(session):
    """max_slabs from the plan, the chunk arithmetic of tr_loss_grad_f64 from it: the table's claims."""
    for case, (ms, rpc, nchunks, last) in CHUNKS.items():
        shape, rank = fr.CASES[case]
        N, P = shape[0], int(np.prod(shape[1:]))
        s = session(dict(fr.make_inputs(case), X=np.zeros((1,) + shape[1:])), max_rows=N)
        got_ms = int(s.plan.describe.split("max_slabs=")[1].split()[0])
        assert got_ms == ms == min(1024, 2097152 // P), (case, s.plan.describe)
        k = min(got_ms, N)
        r = -(-N // k)
        k = -(-N // r)
        assert (r, k, N - (k - 1) * r) == (rpc, nchunks, last), (case, r, k)
    assert -(-4100 // 256) == 17 and 4100 % 256 == 4
    assert 75000 > 256 * 256 and 560000 > 2048 * 256           # k64_prep's and k64_dense's grids wrap
    assert 4 * -(-1027 // 4) == 1028                            # nd of case 13


# ---- 4. the sweep --------------------------------------------------------------------------

@pytest.mark.parametrize("case,sp", fr.SWEEP, ids=CASE_IDS)
def test_sweep_vs_longdouble(case, sp, session):
    inp, ref, yard = fr.reference_of(case, sp)
    s = session(inp)
    got, _ = s.run()
    assert_rule(f"case {case} {sp}", got, ref, yard, inp["shape"])


# ---- 5. behaviour around the sweep -----------------------------------------------------------

@pytest.mark.parametrize("pad", [5, -3])
@pytest.mark.parametrize("case", [13, 2])
def test_strided_rows_are_bitwise_the_contiguous_result(case, pad, session):
    """Rows P + pad doubles apart in a 1-D base (pad < 0: overlapping windows), then the contiguous copy on the
    same plan: tr_plan_set_x_stride's re-run of the fp32 strategy choosers leaves a float64 plan as it was."""
    inp, ref, yard = fr.reference_of(case, "odd", pad)
    s = session(inp)
    desc0 = s.plan.describe
    base = dev(inp["base"])
    Xv = strided_view(base, inp["shape"], inp["row_stride"])
    assert Xv.stride(0) == int(np.prod(inp["shape"][1:])) + pad and not Xv.is_contiguous()
    assert np.array_equal(Xv.cpu().numpy(), inp["X"])
    got_v, raw_v = s.run(Xv)
    assert s.plan._xstride == inp["row_stride"]
    assert "path=2pass-f64-valu" in s.plan.describe and s.plan.describe == desc0
    got_c, raw_c = s.run()                      # stride 0 again
    assert s.plan._xstride == 0 and s.plan.describe == desc0
    for k in raw_v:
        assert same_bits(raw_v[k], raw_c[k]), k
    assert_rule(f"case {case} stride P{pad:+d}", got_v, ref, yard, inp["shape"])
    assert_rule(f"case {case} contiguous after stride", got_c, ref, yard, inp["shape"])


@pytest.mark.parametrize("case", [14, 18])
def test_bitwise_reproducible_across_runs_and_plans(case, session):
    """"Every reduction is a fixed-order tree": twice on one plan and once on a fresh one."""
    inp, _, _ = fr.reference_of(case, "odd")
    s = session(inp)
    _, a = s.run()
    _, b = s.run()
    s2 = session(inp)
    assert s2.plan.h.value != s.plan.h.value
    _, c = s2.run()
    for k in a:
        assert same_bits(a[k], b[k]) and same_bits(a[k], c[k]), k
    assert np.isfinite(a["grad"].cpu().numpy()).all()


@pytest.mark.parametrize("case", [2, 13])
def test_stop_flag(case, session):
    inp, _, _ = fr.reference_of(case, "odd")
    s = session(inp)
    grad0, yhat0 = s.loss_grad()
    assert np.isfinite(grad0.cpu().numpy()).all() and np.isfinite(yhat0.cpu().numpy()).all()
    grad1, yhat1 = s.loss_grad(stop=torch.ones(1, dtype=torch.int32, device=DEV), fill=SENT)
    assert same_bits(grad1, np.full(grad1.shape[0], SENT)) and same_bits(yhat1, np.full(yhat1.shape[0], SENT))
    grad2, yhat2 = s.loss_grad(stop=torch.zeros(1, dtype=torch.int32, device=DEV), fill=SENT)
    assert same_bits(grad2, grad0) and same_bits(yhat2, yhat0)


def test_empty_shard_writes_zeros(session):
    inp, _, _ = fr.reference_of(2, "odd")
    s = session(inp)
    grad, _ = s.loss_grad(X=s.X[:0], y=s.y[:0])
    assert grad.shape[0] == s.plan.num_grads and same_bits(grad, np.zeros(s.plan.num_grads))


@pytest.mark.parametrize("cut", [1000, 2499])
def test_two_shards_sum_to_the_full_problem(cut, session):
    """Case 14 cut in two, each shard with norm = 2500 on the plan built for 2500 rows (max_rows > n_rows):
    the summed arenas (data loss, bias gradient, factor gradients before the penalty) against the full problem."""
    inp, ref, yard = fr.reference_of(14, "odd")
    s = session(inp)
    N = s.N
    ga, ya = s.loss_grad(X=s.X[:cut], y=s.y[:cut], norm=N)
    gb, yb = s.loss_grad(X=s.X[cut:], y=s.y[cut:], norm=N)
    p = s.plan
    tot = (ga + gb).cpu().numpy()
    got = {"y_hat": np.concatenate([ya.cpu().numpy(), yb.cpu().numpy()]), "data_loss": tot[p.num_params],
           "bias_grad": tot[p.num_params - 1],
           "data_grads": [v.cpu().numpy() for v in p.factor_views(dev(tot[:p.num_params]))]}
    bad, _ = fr.check(f"case 14 shards {cut}+{N - cut}", got, ref, yard, inp["shape"],
                      keys=("y_hat", "data_loss", "data_grads", "bias_grad"))
    assert not bad, bad
    assert tot[p.num_params + 1] == 0.0


def test_argument_errors(session):
    from tensor_regression_amd import _engine, _lib
    inp, _, _ = fr.reference_of(2, "odd")
    s = session(inp)
    p = s.plan
    N = s.N
    grad = torch.zeros(p.num_grads, dtype=torch.float64, device=DEV)
    X8 = torch.zeros((N + 1,) + tuple(inp["shape"][1:]), dtype=torch.float64, device=DEV)
    y8 = torch.zeros(N + 1, dtype=torch.float64, device=DEV)
    with pytest.raises(ValueError, match="max_rows"):
        p.loss_grad(X8, y8, None, float(N + 1), s.arena, s.w, grad)
    for norm in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match="norm"):
            p.loss_grad(s.X, s.y, None, norm, s.arena, s.w, grad)
    assert same_bits(grad, np.zeros(p.num_grads))
    # the fp32 entry points on a float64 plan, and the reverse: TR_E_ARG before any launch
    lib, ptr, st = p.lib, _lib.ptr, _engine.stream_handle(p.dev)
    p32 = _engine.Plan(_lib.TR_MODEL_LINEAR, inp["shape"][1:], 1, inp["rank"], N, inp["nn"], dict(inp["sp"]), DEV)
    try:
        buf = torch.zeros(4 * p.num_grads + N, dtype=torch.float64, device=DEV)  # large enough in either type
        hp = (1e-3, 0.9, 0.999, 1e-8, 0.0, 0, 1)
        for plan, sfx, msg in ((p, "", "float64 plan"), (p32, "_f64", "needs a float64 plan")):
            cw = () if sfx else (None,)
            calls = {
                "tr_forward": lambda f: f(plan.h, ptr(s.X), N, ptr(buf), ptr(buf), ptr(buf), st),
                "tr_loss_grad": lambda f: f(plan.h, ptr(s.X), N, ptr(s.y), *cw, float(N), ptr(buf), ptr(buf), ptr(buf),
                                            None, None, st),
                "tr_finalize_grad": lambda f: f(plan.h, ptr(buf), ptr(buf), 0.01, ptr(buf), ptr(buf), st),
                "tr_adam_step": lambda f: f(plan.h, ptr(buf), ptr(buf), ptr(buf), ptr(buf), None, 0.01, *hp, None, 0, 0, 10,
                                            0.0, None, st),
            }
            for name, call in calls.items():
                rc = call(getattr(lib, name + sfx))
                assert rc == TR_E_ARG, (name + sfx, rc)
                assert msg in lib.tr_last_error().decode(), (name + sfx, lib.tr_last_error())
        torch.cuda.synchronize()
        assert same_bits(buf, np.zeros(buf.shape[0]))
    finally:
        p32.destroy()


# ---- 6. one trajectory beyond the fixtures ---------------------------------------------------

ADAM = {'lr': 0.02, 'amsgrad': True, 'weight_decay': 0.01}
FIT_NN = (True, False, True)


def _fit(session, inp, X, iters):
    s = session(inp, fresh_factors=True)
    conv = s.model.fit_Adam(X, s.y, lambda_L2=inp["lam"], max_iter=iters, tol=0, patience=10, Adam_kwargs=dict(ADAM))
    assert "float64" in s.model._plan.describe and not conv
    return s.model


def test_adam_trajectory_vs_oracle_and_its_strided_twin(session):
    """Case 14's shape, softplus (0.7, 1.3) on the outer modes, 25 AMSGrad steps with weight decay against the
    oracle's fp64 fit on the CPU; then 10 steps on the stride-(P - 3) view of that X, bitwise the contiguous fit."""
    from oracle import cp_oracle
    inp = fr.make_inputs(14, "odd", pad=-3, non_negative=FIT_NN)
    ref = cp_oracle.fit_adam_linear(inp["X"], inp["y"], inp["Bcp"], inp["bias"], inp["w"], list(FIT_NN), inp["lam"], 25,
                                    0, 10, dict(ADAM), dict(inp["sp"]), dtype=torch.float64)
    m = _fit(session, inp, dev(inp["X"]), 25)
    assert len(m.loss_running) == 25 and m.Bcp[0].dtype == torch.float64
    np.testing.assert_allclose(m.loss_running, ref["loss_running"], rtol=F64_RTOL)
    for A, B in zip(m.Bcp, ref["Bcp"]):
        assert normwise_rel(A.detach().cpu().numpy(), B) <= 100 * F64_RTOL
    assert abs(m.bias.item() - float(ref["bias"][0])) <= 100 * F64_RTOL
    base = dev(inp["base"])
    Xv = strided_view(base, inp["shape"], inp["row_stride"])
    assert Xv.stride(0) == 57 and np.array_equal(Xv.cpu().numpy(), inp["X"])
    mv = _fit(session, inp, Xv, 10)
    mc = _fit(session, inp, dev(inp["X"]), 10)
    assert mv._plan._xstride == 57 and getattr(mc._plan, "_xstride", 0) == 0
    assert same_bits(np.array(mv.loss_running), np.array(mc.loss_running)) and len(mv.loss_running) == 10
    for A, B in zip(mv.Bcp + [mv.bias], mc.Bcp + [mc.bias]):
        assert same_bits(A, B)
    assert np.allclose(mc.loss_running, ref["loss_running"][:10], rtol=F64_RTOL, atol=0)
