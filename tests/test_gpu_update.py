"""GPU checks of the update step: tr_finalize_grad / tr_adam_step called directly with chosen inputs
(k_update, k64_update, and both instantiations of k_update_conv, the one update kernel of the conv,
phase and Fourier plans; k_converge and k_converge_tail behind them).

No X is ever passed: the test writes the gradient arena itself (random data gradients, the data loss,
the status slot) and reads back parameters, Adam state, loss history and stop flag.

  * step parity at arenas around the 1024-thread stride of the update loops, three hyperparameter
    sets, steps 1 .. 100000, against tests/update_ref.py: the penalty gradient by fp64 autograd and
    the header's Adam formulas in fp64.  Per array (params, m, v, vmax, and finalize_grad's total
    gradient), e = max_i |got_i - ref_i| / (|ref_i| + rms(ref)) must satisfy
        e <= 2 * e_torch32 + 2^-22
    where e_torch32 is the same measure of torch.optim.Adam on the CPU in fp32 (foreach=False, state
    preloaded, penalty by fp32 autograd): the factor 2 covers another summation order in the norms,
    the floor is a few fp32 ulps for cases where torch happens to be exact.  The f64 plan uses the
    same rule with a 2^-50 floor, torch.optim.Adam in fp64 as the yardstick and a reference evaluated
    in numpy.longdouble (x87 extended, eps 2^-63; the module asserts that longdouble is wider than
    double and falls back to a 16-ulp fp64 bound against the fp64 reference where it is not).
  * the loss record (exactly an fp32 value, within 4 fp32 ulps of the fp64 total), untouched
    history / gradient arena / vmax, softplus flags without effect on the update
  * the three stop rules (flag already set, status slot, NaN data loss) with bitwise no-ops
  * the plateau sum on the device against np.sum(np.abs(np.diff(...))) at tol = d and nextafter(d),
    at lengths on both sides of every branch of numpy's pairwise order; k_converge_tail's slices

Conv, phase and Fourier plans need max_series_rows >= the temporal window, so they are created with
max_rows = W; every other plan with max_rows = 1.  The Fourier cases run with the spectrum penalty off
(its value in the total is covered by the cfs_* fixtures of test_gpu_fourier.py).  A phase plan and a
Fourier plan with one component are the same update and must agree bitwise.  With hist_base = 37 the plateau lengths below 37
do not exist (the patience would be negative) and are run at hist_base = 0 only.

Largest measured e / e_torch of the same case, per plan family (MI355X; printed by every case with -s):
              params             m                  v                  vmax               finalize_grad
  linear      3.68e-7 / 3.68e-7  2.20e-7 / 3.73e-8  1.66e-7 / 1.66e-7  1.66e-7 / 1.66e-7  4.02e-8 / 4.02e-8
  multinomial 1.48e-7 / 1.48e-7  1.81e-7 / 3.84e-8  1.76e-7 / 1.76e-7  1.59e-7 / 1.59e-7  3.84e-8 / 3.84e-8
  spectral    1.67e-7 / 1.67e-7  2.70e-7 / 2.70e-7  1.85e-7 / 1.85e-7  1.58e-7 / 1.58e-7  3.97e-8 / 3.97e-8
  conv        2.50e-7 / 2.50e-7  2.67e-7 / 2.67e-7  1.83e-7 / 1.83e-7  1.83e-7 / 1.83e-7  3.89e-8 / 3.89e-8
  phase       2.46e-7 / 2.46e-7  4.17e-7 / 3.32e-7  5.00e-7 / 3.81e-7  3.75e-7 / 2.99e-7  4.29e-7 / 3.28e-7
  f64         7.01e-15 / 7.01e-15  3.82e-16 / 8.06e-17  3.30e-16 / 3.30e-16  2.86e-16 / 2.86e-16  8.06e-17 / 8.06e-17
The kernels mostly reproduce torch's own fp32 result (e = e_torch); the phase maxima are the order-8
smoothness stencil.  The one place they differ visibly is m at betas[0] = 0 (set 3, t = 100000): torch's
lerp takes its other branch for a weight >= 0.5 (end - (end - start) * (1 - weight), exact at weight 1),
the kernels always start + weight * (end - start), within one rounding of m: 2.2e-7 where torch has 3.7e-8,
inside the bound (3.1e-7) through its floor.  The longest case, the 100000-term plateau sum, takes 0.10 s.

Found with this module and fixed with it: beyond 8192 terms np.sum is not one pairwise sum (numpy reduces
8192 elements at a time and adds the chunk sums one after another), which np_pairwise_sum_absdiff did not
follow; the lengths 8193, 20000 and 100000 below fail on the earlier kernel.
"""
import functools

import numpy as np
import pytest
import torch

import update_ref as ur

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
SENT = -1234.5  # history sentinel
FLOOR32, FLOOR64 = 2.0 ** -22, 2.0 ** -50
LONGDOUBLE = np.finfo(np.longdouble).eps < np.finfo(np.float64).eps

HP = {
    1: ur.hparams(),
    2: ur.hparams(lr=0.02, beta1=0.8, beta2=0.99, eps=1e-6, weight_decay=0.01, amsgrad=True),
    3: ur.hparams(beta1=0.0, beta2=0.5, amsgrad=True),
}
STEPS = {1: (1, 2, 1000), 2: (1, 7, 1000), 3: (100000,)}

# name -> (kind, plan arguments, intended num_params)
ARENAS = {
    "lin_17": ("linear", ((5, 3), 2), 17),
    "lin_1024": ("linear", ((31, 2), 31), 1024),
    "lin_1025": ("linear", ((64, 64), 8), 1025),
    "lin_2048": ("linear", ((20, 3), 89), 2048),
    "lin_2049": ("linear", ((128, 128), 8), 2049),
    "lin_3073": ("linear", ((256, 128), 8), 3073),
    "lin_7modes": ("linear", ((3, 5, 2, 7, 4, 6, 9), 37), 1333),
    "mnl_8factors": ("multinomial", ((3, 5, 2, 7, 4, 6, 2), 9, 37), 1406),
    "spec_2831": ("spectral", (256, 33, 5, 4, 3, 2), 2831),
    "spec_small": ("spectral", (40, 17, 3, 3, 2, 2), 40 * 3 + 17 * 3 + 3 * 3 + 40 * 2 * 2 + 17 * 2 + 3 * 2 + 3),
    "conv_2413": ("conv", (65, 300, 4, 3, 3, 2), 2413),
    "conv_rn0": ("conv", (9, 400, 2, 0, 3, 1), 1235),
    "conv_rs0": ("conv", (9, 400, 2, 3, 0, 1), 1235),
    "phase_2218_q0": ("phase", (65, 300, 4, 3, 3, 0), 2218),
    "phase_2218_q2": ("phase", (65, 300, 4, 3, 3, 2), 2218),
    "phase_2218_q8": ("phase", (65, 300, 4, 3, 3, 8), 2218),
    "phase_rn0_q0": ("phase", (9, 400, 2, 0, 3, 0), 1235),
    "phase_rn0_q2": ("phase", (9, 400, 2, 0, 3, 2), 1235),
    "phase_rn0_q8": ("phase", (9, 400, 2, 0, 3, 8), 1235),
    "f64_1025": ("f64", ((64, 64), 8), 1025),
    "f64_2049": ("f64", ((128, 128), 8), 2049),
    "f64_7modes": ("f64", ((3, 5, 2, 7, 4, 6, 9), 37), 1333),
    # (W, D, N, Rn, Rs, C, q); appended: a case's index seeds its inputs
    "fourier_c2_q0": ("fourier", (65, 300, 4, 3, 3, 2, 0), 2413),
    "fourier_c2_q2": ("fourier", (65, 300, 4, 3, 3, 2, 2), 2413),
    "fourier_c2_q8": ("fourier", (65, 300, 4, 3, 3, 2, 8), 2413),
    "fourier_rn0_q2": ("fourier", (9, 400, 2, 0, 3, 2, 2), 9 * 6 + 400 * 3 + 2 * 3 + 2),
}
# one small and one > 1024 arena per plan kind for the stop rules
STOP_ARENAS = ["lin_17", "lin_2049", "mnl_small", "mnl_8factors", "spec_small", "spec_2831", "conv_small",
               "conv_2413", "phase_small", "phase_2218_q2", "fourier_small", "fourier_c2_q2", "f64_small", "f64_2049"]
ARENAS_EXTRA = {
    "mnl_small": ("multinomial", ((5, 3), 4, 2), 24),
    "conv_small": ("conv", (9, 5, 2, 1, 1, 2), 5 * 2 + 2 * 2 + 9 + 18 + 2),
    "phase_small": ("phase", (9, 5, 2, 1, 1, 2), 5 * 2 + 2 * 2 + 9 + 9 + 2),
    "fourier_small": ("fourier", (9, 5, 2, 1, 1, 2, 2), 5 * 2 + 2 * 2 + 9 + 18 + 2),
    "fourier_c1_q2": ("fourier", (65, 300, 4, 3, 3, 1, 2), 2218),  # phase_2218_q2's arena
    "f64_small": ("f64", ((5, 3), 2), 17),
}
# the largest Delta^q scratch of each family, 265 x 32 and 265 x 64 floats (67,840 B: past 64 KiB); one
# hyperparameter set each
LDS_MAX = {
    "phase_lds_max": ("phase", (257, 3, 1, 16, 16, 8), 3 * 32 + 32 + 257 * 16 + 257 * 16 + 1),
    "fourier_lds_max": ("fourier", (257, 3, 1, 0, 16, 4, 8), 3 * 16 + 16 + 257 * 64 + 1),
}
LAM_L2 = 0.03
LAM_CONV = (0.02, 0.05, 0.11)  # (w, d, out)
LAM_SMOOTH = 0.05


class Arena:
    """A plan, its layout (checked against the intended total) and the fp64 penalty of its family."""

    def __init__(self, name, flags=False):
        from tensor_regression_amd import _engine, _lib
        kind, a, total = {**ARENAS, **ARENAS_EXTRA, **LDS_MAX}[name]
        self.name, self.kind = name, kind
        self.smooth = None
        if kind in ("linear", "f64", "multinomial"):
            dims, rank = a[0], a[-1]
            ncls = a[1] if kind == "multinomial" else 1
            nf = len(dims) + (kind == "multinomial")
            nn = [bool(flags and f % 2 == 0) for f in range(nf)]
            model = _lib.TR_MODEL_MULTINOMIAL if kind == "multinomial" else _lib.TR_MODEL_LINEAR
            self.plan = _engine.Plan(model, dims, ncls, rank, 1, nn, None, DEV,
                                     dtype=torch.float64 if kind == "f64" else torch.float32)
            self.n_bias = 0 if kind == "multinomial" else 1
            self.lam, pk = LAM_L2, "l2"
        else:
            nn = [bool(flags), False, bool(flags)]
            if kind == "spectral":
                self.plan = _engine.SpectralPlan(*a, 1, nn, None, DEV)
                self.lam, pk = LAM_L2, "l2"
            elif kind == "conv":
                self.plan = _engine.ConvPlan(*a, a[0], nn, None, DEV)
                self.lam, pk = LAM_CONV, "conv"
            elif kind == "phase":
                self.smooth = (LAM_SMOOTH, a[5])
                self.plan = _engine.ConvPhasePlan(*a[:5], a[0], nn, None, DEV, *self.smooth)
                self.lam, pk = LAM_CONV, "phase"
            else:
                self.smooth = (LAM_SMOOTH, a[6])
                self.plan = _engine.ConvFourierPlan(*a[:6], a[0], nn, None, DEV, *self.smooth)
                self.lam, pk = LAM_CONV, "fourier"
            self.n_bias = a[2]
        p = self.plan
        self.shapes = [tuple(s) for s in p.factor_shapes()]
        nf = len(self.shapes)
        self.off = list(p.offsets[:nf + 1])
        self.np = p.num_params
        # the layout the cases were chosen for: every offset from the plan, the total as intended
        assert self.off[0] == 0
        for f, shp in enumerate(self.shapes):
            assert self.off[f + 1] - self.off[f] == int(np.prod(shp)), (name, f)
        self.nfe = self.off[nf]
        assert self.nfe + self.n_bias == self.np == total, (name, self.nfe, self.n_bias, self.np, total)
        assert p.num_grads == self.np + 2
        self.dtype = p.dtype
        self.npdt = np.float64 if kind == "f64" else np.float32

    def penalty(self, lam=None, smooth=None):
        lam = self.lam if lam is None else lam
        sm = self.smooth if smooth is None else smooth
        if self.kind in ("conv", "phase", "fourier"):
            return ur.make_penalty(self.kind, self.off, self.shapes, list(lam), *(sm or ()))
        return ur.make_penalty("l2", self.off, self.shapes, lam)


@functools.lru_cache(maxsize=None)
def arena_of(name, flags=False):
    return Arena(name, flags)


def test_layouts_hit_the_intended_boundaries():
    """The boundary cases are what the table says: a typo in a shape cannot move one silently."""
    a = arena_of("lin_1025")
    assert a.nfe == 1024 and a.np == 1025          # bias alone in the second slot of thread 0's trip
    a = arena_of("lin_2049")
    assert a.nfe == 2048 and a.np == 2049          # bias alone in the tail loop
    a = arena_of("lin_7modes")
    assert len(a.shapes) == 7 and any(a.off[f] < 1024 < a.off[f + 1] - 1 for f in range(7))  # one factor straddles
    a = arena_of("mnl_8factors")
    assert len(a.shapes) == 8 and a.n_bias == 0    # TR_MAXF
    a = arena_of("spec_2831")
    assert a.n_bias == 5 and a.nfe == 2826
    for n in ("conv_rn0", "conv_rs0", "phase_rn0_q2", "fourier_rn0_q2"):
        a = arena_of(n)
        assert a.np > 1024 and any(int(np.prod(s)) == 0 for s in a.shapes)
    assert arena_of("fourier_c2_q2").np > 2048     # past two trips of the 1024-thread loop
    for n, cols in (("phase_lds_max", 32), ("fourier_lds_max", 64)):  # Delta^q: (W + q) x (Rn + RsK) floats
        a = arena_of(n)
        assert (a.shapes[2][0] + a.smooth[1]) * int(np.prod(a.shapes[2][1:]) + np.prod(a.shapes[3][1:])) == 265 * cols


# ---- synthetic inputs ----------------------------------------------------------------------

def _mag(rng, n):
    """signed magnitudes spread over 1e-4 .. 1"""
    return rng.choice([-1.0, 1.0], n) * 10.0 ** rng.uniform(-4, 0, n)


def make_inputs(a, rng, zero_state, hp):
    """Host inputs in the plan's dtype: params, gradient arena (data gradients, loss, status 0), m, v, vmax."""
    dt = a.npdt
    P = a.np
    params = (0.5 * rng.standard_normal(P)).astype(dt)
    grad = np.zeros(P + 2, dt)
    grad[:P] = _mag(rng, P).astype(dt)
    grad[P] = dt(rng.uniform(0.5, 2.0))
    if zero_state:
        m, v, vmax = np.zeros(P, dt), np.zeros(P, dt), np.zeros(P, dt)
    else:
        m = _mag(rng, P).astype(dt)
        v = (_mag(rng, P) ** 2).astype(dt)
        # about half of vmax above the new v and half below: both sides of the max decide a denominator
        g64, _ = ur.total_grad(params, grad[:P], float(grad[P]), a.penalty())
        g64 = g64 + hp["weight_decay"] * params.astype(np.float64)
        vnew = hp["beta2"] * v.astype(np.float64) + (1.0 - hp["beta2"]) * g64 * g64
        vmax = (vnew * np.where(rng.random(P) < 0.5, 1.5, 0.5)).astype(dt)
    return dict(params=params, grad=grad, m=m, v=v, vmax=vmax)


def to_dev(inp):
    return {k: torch.tensor(x, device=DEV) for k, x in inp.items()}


def bits(x):
    x = x.detach().cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)
    return x.view(np.int64 if x.dtype.itemsize == 8 else np.int32).copy()


def same_bits(x, y):
    return np.array_equal(bits(x), bits(y))


def dev_step(a, d, hp, t, hist, hist_base=0, it=0, patience=10, tol=0.0, stop=None, lam=None):
    vmax = d["vmax"] if hp["amsgrad"] else None
    a.plan.adam_step(d["params"], d["grad"], d["m"], d["v"], vmax, a.lam if lam is None else lam, hp, t, hist,
                     hist_base, it, patience, tol, stop)


def new_hist(n):
    return torch.full((n,), SENT, dtype=torch.float64, device=DEV)


def new_stop(value=0):
    return torch.full((1,), value, dtype=torch.int32, device=DEV)


# ---- reference of one step -----------------------------------------------------------------

def reference_step(a, inp, hp, t, tadam=None):
    """(ref, yardstick): dicts of params / m / v / vmax / gtot / total; the yardstick is torch.optim.Adam in
    the plan's dtype (a TorchAdam carried over a chain when given)."""
    P = a.np
    pen = a.penalty()
    if a.kind == "f64" and LONGDOUBLE:
        g, total = ur.total_grad_longdouble(inp["params"], inp["grad"][:P], inp["grad"][P], a.off, len(a.shapes),
                                            a.lam)
        g64, total64 = ur.total_grad(inp["params"], inp["grad"][:P], float(inp["grad"][P]), pen)
        assert ur.err(g64, g.astype(np.float64)) < 1e-13 and abs(total64 - float(total)) < 1e-13 * abs(total64)
        ft = np.longdouble
    else:
        g, total = ur.total_grad(inp["params"], inp["grad"][:P], float(inp["grad"][P]), pen)
        ft = np.float64
    p, m, v, vmax = ur.adam_ref(inp["params"], g, inp["m"], inp["v"], inp["vmax"], hp, t, ft)
    ref = dict(params=p, m=m, v=v, vmax=vmax, gtot=g, total=total)
    if tadam is None:
        tadam = ur.TorchAdam(inp["params"], inp["m"], inp["v"], inp["vmax"], hp, t, pen, a.dtype)
    # the yardstick's total gradient: the same autograd in the plan's dtype
    gy, _ = ur.total_grad(inp["params"], inp["grad"][:P], float(inp["grad"][P]), pen, a.dtype)
    py, my, vy, vmy = tadam.step(inp["grad"][:P])
    return ref, dict(params=py, m=my, v=vy, vmax=vmy, gtot=gy)


def check_accuracy(a, tag, got, ref, yard, keys):
    floor = FLOOR64 if a.kind == "f64" else FLOOR32
    bad = []
    for k in keys:
        e, ey = ur.err(got[k], ref[k]), ur.err(yard[k], ref[k])
        if a.kind == "f64" and not LONGDOUBLE:
            bound = 16 * np.finfo(np.float64).eps
        else:
            bound = 2.0 * ey + floor
        print(f"{a.name} {tag} {k}: e {e:.3e} e_torch {ey:.3e} bound {bound:.3e}")
        if not e <= bound:
            bad.append((k, e, ey, bound))
    assert not bad, (a.name, tag, bad)


def check_loss_record(a, got, total):
    if a.kind == "f64":
        tol = 4 * np.spacing(abs(float(total)))
    else:
        assert float(np.float32(got)) == got, got  # exactly an fp32 value
        tol = 4 * float(np.spacing(np.float32(abs(float(total)))))
    assert abs(np.longdouble(got) - np.longdouble(total)) <= tol, (a.name, got, float(total), tol)


def run_case(a, rng, hp, t, hist_base=0, it=0, with_finalize=False, twin=None):
    """One device step on fresh inputs against the reference; `twin`: the same shape with other softplus
    flags, which must give bitwise the same update."""
    inp = make_inputs(a, rng, zero_state=(t == 1), hp=hp)
    ref, yard = reference_step(a, inp, hp, t)
    d = to_dev(inp)
    hist = new_hist(hist_base + it + 3)
    stop = new_stop()
    dev_step(a, d, hp, t, hist, hist_base, it, stop=stop)
    got = {k: d[k].cpu().numpy() for k in ("params", "m", "v", "vmax")}
    h = hist.cpu().numpy()
    keys = ["params", "m", "v"] + (["vmax"] if hp["amsgrad"] else [])
    check_accuracy(a, f"t={t}", got, ref, yard, keys)
    if not hp["amsgrad"]:
        assert same_bits(got["vmax"], inp["vmax"])  # AMSGrad off: vmax untouched
    assert same_bits(d["grad"], inp["grad"])        # the gradient arena is read only
    assert int(stop.item()) == 0
    check_loss_record(a, h[hist_base + it], ref["total"])
    rest = np.delete(h, hist_base + it)
    assert same_bits(rest, np.full(rest.shape, SENT))
    if twin is not None:
        d2 = to_dev(inp)
        hist2 = new_hist(hist_base + it + 3)
        dev_step(twin, d2, hp, t, hist2, hist_base, it, stop=new_stop())
        for k in ("params", "m", "v", "vmax"):
            assert same_bits(d2[k], d[k]), (a.name, "softplus flags changed the update", k)
        assert same_bits(hist2, hist)
    if with_finalize:
        d3 = to_dev(inp)
        gtot = torch.full((a.np,), float("nan"), dtype=a.dtype, device=DEV)
        loss = torch.full((1,), float("nan"), dtype=a.dtype, device=DEV)
        a.plan.finalize_grad(d3["params"], d3["grad"], a.lam, gtot, loss)
        check_accuracy(a, "finalize", dict(gtot=gtot.cpu().numpy()), ref, yard, ["gtot"])
        check_loss_record(a, float(loss.item()), ref["total"])
        assert same_bits(d3["params"], inp["params"]) and same_bits(d3["grad"], inp["grad"])


# ---- 2. step parity at the boundary arenas ---------------------------------------------------

@pytest.mark.parametrize("hpset", [1, 2, 3])
@pytest.mark.parametrize("name", list(ARENAS))
def test_step_parity(name, hpset):
    idx = list(ARENAS).index(name)
    flags = (idx + hpset) % 2 == 0  # half the cases run with softplus flags on some factors
    a = arena_of(name, flags)
    twin = arena_of(name, False) if flags else None
    rng = np.random.default_rng(1000 * idx + hpset)
    hp = HP[hpset]
    for j, t in enumerate(STEPS[hpset]):
        run_case(a, rng, hp, t, hist_base=(0, 4)[j % 2], it=(0, 3, 1)[j % 3], with_finalize=(j == 0), twin=twin)


@pytest.mark.parametrize("name", list(LDS_MAX))
def test_step_parity_at_the_largest_smoothness_scratch(name):
    a = arena_of(name)
    run_case(a, np.random.default_rng(4000 + list(LDS_MAX).index(name)), HP[2], 7, hist_base=4, it=3,
             with_finalize=True)


def test_phase_and_one_component_fourier_agree_bitwise():
    """The phase plan and the Fourier plan with C = 1 have the same arena and the same update: one kernel,
    the same arguments.  Same bytes in, same bytes out, for the Adam step and for finalize_grad."""
    ph, fo = arena_of("phase_2218_q2"), arena_of("fourier_c1_q2")
    assert ph.off == fo.off and ph.np == fo.np and ph.smooth == fo.smooth and ph.lam == fo.lam
    hp = HP[2]
    inp = make_inputs(ph, np.random.default_rng(91), zero_state=False, hp=hp)
    out = []
    for a in (ph, fo):
        d = to_dev(inp)
        hist, stop = new_hist(8), new_stop()
        dev_step(a, d, hp, 7, hist, 4, 1, stop=stop)
        d2 = to_dev(inp)
        gtot = torch.full((a.np,), float("nan"), device=DEV)
        loss = torch.full((1,), float("nan"), device=DEV)
        a.plan.finalize_grad(d2["params"], d2["grad"], a.lam, gtot, loss)
        out.append(dict(params=d["params"], m=d["m"], v=d["v"], vmax=d["vmax"], hist=hist, stop=stop, gtot=gtot,
                        loss=loss))
    assert not same_bits(out[0]["params"], inp["params"]) and np.isfinite(out[0]["hist"][5].item())
    for k in out[0]:
        assert same_bits(out[0][k], out[1][k]), k


CHAIN = ["lin_2049", "mnl_8factors", "spec_2831", "conv_2413", "phase_2218_q2", "f64_2049", "fourier_c2_q2"]


@pytest.mark.parametrize("name", CHAIN)
def test_three_chained_steps(name):
    """Three device steps from zero state, fresh synthetic gradients each, against the chained reference."""
    a = arena_of(name)
    hp = HP[2]
    rng = np.random.default_rng(77 + CHAIN.index(name))
    inp = make_inputs(a, rng, zero_state=True, hp=hp)
    d = to_dev(inp)
    hist = new_hist(3)
    stop = new_stop()
    tadam = ur.TorchAdam(inp["params"], inp["m"], inp["v"], inp["vmax"], hp, 1, a.penalty(), a.dtype)
    cur = dict(inp)
    totals = []
    for it in range(3):
        P = a.np
        cur["grad"] = np.concatenate([_mag(rng, P), [rng.uniform(0.5, 2.0), 0.0]]).astype(a.npdt)
        d["grad"].copy_(torch.tensor(cur["grad"]))
        dev_step(a, d, hp, it + 1, hist, 0, it, stop=stop)
        ref, yard = reference_step(a, cur, hp, it + 1, tadam)
        totals.append(ref["total"])
        cur = dict(cur, params=ref["params"], m=ref["m"], v=ref["v"], vmax=ref["vmax"])  # chained at full precision
    got = {k: d[k].cpu().numpy() for k in ("params", "m", "v", "vmax")}
    check_accuracy(a, "chain3", got, ref, yard, ["params", "m", "v", "vmax"])
    assert int(stop.item()) == 0
    h = hist.cpu().numpy()
    # the first record belongs to the untouched parameters; later ones to device parameters that differ from
    # the reference's by the measured e (a few 1e-7 of the penalty): 1e-5 relative
    check_loss_record(a, h[0], totals[0])
    for it in (1, 2):
        assert abs(h[it] - float(totals[it])) <= 1e-5 * abs(float(totals[it]))


@pytest.mark.parametrize("name", ["lin_17", "conv_small", "phase_small", "spec_small"])
def test_all_zero_factor_gradient_is_nan_where_autograd_says(name):
    """lambda > 0 and a factor of zeros: sqrt backward at 0 times 0 is NaN on exactly that factor."""
    a = arena_of(name)
    rng = np.random.default_rng(5)
    inp = make_inputs(a, rng, zero_state=True, hp=HP[1])
    zf = len(a.shapes) - 1
    inp["params"][a.off[zf]:a.off[zf + 1]] = 0.0
    g32, total32 = ur.total_grad(inp["params"], inp["grad"][:a.np], float(inp["grad"][a.np]), a.penalty(),
                                 torch.float32)
    want = np.isnan(g32)
    assert want[a.off[zf]:a.off[zf + 1]].all() and want.sum() == a.off[zf + 1] - a.off[zf]
    d = to_dev(inp)
    gtot = torch.zeros(a.np, device=DEV)
    loss = torch.full((1,), float("nan"), device=DEV)
    a.plan.finalize_grad(d["params"], d["grad"], a.lam, gtot, loss)
    g = gtot.cpu().numpy()
    assert np.array_equal(np.isnan(g), want)
    assert np.isfinite(g[~want]).all()
    assert ur.err(g[~want], g32[~want].astype(np.float64)) < 1e-5
    assert np.isfinite(loss.item()) and abs(loss.item() - float(total32)) <= 1e-6 * abs(float(total32))
    assert same_bits(d["params"], inp["params"])


# ---- 3. stop rules -------------------------------------------------------------------------

def _stop_setup(name, seed=3):
    a = arena_of(name)
    hp = HP[2]
    inp = make_inputs(a, np.random.default_rng(seed), zero_state=False, hp=hp)
    return a, hp, inp


def _assert_untouched(d, inp, hist):
    for k in ("params", "m", "v", "vmax", "grad"):
        assert same_bits(d[k], inp[k]), k
    assert same_bits(hist, np.full(hist.shape[0], SENT))


@pytest.mark.parametrize("name", STOP_ARENAS)
def test_flag_already_set_is_a_no_op(name):
    a, hp, inp = _stop_setup(name)
    d = to_dev(inp)
    hist, stop = new_hist(8), new_stop(5)
    # iter > patience and tol = inf: a plateau launch that ignored the flag would overwrite it
    dev_step(a, d, hp, 4, hist, 0, 3, patience=1, tol=float("inf"), stop=stop)
    assert int(stop.item()) == 5
    _assert_untouched(d, inp, hist)


@pytest.mark.parametrize("status", [1.0, 2.0])
@pytest.mark.parametrize("name", STOP_ARENAS)
def test_status_slot_stops_before_the_step(name, status):
    from tensor_regression_amd import _lib
    a, hp, inp = _stop_setup(name)
    inp["grad"][a.np + 1] = status
    d = to_dev(inp)
    hist, stop = new_hist(8), new_stop()
    dev_step(a, d, hp, 4, hist, 0, 3, patience=1, tol=float("inf"), stop=stop)
    assert int(stop.item()) == _lib.TR_STOP_DEVICE_ERROR - 3
    _assert_untouched(d, inp, hist)


def _nan_step(a, hp, inp, hist_base, it, patience):
    d = to_dev(inp)
    hist, stop = new_hist(hist_base + it + 2), new_stop()
    dev_step(a, d, hp, it + 1, hist, hist_base, it, patience=patience, tol=0.0, stop=stop)
    h = hist.cpu().numpy()
    assert np.isnan(h[hist_base + it])
    rest = np.delete(h, hist_base + it)
    assert same_bits(rest, np.full(rest.shape, SENT))
    assert np.isfinite(d["params"].cpu().numpy()).all()  # only the loss was NaN: the step itself is applied
    assert not same_bits(d["params"], inp["params"])
    return int(stop.item())


@pytest.mark.parametrize("name", STOP_ARENAS)
def test_nan_data_loss(name):
    a, hp, inp = _stop_setup(name)
    inp["grad"][a.np] = np.nan
    pat = 6
    if a.kind in ("linear", "multinomial", "f64"):  # the reference's standard / multinomial fits have no NaN stop
        for hb, it in ((0, 0), (0, pat), (0, pat + 1), (4, 1)):
            assert _nan_step(a, hp, inp, hb, it, pat) == 0
    elif a.kind in ("spectral", "conv"):            # iter <= patience, whatever hist_base
        for hb in (0, 4):
            assert _nan_step(a, hp, inp, hb, 0, pat) == -1
            assert _nan_step(a, hp, inp, hb, pat, pat) == -(pat + 1)
            assert _nan_step(a, hp, inp, hb, pat + 1, pat) == 0
    else:                                           # phase, Fourier: hist_base + iter + 1 <= patience
        assert _nan_step(a, hp, inp, 0, pat - 1, pat) == -pat
        assert _nan_step(a, hp, inp, 0, pat, pat) == 0
        assert _nan_step(a, hp, inp, 4, 1, pat) == -2
        assert _nan_step(a, hp, inp, 4, 2, pat) == 0


# ---- 4. plateau sum on the device ----------------------------------------------------------

# (8192, 8193, 20000: on both sides of numpy's reduction buffer, see _np_sum_model)
LENGTHS = [1, 7, 8, 9, 15, 16, 127, 128, 129, 136, 255, 256, 257, 300, 1000, 4097, 8192, 8193, 20000, 100000]


def _halved(a, round8, cuts=None, base=0):
    """np.sum's recursion above 128 terms with the split n // 2 rounded down to a multiple of 8 (numpy's) or
    left as it is; the leaves (<= 128 terms) are numpy's own.  `cuts` collects the split positions."""
    n = len(a)
    if n <= 128:
        return np.sum(a)
    n2 = n // 2
    if round8:
        n2 -= n2 % 8
    if cuts is not None:
        cuts.append(base + n2)
    return _halved(a[:n2], round8, cuts, base) + _halved(a[n2:], round8, cuts, base + n2)


NP_BUF = 8192  # np.sum takes its operand in chunks of np.getbufsize() elements


def _np_sum_model(a, round8, cuts=None, buf=NP_BUF):
    """np.sum as numpy runs it: one _halved sum per chunk of `buf` elements, added one after another."""
    tot = -0.0
    for c in range(0, len(a), buf):
        tot = tot + _halved(a[c:c + buf], round8, cuts, c)
    return tot


def _history(n, min_diffs_checked, lo, hi):
    """h of n entries, standard_normal * 10^uniform(-6, 2) (the host test's distribution); when the checked
    slice h[lo:hi] has >= 8 diffs, the first seed at which np.sum of them differs from
      - a plain left-to-right sum,
      - up to 8192 terms: the sum with the recursion's splits not rounded to multiples of 8, where that
        moves a split,
      - beyond the 8192 terms that numpy reduces at a time: one pairwise sum over all of them,
    so a wrong summation order cannot pass."""
    for seed in range(200):
        rng = np.random.default_rng(seed)
        h = rng.standard_normal(n) * 10 ** rng.uniform(-6, 2)
        h[-1] = np.float64(np.float32(h[-1]))  # the step records an fp32 loss, widened
        dd = np.abs(np.diff(h[lo:hi]))
        if len(dd) < min_diffs_checked:
            return h, dd
        want = np.sum(dd)
        c8, c1 = [], []
        assert _np_sum_model(dd, True, c8) == want  # the order as this numpy runs it
        if np.cumsum(dd)[-1] == want:
            continue
        if len(dd) > NP_BUF:  # (the unrounded splits are left to the shorter lengths)
            if _halved(dd, True) != want:
                return h, dd
        elif _np_sum_model(dd, False, c1) != want or c8 == c1:
            return h, dd
    raise AssertionError("no seed separates the summation orders")


class _Plateau:
    """A plan whose step records exactly the data-loss slot: lambda = 0 (and no smoothness), zero gradients."""

    def __init__(self, name):
        self.a = a = arena_of(name)
        self.hp = HP[1]
        rng = np.random.default_rng(11)
        inp = dict(params=(0.5 * rng.standard_normal(a.np) + 0.1).astype(a.npdt), grad=np.zeros(a.np + 2, a.npdt),
                   m=np.zeros(a.np, a.npdt), v=np.zeros(a.np, a.npdt), vmax=np.zeros(a.np, a.npdt))
        self.d = to_dev(inp)
        self.params0 = inp["params"]
        self.lam = (0.0, 0.0, 0.0) if a.kind in ("conv", "phase", "fourier") else 0.0
        if a.kind in ("phase", "fourier"):
            a.plan.set_smoothness(0.0, 2)

    def close(self):
        if self.a.kind in ("phase", "fourier"):
            self.a.plan.set_smoothness(*self.a.smooth)

    def flag(self, h, hist_base, it, patience, tol):
        """The stop flag after one step whose loss is h[hist_base + it], on the history h[:hist_base + it]."""
        n = hist_base + it + 1
        assert len(h) == n
        hist = torch.tensor(h, dtype=torch.float64, device=DEV)
        hist[n - 1] = SENT  # the step writes this one
        loss = h[-1]
        self.d["grad"][self.a.np] = float(loss)
        stop = new_stop()
        dev_step(self.a, self.d, self.hp, 1, hist, hist_base, it, patience=patience, tol=tol, stop=stop, lam=self.lam)
        assert same_bits(hist, h), "the step must record exactly the loss slot and leave the history alone"
        return int(stop.item())


@pytest.fixture(scope="module")
def plateau_linear():
    p = _Plateau("lin_17")
    yield p
    assert same_bits(p.d["params"], p.params0)  # zero gradients, zero state: no step moved the parameters


def _check_k_converge(p, length, hist_base):
    patience = length - hist_base
    it = patience + 1
    n = hist_base + it + 1
    h, dd = _history(n, 8, it - patience, n)
    assert len(dd) == length
    if length >= 8:
        assert np.cumsum(dd)[-1] != np.sum(dd)
    dsum = np.sum(np.abs(np.diff(h[it - patience: hist_base + it + 1])))
    assert p.flag(h, hist_base, it, patience, dsum) == 0, (length, hist_base, "fired at tol = d")
    assert p.flag(h, hist_base, it, patience, np.nextafter(dsum, np.inf)) == it + 1, (length, hist_base)


# patience = length - hist_base: with hist_base = 37 the lengths below 37 do not exist (module docstring)
@pytest.mark.parametrize("length,hist_base", [(n, hb) for n in LENGTHS for hb in (0, 37) if n >= hb])
def test_plateau_sum_matches_numpy(plateau_linear, length, hist_base):
    _check_k_converge(plateau_linear, length, hist_base)


def test_plateau_guards(plateau_linear):
    p = plateau_linear
    h, _ = _history(12, 8, 1, 12)
    assert p.flag(h, 0, 11, 11, float("inf")) == 0   # iter == patience: not tested yet
    assert p.flag(h, 0, 11, 10, float("inf")) == 12  # (one iteration later it is)
    assert p.flag(h, 0, 11, 10, 0.0) == 0            # tol = 0 never fires


@pytest.mark.parametrize("name", ["conv_small", "f64_small"])
def test_plateau_sum_other_launch_sites(name):
    p = _Plateau(name)
    for length in (8, 129, 1000):
        for hist_base in (0, 37) if length >= 37 else (0,):
            _check_k_converge(p, length, hist_base)
    assert same_bits(p.d["params"], p.params0)


@pytest.mark.parametrize("patience", [0, 1, 2, 3, 10, 200])
def test_converge_tail_slices(patience):
    """The later modules' rule: tested once len(loss_running) > patience, over loss_running[-patience + 1:]."""
    p = _Plateau("phase_small")
    try:
        for n_losses in (patience + 1, patience + 50):
            for hist_base in (0, 4):
                it = n_losses - 1 - hist_base
                if it < 0:
                    continue
                lo = 1 if patience == 0 else 0 if patience == 1 else n_losses - (patience - 1)  # (seed choice only)
                h, _ = _history(n_losses, 8, lo, n_losses)
                sl = np.array(h[:n_losses])[-patience + 1:]
                dsum = np.sum(np.abs(np.diff(sl)))
                if patience == 2:
                    assert len(sl) == 1 and dsum == 0.0  # no diffs: fires for any tol > 0
                assert p.flag(h, hist_base, it, patience, dsum) == 0, (patience, n_losses, hist_base)
                assert p.flag(h, hist_base, it, patience, np.nextafter(dsum, np.inf)) == it + 1, \
                    (patience, n_losses, hist_base)
        if patience >= 5:  # n_losses == patience: not tested, even with tol = inf
            h, _ = _history(patience, 8, 0, patience)
            assert p.flag(h, 4, patience - 5, patience, float("inf")) == 0
            assert p.flag(h, 0, patience - 1, patience, float("inf")) == 0
        assert same_bits(p.d["params"], p.params0)
    finally:
        p.close()
