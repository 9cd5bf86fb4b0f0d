"""GPU checks of fit_Adam_many (multinomial_tensor_regression_hierarchical): many independent resident
fits in one launch, workgroup j fitting member j (k_mnl_resident_many).

The yardstick is the single route: "alone" is `fit_Adam` on a fresh, identically built model, which
takes the resident route (one workgroup, k_mnl_resident).  Both kernels run the same device function
in the same fixed order, so a member of any batch must come back bit for bit as it does alone:
factors, loss history and the convergence flag.

  * a heterogeneous batch of seven shapes (one sample; N below the G-pass split count; N no multiple
    of 64; the notebook's features; C and R at their limits; P C > 1024) with different non_negative,
    lambda, lr, one amsgrad + weight_decay member and group_lr breakpoints at 3 and 66, over 70
    iterations (two launches)
  * members that stop in different chunks, one that never stops; per-member max_iter 3 / 64 / 65 / 130
  * 300 members (more workgroups than CUs), and 1 and 2
  * the largest carve beside the smallest in one launch
  * every Adam fixture in one call against the reference's recorded outputs, hier_4d falling back
  * a second call continues the history; TR_MNL_RESIDENT=0 sends every member to its own fit_Adam
"""
import functools

import numpy as np
import pytest
import torch

import hier_ref
import test_gpu_hier as tg

pytestmark = pytest.mark.gpu

DEV = tg.DEV


def _H():
    return tg._H()


class Case:
    """One member: seeded data and start (test_gpu_hier.sweep_case) plus its own fit arguments."""

    def __init__(self, N, dims, C, R, nn, lam=0.01, ak=None, group_lr=None, max_iter=70, tol=0.0, patience=10,
                 seed=None):
        self.N, self.dims, self.C, self.R, self.nn = N, tuple(dims), C, R, list(nn)
        self.lam, self.ak, self.group_lr = lam, dict(ak or {"lr": 0.01}), group_lr
        self.max_iter, self.tol, self.patience = max_iter, tol, patience
        self.X, self.y, self.B0, self.w = tg.sweep_case(N, self.dims, C, R, self.nn,
                                                         seed=(N + 7 * C + R) if seed is None else seed)

    def model(self):
        Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in self.B0]
        return _H().CP_logistic_regression(self.X, self.y, rank=self.R, non_negative=self.nn, weights=self.w,
                                           Bcp_init=Bcp, device=DEV)

    def kwargs(self):
        return dict(lambda_L2=self.lam, max_iter=self.max_iter, tol=self.tol, patience=self.patience,
                    Adam_kwargs=dict(self.ak), group_lr=self.group_lr)


class FixtureCase:
    """A member built from a hier_* fixture with the fixture's own arguments (optionally overridden)."""

    def __init__(self, name, **over):
        self.d = tg.fixture(name)
        m = self.d["meta"]
        self.kw = dict(lambda_L2=m["lambda_L2"], max_iter=m["max_iter"], tol=m["tol"], patience=m["patience"],
                       Adam_kwargs=dict(m["adam_kwargs"]), group_lr=m["group_lr"])
        self.kw.update(over)

    def model(self):
        return tg.new_model(self.d)

    def kwargs(self):
        return dict(self.kw, Adam_kwargs=dict(self.kw["Adam_kwargs"]))


def fit_alone(case, calls=1, resident=True):
    mm = case.model()
    conv = None
    for _ in range(calls):
        conv = mm.fit_Adam(**case.kwargs())
    if resident:
        assert tg.route_of(mm) == "resident", mm._plan.describe
    return mm, conv


def fit_many(cases, calls=1):
    H = _H()
    models = [c.model() for c in cases]
    kws = [c.kwargs() for c in cases]
    report, conv = {}, None
    for _ in range(calls):
        conv = H.fit_Adam_many(models, report=report, **{k: [kw[k] for kw in kws] for k in kws[0]})
    return models, conv, report


def assert_same_fit(got, got_conv, want, want_conv, what):
    assert bool(got_conv) == bool(want_conv), what
    assert len(got.loss_running) == len(want.loss_running), (what, len(got.loss_running), len(want.loss_running))
    assert list(got.loss_running) == list(want.loss_running), what  # exact float equality
    for x, y in zip(tg.bits_of_fit(got), tg.bits_of_fit(want)):
        assert np.array_equal(x, y), what


def check_batch_against_alone(cases, calls=1, batched=None):
    models, conv, report = fit_many(cases, calls=calls)
    assert report["batched"] == (list(range(len(cases))) if batched is None else batched), report
    for j, c in enumerate(cases):
        a, ca = fit_alone(c, calls=calls)
        assert_same_fit(models[j], conv[j], a, ca, f"member {j}")
    return models, conv, report


# ---- 1: a heterogeneous batch --------------------------------------------------------------------

def hetero_cases():
    return [
        Case(1, (2, 3), 2, 1, [False, False, False], lam=0.01, ak={"lr": 0.01}),                 # one sample
        Case(5, (3, 4), 3, 2, [True, False, True], lam=0.02,                                     # N < split count
             ak={"lr": 0.02}, group_lr=[[(0, 0.02), (3, 0.004)], 0.01, 0.03]),
        Case(37, (2, 5), 2, 3, [False, True, False], lam=0.005, ak={"lr": 0.005}),               # N % 64 != 0
        Case(40, (8, 12), 4, 6, [True, True, True], lam=0.005,                                   # the notebook's features
             ak={"lr": 0.05, "amsgrad": True, "weight_decay": 0.01, "betas": (0.8, 0.99), "eps": 1e-6}),
        Case(65, (4, 4), 16, 2, [True, True, False], lam=0.03,                                   # C at its limit
             ak={"lr": 0.01, "amsgrad": True}, group_lr=[0.01, [(0, 0.02), (66, 0.001)], 0.005]),
        Case(20, (3, 3), 3, 16, [False, False, True], lam=0.015, ak={"lr": 0.03}),               # R at its limit
        Case(30, (33, 8), 4, 2, [False, False, False], lam=0.01, ak={"lr": 0.007}),              # P C = 1056 > 1024
    ]


def test_heterogeneous_batch_is_bitwise_the_single_route():
    cases = hetero_cases()
    models, conv, report = check_batch_against_alone(cases)
    assert report["batched"] == list(range(7)) and report["alone"] == []
    # 70 iterations with breakpoints at 3 and 66: launches [0, 3), [3, 66) in one piece of 63, [66, 70)
    assert report["launches"] == 3
    assert all(len(m.loss_running) == 70 for m in models) and not any(conv)


# ---- 2: different stops --------------------------------------------------------------------------

def test_members_stop_in_different_chunks():
    cases = [
        FixtureCase("hier_converge"),                                     # the recorded plateau stop
        FixtureCase("hier_converge", tol=3e-4),                           # a later chunk
        FixtureCase("hier_kim"),                                          # never (tol 1e-6 over 100 losses)
    ]
    models, conv, report = check_batch_against_alone(cases)
    n = [len(m.loss_running) for m in models]
    print("stops", n, conv)
    assert conv[0] and conv[1] and not conv[2] and n[2] == cases[2].kw["max_iter"] == 150
    assert n[0] == len(cases[0].d["loss_running"])  # the reference stops where we do
    assert (n[0] - 1) // 64 < (n[1] - 1) // 64  # launches after member 0's stop left it untouched
    assert report["launches"] == 5


def test_per_member_max_iter():
    shapes = [(9, (2, 3), 2, 1), (12, (3, 4), 3, 2), (17, (2, 5), 2, 3), (8, (4, 3), 3, 2)]
    cases = [Case(N, dims, C, R, [False, True, False], max_iter=mi)
             for (N, dims, C, R), mi in zip(shapes, (3, 64, 65, 130))]
    models, conv, report = check_batch_against_alone(cases)
    assert [len(m.loss_running) for m in models] == [3, 64, 65, 130]
    assert report["launches"] == 3


# ---- 3: more workgroups than CUs -----------------------------------------------------------------

def tiny_cases():
    return [Case(8 + k, (2, 3), 2, 1 + k % 2, [bool(k & 1), bool(k & 2), bool(k & 4)], lam=0.01 + 0.002 * k,
                 ak={"lr": 0.01 + 0.003 * k}, max_iter=3, seed=100 + k) for k in range(10)]


@functools.lru_cache(maxsize=None)
def tiny_alone():
    """The ten tiny configurations fitted alone (computed once, shared, never modified)."""
    return [fit_alone(c) for c in tiny_cases()]


@pytest.mark.parametrize("M", [1, 2, 300])
def test_more_workgroups_than_compute_units(M):
    base = tiny_cases()
    cases = [base[j % 10] for j in range(M)]
    models, conv, report = fit_many(cases)
    assert report["batched"] == list(range(M)) and report["launches"] == 1
    alone = tiny_alone()
    for j in range(M):
        a, ca = alone[j % 10]
        assert_same_fit(models[j], conv[j], a, ca, f"member {j}")  # hence replicas equal one another


# ---- 4: mixed LDS sizes --------------------------------------------------------------------------

def test_largest_and_smallest_carve_in_one_launch():
    _, dims, C, R = tg.NMAX_KIM
    cases = [Case(tg.max_rows(dims, C, R), dims, C, R, [True] * 3, ak={"lr": 0.01, "amsgrad": True}, max_iter=2),
             Case(1, (2, 3), 2, 1, [False] * 3, max_iter=2)]
    check_batch_against_alone(cases)


# ---- 5: reference parity -------------------------------------------------------------------------

def test_every_adam_fixture_in_one_call_matches_the_reference():
    names = list(hier_ref.ADAM_FIXTURES)
    cases = [FixtureCase(n) for n in names]
    models, conv, report = fit_many(cases)
    at4 = names.index("hier_4d")
    assert report["alone"] == [at4] and report["batched"] == [j for j in range(len(names)) if j != at4]
    for name, c, mm, cv in zip(names, cases, models, conv):
        d = c.d
        assert len(mm.loss_running) == len(d["loss_running"]) and int(cv) == int(d["converged"]), name
        e_loss = np.max(np.abs(np.asarray(mm.loss_running) - d["loss_running"]) / np.abs(d["loss_running"]))
        print(f"{name}: loss {e_loss:.2e}")
        assert e_loss <= tg.RTOL, name
        r64 = tg.ref64(name)
        for a, b, c64 in zip(tg.factors(mm), d["Bcp_final_list"], r64["Bcp"]):
            if hier_ref.normwise_rel(a, b) <= tg.RTOL:
                continue
            assert hier_ref.normwise_rel(a, c64) <= 2.0 * hier_ref.normwise_rel(b, c64), (name, a.shape)


# ---- 6: second call and fallbacks ----------------------------------------------------------------

def test_second_call_continues_the_history():
    cases = [FixtureCase("hier_signed", max_iter=7, tol=1e-9, patience=3),
             FixtureCase("hier_cpw", max_iter=5, tol=1e-9, patience=4),
             Case(12, (3, 4), 3, 2, [False, True, False], max_iter=6, tol=1e-9, patience=2)]
    models, _, _ = check_batch_against_alone(cases, calls=2)
    assert [len(m.loss_running) for m in models] == [14, 10, 12]


def test_route_switched_off_fits_every_member_alone(monkeypatch):
    cases = hetero_cases()[:3]
    for c in cases:
        c.max_iter = 5
    tg.set_route(monkeypatch, "streamed")
    models, conv, report = fit_many(cases)
    assert report == {"batched": [], "alone": [0, 1, 2], "launches": 0}
    for j, c in enumerate(cases):  # the members' own streamed fit_Adam
        a, ca = fit_alone(c, resident=False)
        assert tg.route_of(a) == "streamed"
        assert_same_fit(models[j], conv[j], a, ca, f"member {j}")
