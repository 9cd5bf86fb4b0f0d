"""GPU checks of score_many / predict_many (multinomial_tensor_regression): the forward pass, argmax,
confusion counts and data loss of many (model, data set) pairs in one launch (k_mnl_score_many).

The yardstick for values is the fp64 closed form of tests/hier_ref.py (`model(..., dtype=float64)` and
torch's CrossEntropyLoss on it), never `predict` or the code under test.  Bars: 1e-5 normwise relative
on the probabilities and 1e-5 relative on the loss (the project's fixture bar); the integer results
(pred against the returned prob, counts, acc, cm) are exact; pred against fp64 on every row whose fp64
top-two probabilities differ by more than 1e-4, at most 5 % of the rows left out.

Measured on the MI355X (pytest -s prints them): see DESIGN.md, "Scoring the sweep".
"""
import functools

import numpy as np
import pytest
import torch

import hier_ref

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5      # prob (normwise relative) and loss (relative)
GAP = 1e-4       # fp64 top-two gap below which a row's argmax is not compared
CAP = 0.05       # at most this share of rows may be left out
PATTERNS = [[bool(k & 1), bool(k & 2), bool(k & 4)] for k in range(8)]


def _M():
    from tensor_regression_amd import multinomial_tensor_regression as M
    return M


def _H():
    from tensor_regression_amd import multinomial_tensor_regression_hierarchical as H
    return H


def block():
    from tensor_regression_amd import _engine
    return int(_engine.SCORE_ROW_BLOCK)


class Case:
    """Seeded data and factors of one (model, data set) pair.  The factors hold values on both sides of
    the softplus threshold (beta 50, threshold 1: a = 0.02): every factor of two or more elements has
    0.015 at its first and 0.5 at its last; of one-element factors the first mode's is above and the
    second's below."""

    def __init__(self, N, dims, C, R, nn, seed, scale=1.6, xscale=1.0, cw=False):
        rng = np.random.default_rng(seed)
        self.N, self.dims, self.C, self.R, self.nn = N, tuple(dims), C, R, list(nn)
        self.X = (rng.standard_normal((N,) + self.dims) * xscale).astype(np.float32)
        self.y = rng.integers(0, C, size=N).astype(np.int64)
        self.y[:min(N, C)] = np.arange(min(N, C))
        self.B = []
        for f, k in enumerate(self.dims + (C,)):
            A = ((rng.random((k, R)) - (0.0 if nn[f] else 0.5)) * scale).astype(np.float32)
            if A.size >= 2:
                A.reshape(-1)[0], A.reshape(-1)[-1] = 0.015, 0.5
            else:
                A.reshape(-1)[0] = (0.8, 0.015, 0.5)[f]
            self.B.append(A)
        self.w = (0.5 + rng.random(R)).astype(np.float32)
        self.cw = (0.5 + rng.random(C)).astype(np.float32) if cw else None

    def model(self, mod=None):
        Bcp = [torch.tensor(a, device=DEV) for a in self.B]
        return (mod or _M()).CP_logistic_regression(self.X, self.y, rank=self.R, non_negative=self.nn,
                                                    weights=self.w, Bcp_init=Bcp, device=DEV)


def ref64(B, w, nn, X, y=None, cw=None):
    """(probabilities, weighted-mean CrossEntropyLoss of them) in float64 on the CPU."""
    t = lambda a: torch.tensor(np.asarray(a), dtype=torch.float64)
    S = hier_ref.model(t(X), [t(A) for A in B], t(w), nn)
    if y is None:
        return S.numpy(), None
    loss = torch.nn.CrossEntropyLoss(weight=None if cw is None else t(cw))(S, torch.tensor(np.asarray(y)))
    return S.numpy(), float(loss)


def left_out(S64):
    """Rows whose fp64 top-two probabilities are within GAP of one another."""
    if S64.shape[1] < 2:
        return np.zeros(S64.shape[0], dtype=bool)
    top = np.sort(S64, axis=1)
    return (top[:, -1] - top[:, -2]) <= GAP


def host_counts(pred, y, C):
    counts = np.zeros((C, C), dtype=np.int64)
    for p, t in zip(pred, y):
        counts[p, t] += 1
    return counts


def check_entry(what, score, prob, pred, S64, loss64, y, C):
    """One entry's results against fp64 (bars above) and against one another (exact)."""
    N = y.size
    e_prob = hier_ref.normwise_rel(prob, S64)
    e_loss = abs(score["loss"] - loss64) / abs(loss64)
    out = left_out(S64)
    print(f"{what}: prob {e_prob:.2e}  loss {e_loss:.2e}  rows left out {int(out.sum())}/{N}")
    assert prob.dtype == np.float32 and prob.shape == (N, C) and pred.dtype == np.int64 and pred.shape == (N,)
    assert e_prob <= RTOL, what
    assert e_loss <= RTOL, what
    assert np.array_equal(pred, np.argmax(prob, axis=1)), what
    assert out.mean() <= CAP, (what, out.mean())
    assert np.array_equal(pred[~out], np.argmax(S64, axis=1)[~out]), what
    counts = score["counts"]
    assert counts.dtype == np.int64 and np.array_equal(counts, host_counts(pred, y, C)), what
    assert counts.sum() == N and score["acc"] == np.trace(counts) / N, what
    if len(np.unique(y)) == C:
        cm = _M().confusion_matrix(pred, y)
        assert score["cm"].dtype == np.float64 and score["cm"].tobytes() == cm.tobytes(), what


def score_and_predict(models, X=None, y=None, weights=None, expect_batched=True):
    M = _M()
    rs, rp = {}, {}
    scores = M.score_many(models, X=X, y_true=y, weights=weights, report=rs)
    preds = M.predict_many(models, X=X, report=rp)
    if expect_batched:
        assert rs == rp == {"batched": list(range(len(models))), "alone": [], "launches": 1}, (rs, rp)
    return scores, preds


# ---- 1, 2, 3: values against fp64, the exact quantities, the capped argmax -------------------------

def largest_image():
    """(dims, C, R) at the largest P * C of the kernel's envelope: C = 16, R = 1, the feature dims that
    leave the factors the fewest words."""
    from tensor_regression_amd import _engine
    best = None
    for I0 in range(1, 65):
        lo, hi = 0, 1 << 16
        while lo < hi:
            mid = (lo + hi + 1) // 2
            lo, hi = (mid, hi) if _engine.score_envelope(I0, mid, 16, 1) else (lo, mid - 1)
        if lo >= 1 and (best is None or I0 * lo > best[0] * best[1]):
            best = (I0, lo)
    return best, 16, 1


SHAPES = {"one": (1, (1, 1), 2, 1, 1.6), "odd_p": (7, (3, 5), 3, 2, 1.6), "kim": (227, (8, 12), 4, 6, 1.6),
          "c16_r16": (50, (5, 7), 16, 16, 1.6), "largest": None}


@pytest.mark.parametrize("name", list(SHAPES))
def test_values_against_fp64_for_every_nonneg_pattern(name):
    if name == "largest":
        dims, C, R = largest_image()
        N, scale = 3, 1.0
        from tensor_regression_amd import _engine
        assert not _engine.score_envelope(dims[0], dims[1] + 1, C, R)
        print("largest image:", dims, "P*C =", dims[0] * dims[1] * C)
    else:
        N, dims, C, R, scale = SHAPES[name]
    cases = [Case(N, dims, C, R, nn, seed=14 + k, scale=scale, cw=bool(k % 2)) for k, nn in enumerate(PATTERNS)]
    models = [c.model() for c in cases]
    scores, preds = score_and_predict(models, weights=[c.cw for c in cases])
    for c, s, (prob, pred) in zip(cases, scores, preds):
        S64, loss64 = ref64(c.B, c.w, c.nn, c.X, c.y, c.cw)
        check_entry(f"{name} nn={c.nn}", s, prob, pred, S64, loss64, c.y, C)


def test_large_logits_stay_finite_and_rows_sum_to_one():
    cases = [Case(227, (8, 12), 4, 6, nn, seed=40 + k, xscale=1e3) for k, nn in enumerate(PATTERNS)]
    scores, preds = score_and_predict([c.model() for c in cases])
    for c, s, (prob, pred) in zip(cases, scores, preds):
        # the logits are linear in X: their spread at X / 1e3, from the fp64 probabilities, times 1e3
        L = np.log(ref64(c.B, c.w, c.nn, c.X.astype(np.float64) / 1e3)[0])
        spread = 1e3 * (L.max(axis=1) - L.min(axis=1)).max()
        e_sum = np.abs(prob.astype(np.float64).sum(axis=1) - 1.0).max()
        print(f"nn={c.nn}: logits spread over {spread:.0f}, rows sum to 1 within {e_sum:.1e}")
        assert spread >= 1e3
        assert np.isfinite(prob).all() and (prob >= 0).all()
        assert e_sum <= 1e-6
        assert np.isfinite(s["loss"]) and np.array_equal(pred, np.argmax(prob, axis=1))
        assert np.array_equal(s["counts"], host_counts(pred, c.y, c.C))


def test_zero_class_factor_gives_equal_probabilities_and_class_zero():
    cases = [Case(70, (3, 5), 3, 2, nn, seed=60 + k) for k, nn in enumerate(PATTERNS)]
    for c in cases:
        c.B[2][:] = 0.0
    scores, preds = score_and_predict([c.model() for c in cases])
    for c, s, (prob, pred) in zip(cases, scores, preds):
        assert (prob == prob[0, 0]).all() and abs(float(prob[0, 0]) - 1.0 / 3.0) < 1e-7
        assert (pred == 0).all()
        assert np.array_equal(s["counts"], host_counts(pred, c.y, 3)) and s["counts"][1:].sum() == 0


# ---- 4: row blocks ---------------------------------------------------------------------------------

@pytest.mark.parametrize("where", ["below", "at", "above", "three_and_one"])
def test_row_blocks(where):
    B = block()
    N = {"below": B - 1, "at": B, "above": B + 1, "three_and_one": 3 * B + 1}[where]
    cases = [Case(N, (3, 5), 3, 2, nn, seed=70 + k, cw=bool(k % 2)) for k, nn in enumerate(PATTERNS[::3])]
    scores, preds = score_and_predict([c.model() for c in cases], weights=[c.cw for c in cases])
    for c, s, (prob, pred) in zip(cases, scores, preds):
        S64, loss64 = ref64(c.B, c.w, c.nn, c.X, c.y, c.cw)
        check_entry(f"N={N} nn={c.nn}", s, prob, pred, S64, loss64, c.y, 3)


def same_bits(a, b):
    (sa, (pa, qa)), (sb, (pb, qb)) = a, b
    return (pa.tobytes() == pb.tobytes() and np.array_equal(qa, qb) and np.array_equal(sa["counts"], sb["counts"])
            and np.float64(sa["loss"]).tobytes() == np.float64(sb["loss"]).tobytes() and sa["acc"] == sb["acc"])


def test_strided_device_view_is_bitwise_its_contiguous_copy():
    B = block()
    c = Case(2 * (B + 3), (3, 5), 3, 2, [True, False, True], seed=80, cw=True)
    Xd = torch.tensor(c.X, device=DEV)
    view = Xd[::2]
    assert not view.is_contiguous() and view.stride(0) == 30
    y = c.y[::2].copy()
    m = c.model()
    sv, pv = score_and_predict([m], X=[view], y=[y], weights=[c.cw])
    sc, pc = score_and_predict([m], X=[view.contiguous()], y=[y], weights=[c.cw])
    assert same_bits((sv[0], pv[0]), (sc[0], pc[0]))
    S64, loss64 = ref64(c.B, c.w, c.nn, c.X[::2], y, c.cw)
    check_entry("strided view", sv[0], pv[0][0], pv[0][1], S64, loss64, y, 3)


# ---- 5: independence and reproducibility -----------------------------------------------------------

def one_alone(m, X, y, cw):
    s, p = score_and_predict([m], X=[X], y=[y], weights=[cw])
    return s[0], p[0]


def test_heterogeneous_batch_is_bitwise_every_entry_alone():
    B = block()
    cases = [Case(1, (1, 1), 2, 1, [False] * 3, seed=90),
             Case(B + 5, (3, 5), 3, 2, [True, False, True], seed=91, cw=True),
             Case(227, (8, 12), 4, 6, [True] * 3, seed=92),
             Case(40, (4, 4), 16, 2, [False, True, False], seed=93, cw=True),
             Case(2 * B + 1, (3, 3), 3, 16, [False, False, True], seed=94),
             Case(30, (33, 8), 4, 2, [False] * 3, seed=95, cw=True)]
    models = [c.model(_H() if k % 2 else _M()) for k, c in enumerate(cases)]  # the two modules mixed
    Xs, ys, cws = [None] * len(cases), [None] * len(cases), [c.cw for c in cases]
    # one model on four data sets: its own, two other draws and a strided device view
    kim = cases[2]
    rng = np.random.default_rng(99)
    for k in range(3):
        n = (50, B, B + 77)[k]
        Xk = rng.standard_normal((n, 8, 12)).astype(np.float32)
        models.append(models[2])
        Xs.append(torch.tensor(np.repeat(Xk, 2, axis=0), device=DEV)[::2] if k == 2 else Xk)
        ys.append(rng.integers(0, 4, size=n))
        cws.append(kim.cw if k else (0.5 + rng.random(4)).astype(np.float32))
    scores, preds = score_and_predict(models, X=Xs, y=ys, weights=cws)
    again = score_and_predict(models, X=Xs, y=ys, weights=cws)
    for j, m in enumerate(models):
        got = (scores[j], preds[j])
        assert same_bits(got, (again[0][j], again[1][j])), f"entry {j}: second call"
        assert same_bits(got, one_alone(m, Xs[j], ys[j], cws[j])), f"entry {j}: alone"
    for j, c in enumerate(cases):  # and the values are right
        S64, loss64 = ref64(c.B, c.w, c.nn, c.X, c.y, c.cw)
        check_entry(f"entry {j}", scores[j], preds[j][0], preds[j][1], S64, loss64, c.y, c.C)


def tiny_cases():
    B = block()
    return [Case((3, B - 1, 9, B + 2, 17)[k % 5] + k, (2, 3), 2 + k % 2, 1 + k % 3,
                 [bool(k & 1), bool(k & 2), bool(k & 4)], seed=100 + k, cw=bool(k % 2)) for k in range(10)]


@functools.lru_cache(maxsize=None)
def tiny_alone():
    """The ten tiny entries scored alone (computed once, shared, never modified)."""
    return [(c, c.model()) + one_alone(c.model(), None, None, c.cw) for c in tiny_cases()]


@pytest.mark.parametrize("M", [1, 2, 300])
def test_more_workgroups_than_compute_units(M):
    alone = tiny_alone()
    models = [alone[j % 10][1] for j in range(M)]
    scores, preds = score_and_predict(models, weights=[alone[j % 10][0].cw for j in range(M)])
    for j in range(M):
        assert same_bits((scores[j], preds[j]), alone[j % 10][2:]), f"entry {j}"
    if M == 300:
        for c, _, s, (prob, pred) in alone:
            S64, loss64 = ref64(c.B, c.w, c.nn, c.X, c.y, c.cw)
            check_entry(f"tiny N={c.N}", s, prob, pred, S64, loss64, c.y, c.C)


# ---- 6: the sweep end to end -----------------------------------------------------------------------

def test_fit_many_then_score_many_on_held_out_halves():
    H = _H()
    cases = [Case(2 * n, dims, C, R, nn, seed=200 + k, scale=1.0)
             for k, (n, dims, C, R, nn) in enumerate([(40, (3, 4), 3, 2, [False, False, False]),
                                                      (33, (2, 5), 2, 3, [True, False, True]),
                                                      (64, (8, 12), 4, 6, [True, True, True]),
                                                      (25, (4, 3), 3, 2, [False, True, False])])]
    models = []
    for c in cases:
        h = c.N // 2
        Bcp = [torch.tensor(a, device=DEV).requires_grad_(True) for a in c.B]
        models.append(H.CP_logistic_regression(c.X[:h], c.y[:h], rank=c.R, non_negative=c.nn, weights=c.w,
                                               Bcp_init=Bcp, device=DEV))
    rep = {}
    H.fit_Adam_many(models, lambda_L2=0.01, max_iter=40, tol=0.0, Adam_kwargs={"lr": 0.02}, report=rep)
    assert rep["batched"] == [0, 1, 2, 3]
    held_X = [c.X[c.N // 2:] for c in cases]
    held_y = [c.y[c.N // 2:] for c in cases]
    scores, preds = score_and_predict(models + models, X=held_X + [None] * 4, y=held_y + [None] * 4)
    for j, (c, m) in enumerate(zip(cases, models)):
        fitted = [A.detach().cpu().numpy() for A in m.Bcp]
        assert any(not np.array_equal(a, b) for a, b in zip(fitted, c.B))  # the fit moved the factors
        h = c.N // 2
        for at, X, y, what in ((j, held_X[j], held_y[j], "held out"), (4 + j, c.X[:h], c.y[:h], "training")):
            S64, loss64 = ref64(fitted, c.w, c.nn, X, y)
            check_entry(f"model {j} {what}", scores[at], preds[at][0], preds[at][1], S64, loss64, y, c.C)


# ---- 7: fallback -----------------------------------------------------------------------------------

def predict_plus_host_metrics(m, X, y, cw, C):
    """An entry handled alone: its own predict, the metrics on the host."""
    prob, pred = m.predict(X=X)
    lsum, wsum, counts = _M()._host_score(prob, pred, np.asarray(y), cw, C)
    return prob, pred, lsum / wsum, counts


def test_entries_outside_the_batch_keep_predict_and_their_order(monkeypatch):
    M = _M()
    rng = np.random.default_rng(300)
    inside = Case(20, (3, 4), 3, 2, [True, False, False], seed=301)
    r17 = Case(20, (3, 4), 3, 17, [False, True, False], seed=302, cw=True)
    X4 = rng.standard_normal((15, 2, 3, 2)).astype(np.float32)
    y4 = np.arange(15) % 3
    B4 = [torch.tensor((rng.random((k, 2)) - 0.5).astype(np.float32), device=DEV) for k in (2, 3, 2, 3)]
    m4 = M.CP_logistic_regression(X4, y4, rank=2, non_negative=[False] * 4, Bcp_init=B4, device=DEV)
    models = [inside.model(), r17.model(), m4, inside.model(_H())]
    cws = [None, r17.cw, None, None]
    rs, rp = {}, {}
    scores = M.score_many(models, weights=cws, report=rs)
    preds = M.predict_many(models, report=rp)
    assert rs == rp == {"batched": [0, 3], "alone": [1, 2], "launches": 1}
    for j, (m, y, C) in enumerate(zip(models, (inside.y, r17.y, y4, inside.y), (3, 3, 3, 3))):
        prob, pred, loss, counts = predict_plus_host_metrics(m, None, y, cws[j], C)
        assert np.array_equal(preds[j][1], pred) and np.array_equal(scores[j]["counts"], counts), j
        if j in (1, 2):  # alone: predict's own bits
            assert preds[j][0].tobytes() == prob.tobytes() and scores[j]["loss"] == loss, j
        else:
            assert hier_ref.normwise_rel(preds[j][0], prob) <= RTOL and abs(scores[j]["loss"] - loss) <= RTOL * loss
    assert same_bits((scores[0], preds[0]), (scores[3], preds[3]))
    # the values of the entries handled alone against fp64 as well
    S64, loss64 = ref64(r17.B, r17.w, r17.nn, r17.X, r17.y, r17.cw)
    check_entry("rank 17", scores[1], preds[1][0], preds[1][1], S64, loss64, r17.y, 3)
    # the route switched off: every entry alone, same results as predict
    monkeypatch.setenv("TR_MNL_RESIDENT", "0")
    rs = {}
    off = M.score_many(models, weights=cws, report=rs)
    assert rs == {"batched": [], "alone": [0, 1, 2, 3], "launches": 0}
    for j, (m, y) in enumerate(zip(models, (inside.y, r17.y, y4, inside.y))):
        prob, pred, loss, counts = predict_plus_host_metrics(m, None, y, cws[j], 3)
        assert off[j]["loss"] == loss and np.array_equal(off[j]["counts"], counts), j
        assert off[j]["acc"] == np.trace(counts) / y.size
