"""Numerics of the exact three-term bf16 split the column-slice spectral kernel runs its GEMMs
with (bfs_split2 of csrc/tr_bf16_split.h; csrc/tr_spectral_slice.hip: sl_mfma6 / sl_mfma_lp), restated in numpy on the
fp32 bit patterns (CPU; the kernel itself is covered by tests/test_gpu_spectral.py and, at full
config-5 size against fp64, tests/test_gpu_fullsize.py).

  x1 = bf16_rne(x), r = x - x1 (exact), x2 = bf16_rne(r), x3 = r - x2 (at most 8 significant
  bits: exactly a bf16)  (TR_SLICE_SPLITMODE 2, the default)
  a.b ~ a1b1 + a1b2 + a2b1 + a1b3 + a2b2 + a3b1   (dropped: a2b3 + a3b2 + a3b3 < 2^-24 |ab|)

The round-3 split truncated every piece (split3_trunc below, TR_SLICE_SPLITMODE 0): its pieces
all carry the sign of x, so the dropped terms are biased toward the sign of ab, and over the
config-5 gradient sums that bias came to 8-25x the f32 MFMA form's error.  Mode 1 truncates x1
and rounds x2 / x3 (unbiased, dropped terms < 2^-22 |ab|).

By default the kernel splits only the factor side (Phi0, dT) in three; the sample data X goes in
two round-to-nearest pieces (split2_rne, |x - x1 - x2| < 2^-16 |x|), five MFMAs per product
instead of six.  TR_SLICE_XPIECES=3 splits X in three as well (the six terms above).
"""
import numpy as np
import pytest

MASK = np.uint32(0xFFFF0000)


def rne_bf16(v):
    """fp32 -> bf16 (round to nearest even) -> fp32, as v_cvt_pk_bf16_f32 (finite inputs)"""
    u = np.asarray(v, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return (((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16).astype(np.uint32).view(np.float32)


def split3(x):
    """TR_SLICE_SPLITMODE 2 (default): every piece by round-to-nearest"""
    x = np.asarray(x, dtype=np.float32)
    x1 = rne_bf16(x)
    r = (x - x1).astype(np.float32)
    x2 = rne_bf16(r)
    x3 = (r - x2).astype(np.float32)
    return x1, x2, x3


def split3_hybrid(x):
    """TR_SLICE_SPLITMODE 1: x1 truncated, x2 by round-to-nearest"""
    x = np.asarray(x, dtype=np.float32)
    x1 = (x.view(np.uint32) & MASK).view(np.float32)
    r = (x - x1).astype(np.float32)
    x2 = rne_bf16(r)
    return x1, x2, (r - x2).astype(np.float32)


def split3_trunc(x):
    """TR_SLICE_SPLITMODE 0 (round 3): every piece truncated"""
    x = np.asarray(x, dtype=np.float32)
    x1 = (x.view(np.uint32) & MASK).view(np.float32)
    r = (x - x1).astype(np.float32)
    x2 = (r.view(np.uint32) & MASK).view(np.float32)
    x3 = (r - x2).astype(np.float32)
    return x1, x2, x3


def _rand(n, seed):
    g = np.random.default_rng(seed)
    # wide exponent range, both signs, including values whose low bits are all set
    x = (g.standard_normal(n) * np.exp2(g.integers(-60, 60, n))).astype(np.float32)
    x[:8] = np.array([1.0, -1.0, 3.0000002, np.float32(1) - np.float32(2 ** -24), 1e-30, -7.5e30,
                      np.float32(0.1), 0.0], dtype=np.float32)
    # the kernel's domain: finite, below the bf16 overflow threshold (3.39e38)
    return x[np.isfinite(x) & (np.abs(x) < 3.3e38)]


@pytest.mark.parametrize("mode", [2, 1, 0])
def test_split_is_exact_and_bf16(mode):
    sp = {2: split3, 1: split3_hybrid, 0: split3_trunc}[mode]
    x = _rand(200000, 0)
    x1, x2, x3 = sp(x)
    # every piece is a bf16 (low 16 bits zero) and the pieces sum back to x exactly
    for p in (x1, x2, x3):
        assert not np.any(p.view(np.uint32) & np.uint32(0xFFFF))
    s = (x1.astype(np.float64) + x2.astype(np.float64)) + x3.astype(np.float64)
    assert np.array_equal(s, x.astype(np.float64))
    # magnitude bounds the error analysis uses
    ax = np.abs(x.astype(np.float64))
    b2, b3 = {2: (-8, -17), 1: (-7, -16), 0: (-7, -14)}[mode]
    assert np.all(np.abs(x2) <= ax * 2.0 ** b2)
    assert np.all(np.abs(x3) <= ax * 2.0 ** b3)


def _six_term_rel(sp, seed_a=1, seed_b=2, n=200000):
    a, b = _rand(n, seed_a), _rand(n, seed_b)
    m = min(len(a), len(b))
    a, b = a[:m], b[:m]
    a1, a2, a3 = (p.astype(np.float64) for p in sp(a))
    b1, b2, b3 = (p.astype(np.float64) for p in sp(b))
    six = a1 * b1 + a1 * b2 + a2 * b1 + a1 * b3 + a2 * b2 + a3 * b1
    exact = a.astype(np.float64) * b.astype(np.float64)
    nz = exact != 0
    return (six[nz] - exact[nz]) / np.abs(exact[nz]), np.sign(exact[nz])


def test_six_term_product_error():
    # the bound the kernel comment, the public header and DESIGN.md state for the default split:
    # < 2^-24 |ab| worst case (measured 2^-24.3), median 2^-29; no bias toward the sign of ab
    rel, sgn = _six_term_rel(split3)
    assert np.abs(rel).max() < 2.0 ** -24
    assert np.median(np.abs(rel)) < 2.0 ** -28
    assert abs((rel * sgn).mean()) < 0.01 * 2.0 ** -24
    rel, sgn = _six_term_rel(split3_hybrid)
    assert np.abs(rel).max() < 2.0 ** -22
    assert abs((rel * sgn).mean()) < 0.01 * 2.0 ** -24


def test_truncating_split_is_biased():
    """the round-3 split: the dropped terms pull every product toward zero (relative -0.69 x 2^-24
    on average), which is what summed to the full-size gradient error the default avoids"""
    rel, sgn = _six_term_rel(split3_trunc)
    assert np.abs(rel).max() < 2.0 ** -20
    assert (rel * sgn).mean() < -0.3 * 2.0 ** -24


def test_biased_split_error_grows_with_cancellation():
    """a long signed sum with heavy cancellation (a gradient over many samples): the unbiased
    split stays at the fp32 accumulation's error level, the truncating one does not"""
    g = np.random.default_rng(7)
    n = 1 << 18
    a = np.abs(g.standard_normal(n)).astype(np.float32)
    b = (g.standard_normal(n) * 0.2).astype(np.float32)
    b -= np.float32(np.dot(a.astype(np.float64), b.astype(np.float64)) / np.dot(a.astype(np.float64), a))
    b = b.astype(np.float32) * np.float32(1) + np.float32(1e-3)  # small mean: strong cancellation
    exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
    scale = float(np.abs(a.astype(np.float64) * b.astype(np.float64)).sum())

    def six(sp):
        a1, a2, a3 = (p.astype(np.float64) for p in sp(a))
        b1, b2, b3 = (p.astype(np.float64) for p in sp(b))
        return float((a1 * b1 + a1 * b2 + a2 * b1 + a1 * b3 + a2 * b2 + a3 * b1).sum())
    e_rne = abs(six(split3) - exact) / scale
    e_trunc = abs(six(split3_trunc) - exact) / scale
    assert e_rne < 2.0 ** -30
    assert e_trunc > 8 * e_rne


def test_packed_lin_columns_sum_to_the_six_terms():
    """[b1 | b2] with A = a1, a2, a3 and [b3 | 0] with A = a1: columns c and c + 8 summed give the
    six terms plus a3b2 (sl_mfma_lp + sl_fold8)"""
    a, b = _rand(5000, 3), _rand(5000, 4)
    a1, a2, a3 = (p.astype(np.float64) for p in split3(a))
    b1, b2, b3 = (p.astype(np.float64) for p in split3(b))
    col_lo = a1 * b1 + a2 * b1 + a3 * b1 + a1 * b3
    col_hi = a1 * b2 + a2 * b2 + a3 * b2
    six = a1 * b1 + a1 * b2 + a2 * b1 + a1 * b3 + a2 * b2 + a3 * b1
    assert np.allclose(col_lo + col_hi - six, a3 * b2, rtol=0, atol=1e-300 + 1e-12 * np.abs(six).max())


def test_dot_product_matches_fp32_quality():
    """a W x D contraction at config 5's size: the split sum is as close to the exact dot product
    as a plain fp32 accumulation of fp32 products"""
    g = np.random.default_rng(5)
    n = 256 * 129
    a = np.abs(g.standard_normal(n)).astype(np.float32)
    b = (g.standard_normal(n) * 0.2).astype(np.float32)
    exact = float(np.dot(a.astype(np.float64), b.astype(np.float64)))
    a1, a2, a3 = split3(a)
    b1, b2, b3 = split3(b)
    acc = np.float32(0)
    terms = [(a1, b1), (a1, b2), (a2, b1), (a1, b3), (a2, b2), (a3, b1)]
    # fp32 accumulation of exact bf16 x bf16 products, 32 at a time (one MFMA k step)
    prods = sum(np.float64(1) * p.astype(np.float64) * q.astype(np.float64) for p, q in terms)
    for k in range(0, n, 32):
        acc = np.float32(acc + np.float32(prods[k:k + 32].sum()))
    ref32 = np.float32(0)
    for k in range(0, n, 32):
        ref32 = np.float32(ref32 + np.float32((a[k:k + 32] * b[k:k + 32]).astype(np.float32).sum()))
    scale = float(np.abs(a.astype(np.float64) * b.astype(np.float64)).sum())
    assert abs(float(acc) - exact) <= 2 * abs(float(ref32) - exact) + 1e-7 * scale


def split2_rne(x):
    """the sample side (X) as two round-to-nearest-even bf16 pieces: the default
    (TR_SLICE_XPIECES=3 selects split3 for X as well)"""
    x = np.asarray(x, dtype=np.float32)

    def rne_bf16(v):
        u = v.view(np.uint32).astype(np.uint64)
        r = ((u + 0x7FFF + ((u >> 16) & 1)) >> 16) << 16
        return r.astype(np.uint32).view(np.float32)

    x1 = rne_bf16(x)
    r = (x - x1).astype(np.float32)
    return x1, rne_bf16(r)


def test_two_piece_rne_split_bound():
    x = _rand(200000, 6)
    x = x[np.isfinite(x) & (np.abs(x) > 1e-30) & (np.abs(x) < 1e30)]
    x1, x2 = split2_rne(x)
    err = np.abs(x.astype(np.float64) - x1.astype(np.float64) - x2.astype(np.float64))
    # |x - x1| <= half an 8-bit ulp <= 2^-8 |x|, and the second rounding leaves at most 2^-8 of
    # that: <= 2^-16 |x| (measured worst case on this sample 2^-17, median 2^-19.4)
    assert np.all(err <= np.abs(x.astype(np.float64)) * 2.0 ** -16)



def _full_size_grad_errs(n_out=4, terms=129 * 32768, seed=11):
    """A config-5-sized gradient reduction (dPhi0[w, k] = sum over 129 d x 32768 samples of
    X[n, w, d] dT[n, d, k]): n_out outputs of `terms` products each, X = |N(0, 1)| (bench.py's X)
    and a signed dT whose sum cancels (sum |ab| / |sum ab| ~ 40).  Products are formed from the
    pieces the kernel multiplies and summed in float64, i.e. the split's own error with exact
    accumulation.  Returns the normwise relative errors of the default form (X in two
    round-to-nearest pieces, the factor side in three: a1b1 + a1b2 + a2b1 + a1b3 + a2b2) and of
    the round-3 truncating split (three truncated pieces per operand, six terms)."""
    g = np.random.default_rng(seed)
    exact, e_def, e_tr = [], [], []
    for _ in range(n_out):
        a = np.abs(g.standard_normal(terms)).astype(np.float32)
        b = (g.standard_normal(terms) * 0.5 + 0.01).astype(np.float32)
        a64, b64 = a.astype(np.float64), b.astype(np.float64)
        exact.append(float(np.dot(a64, b64)))
        a1, a2 = (p.astype(np.float64) for p in split2_rne(a))
        b1, b2, b3 = (p.astype(np.float64) for p in split3(b))
        e_def.append(float(np.dot(a1, b1 + b2 + b3) + np.dot(a2, b1 + b2)))
        t1, t2, t3 = (p.astype(np.float64) for p in split3_trunc(a))
        u1, u2, u3 = (p.astype(np.float64) for p in split3_trunc(b))
        e_tr.append(float(np.dot(t1, u1 + u2 + u3) + np.dot(t2, u1 + u2) + np.dot(t3, u1)))
    ex = np.array(exact)
    nrm = np.linalg.norm(ex)
    return np.linalg.norm(np.array(e_def) - ex) / nrm, np.linalg.norm(np.array(e_tr) - ex) / nrm


def test_split_errors_alone_stay_far_below_the_bar():
    """At config 5's reduction length (129 x 32768 products per gradient element, cancelling
    sums) the products' own split errors, accumulated exactly, stay ~25x below the full-size
    absolute bar (1e-6, tests/test_gpu_fullsize.py) for BOTH forms: the truncating split is exact
    (its per-product bias is proportional to the product, so it cannot grow with cancellation:
    ~4e-8 here), the default's two-piece X is inexact but unbiased.  So the 2.8e-6 the truncating
    split measured on the GPU is not its products: it is the bf16 MFMA's accumulation, which
    drops the low bits of small addends by a sign-dependent truncation
    (tools/mfma_bf16_round.hip, DESIGN.md "bf16 split GEMMs") — and the truncating split's small
    pieces all carry the sign of their product, so those drops are biased.  That is why the bar is
    held on the GPU, with a negative control
    (test_gpu_fullsize.py::test_spectral_full_size_bar_rejects_truncating_split)."""
    e_def, e_tr = _full_size_grad_errs()
    assert e_def < 1e-6 / 10 and e_tr < 1e-6 / 10, (e_def, e_tr)


def split_bf16_f16(x):
    """The multinomial duo kernel's bf16-split body (k_mnl_bsp, tr_mnl_duo.hip): x1 = bf16_rne(x),
    x2 = f16_rne(x - x1) (v_cvt_pk_bf16_f32 / v_cvt_pk_f16_f32)"""
    x = np.asarray(x, dtype=np.float32)
    x1 = rne_bf16(x)
    x2 = (x - x1).astype(np.float32).astype(np.float16)
    return x1, x2


def test_bf16_f16_split_bound():
    """x1 + x2 represents x to 2^-20 |x| for 2^-5 <= |x| < 2^24: |x - x1| <= 2^-8 |x| (half a bf16
    ulp), and its f16 rounding keeps 11 significant bits (2^-12 relative) while it is a normal f16,
    or an absolute 2^-25 (half the subnormal spacing) below — 2^-20 |x| again at |x| >= 2^-5;
    below 2^-5 the error stays <= 2^-25 absolute.  Median 2^-22.5 (measured here)."""
    g = np.random.default_rng(8)
    x = (g.standard_normal(400000) * np.exp2(g.integers(-12, 24, 400000))).astype(np.float32)
    x1, x2 = split_bf16_f16(x)
    assert np.all(np.isfinite(x2.astype(np.float64)))
    err = np.abs(x.astype(np.float64) - x1.astype(np.float64) - x2.astype(np.float64))
    ax = np.abs(x.astype(np.float64))
    big = ax >= 2.0 ** -5
    assert np.all(err[big] <= ax[big] * 2.0 ** -20)
    assert np.all(err[~big] <= 2.0 ** -25)
    assert np.median(err[big] / ax[big]) < 2.0 ** -22
    # versus two bf16 pieces (the spectral kernel's X): 2^-17 / 2^-19.5 worst / median here,
    # 8x / 7x coarser
    x2b = rne_bf16((x - x1).astype(np.float32))
    errb = np.abs(x.astype(np.float64) - x1.astype(np.float64) - x2b.astype(np.float64))
    assert np.median(errb[big] / ax[big]) > 6 * np.median(err[big] / ax[big])
    assert (errb[big] / ax[big]).max() > 6 * (err[big] / ax[big]).max()


def test_bsp_products_cover_every_term():
    """One 16-wide accumulator per tile: x1.[b1 | b2] + x1.[b3 | 0] (bf16) + x2.[h1 | h2] (f16,
    h1 = f16(b), h2 = f16(b - h1)), columns r and r + 8 folded: x1 (b1 + b2 + b3) + x2 (h1 + h2),
    i.e. x1 b exactly plus x2 b to 2^-22: the product's error is the representation error of x"""
    a, b = _rand(20000, 9), _rand(20000, 10)
    m = min(len(a), len(b))
    a, b = a[:m], b[:m]
    ok = (np.abs(a) > 2.0 ** -5) & (np.abs(a) < 2.0 ** 20) & (np.abs(b) > 2.0 ** -10) & (np.abs(b) < 2.0 ** 14)
    a, b = a[ok], b[ok]
    x1, x2 = (p.astype(np.float64) for p in split_bf16_f16(a))
    b1, b2, b3 = (p.astype(np.float64) for p in split3(b))
    h1 = b.astype(np.float16)
    h2 = (b - h1.astype(np.float32)).astype(np.float16)
    prod = x1 * (b1 + b2 + b3) + x2 * (h1.astype(np.float64) + h2.astype(np.float64))
    exact = a.astype(np.float64) * b.astype(np.float64)
    rel = np.abs(prod - exact) / np.abs(exact)
    assert rel.max() <= 2.0 ** -19.9
