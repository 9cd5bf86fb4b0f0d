"""Strided and windowed X through every fp32 kernel path (tr_plan_set_x_stride).

Every case runs twice, each on a fresh plan: on a view laid out by tests/strided_ref.py (NaN canaries in
every float that belongs to no row) and on view.contiguous().  The contract: a result depends only on
the P floats of each row.

  * Where both plans name the same strategy (strided_ref.strategy_words of tr_plan_describe), every raw
    buffer -- the gradient arena with its data-loss and status slots, per call; the finalised gradient;
    the loss; the forward / predict output -- is bitwise the contiguous copy's.
  * Where the stride forced another kernel, both results meet the sweeps' own bars against the oracle
    (test_gpu_parity.py / test_gpu_spectral.py): loss and data loss rel <= 1e-5, every factor gradient
    normwise <= 1e-5, forward rtol 1e-5 with the sweeps' atol.
  * Nothing in any output is NaN.

Which of the two applies is asserted per cell (expect() below; a plan that silently fell back to another
kernel fails instead of passing on the looser bar):

    layout   stride        P % 4 == 0                      P % 4 != 0
    pad4     P + 4         bitwise                         bitwise (W = 1 either way)
    ovl4     4k <= P/2     bitwise                         bitwise
    win      prod F[1:]    bitwise if stride % 4 == 0      bitwise
    pad5     P + 5         oracle: W = 4 -> 1, no cluster, bitwise (odd or not, the plan had no
    ovl3     P - 3           no factored multinomial or      vector path to lose)
    off1     P + 5, +4 B     MFMA forward, spectral vec=0
    one      N = 1         bitwise (a single row has no stride)

The linear fused and packed passes themselves read any 4-byte aligned row (buffer loads), so in an
"oracle" cell of a fused linear row only W (the forward and two-pass kernels) differs.  Exceptions to
the table, named where they occur: the packed kernel's 32-bit offset guard hands rows more than
2 GiB apart to k_linear_fused (test_rows_2gib_apart), and a cap_* clamp (none occurs in this matrix:
no stride here asks for more workgroups than the creation-time workspace was carved for).

Cells: linear 96 bitwise / 29 oracle, multinomial 101 / 51, spectral 26 / 30.

Forms observed on an MI355X (256 CUs), reported here and not pinned by the tests:
  (130, 16, 16) and (N = 3 grid + 1 = 24577, 16, 16) T=64 CH=1 grid=8192; (200, 100, 100) T=512 CH=5;
  (150, 11, 13) T=64 CH=1; (120, 33, 31) T=64 CH=4; (90, 101, 99) T=512 CH=5; (60, 127, 129) T=256 CH=16;
  (40, 64, 64, 32) S=5 clusters=51; (77, 45000) S=2 clusters=128; (2, 200, 332) S=3 clusters=85;
  multinomial: form=rankblock waves=4; form=bf16split at waves 2, 3, 4 and 8, jt=32, rowblocks=3, rk=16 nbuf=3.
"""
import ctypes
import zlib

import numpy as np
import pytest
import torch

import strided_ref as sr
from golden_util import normwise_rel
from test_gpu_parity import path
from test_gpu_spectral import SHAPES as SPEC_SHAPES, WIDE_SHAPES as SPEC_WIDE_SHAPES, spec_path

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
RTOL = 1e-5


def _seed(*key):
    return zlib.crc32(repr(key).encode()) % 2**31


def expect(P, layout, stride):
    """The table of the module docstring."""
    if layout == "one" or P % 4 != 0 or stride % 4 == 0:
        return "bitwise"
    return "oracle"


def _layouts(N, F):
    return [lay for lay in sr.LAYOUTS if sr.applies(lay, N, F)]


_X_CACHE = {}


def _layout(row, layout, N, F, draw=None):
    """The layout of one matrix row; the non-overlapping layouts of a row share one X (so they share the
    contiguous run and the oracle as well).  -> (layout object, key of its X)"""
    if layout in sr.OVERLAPPING:
        key = (row, layout)
        if key not in _X_CACHE:
            _X_CACHE[key] = sr.build(layout, N, F, seed=_seed(row, layout), draw=draw)
        return _X_CACHE[key], key
    key = (row, "free")
    if key not in _X_CACHE:
        _X_CACHE[key] = sr.build("pad4", N, F, seed=_seed(row), draw=draw).X
    X = _X_CACHE[key]
    if layout == "one":
        return sr.build("one", 1, F, X=X[:1]), (row, "one")
    return sr.build(layout, N, F, X=X), key


def _device_view(lay):
    base = lay.base.to(DEV)
    assert base.data_ptr() % 16 == 0
    Xv = sr.view_of(lay, base)
    assert Xv.data_ptr() % 16 == (4 if lay.layout == "off1" else 0)
    return Xv


_CONTIG = {}  # (X key, kind, extra) -> the contiguous copy's result (computed once, never modified)
_ORACLE = {}


def _judge(rv, rc, want, bars, cell):
    bv, bc = sr.buffers(rv), sr.buffers(rc)
    for k, t in bv.items():
        assert not sr.has_nan(t), (cell, k, "NaN in the view's result: a canary reached it", rv["describe"])
    for k, t in bc.items():
        assert not sr.has_nan(t), (cell, k, "NaN in the contiguous result")
    wv, wc = sr.strategy_words(rv["describe"]), sr.strategy_words(rc["describe"])
    print(f"{cell}: {want}; view: {' '.join(wv)} | contiguous: {' '.join(wc)}")
    if want == "bitwise":
        assert wv == wc, (cell, "the stride moved an aligned plan to another kernel", rv["describe"], rc["describe"])
        for k in bc:
            assert sr.same_bits(bv[k], bc[k]), (cell, k, "differs from the contiguous copy", rv["describe"])
    else:
        assert wv != wc, (cell, "expected the stride to force another kernel", rv["describe"])
        bars(rv)
        bars(rc)


# =====================================================================================================
# (a) linear
# =====================================================================================================
def _lin_params(shape, rank):
    g = torch.Generator().manual_seed(_seed("lin", shape, rank))
    F = shape[1:]
    nn = [bool(i % 2) for i in range(len(F))]
    Bcp0 = [torch.randn(d, rank, generator=g) * 0.3 for d in F]
    w = torch.rand(rank, generator=g) + 0.5
    y = torch.randn(shape[0], generator=g)
    return nn, Bcp0, w, y


def _lin_run(X, shape, rank, calls=2, plan=None):
    from tensor_regression_amd import _engine, _lib
    nn, Bcp0, w, y = _lin_params(shape, rank)
    N = X.shape[0]
    own = plan is None
    if own:
        plan = _engine.Plan(_lib.TR_MODEL_LINEAR, list(shape[1:]), 1, rank, shape[0], nn, None, DEV)
    try:
        return sr.run_linear(plan, X, y[:N].to(DEV), [b.to(DEV) for b in Bcp0], torch.tensor([0.25], device=DEV),
                             w.to(DEV), 0.01, calls=calls)
    finally:
        if own:
            plan.destroy()


def _lin_bars(X, shape, rank, okey):
    from oracle import cp_oracle
    nn, Bcp0, w, y = _lin_params(shape, rank)
    if okey not in _ORACLE:
        _ORACLE[okey] = cp_oracle.linear_loss_grad(X, y[:X.shape[0]], Bcp0, torch.tensor([0.25]), w, nn, 0.01)
    ref = _ORACLE[okey]
    nf = sum(d * rank for d in shape[1:])

    def bars(res):
        for grad in res["grad"]:
            dl = grad[nf + 1].item()
            assert abs(dl - ref["data_loss"]) <= RTOL * abs(ref["data_loss"]), (dl, ref["data_loss"])
        assert abs(res["loss"].item() - ref["loss"]) <= RTOL * abs(ref["loss"])
        at = 0
        for d, r in zip(shape[1:], ref["grads"]):
            got = res["gtot"][at:at + d * rank].reshape(d, rank).cpu().numpy()
            assert normwise_rel(got, r) <= RTOL, (normwise_rel(got, r), got.shape)
            at += d * rank
        np.testing.assert_allclose(res["fwd"].cpu().numpy(), ref["y_hat"].reshape(-1), rtol=RTOL,
                                   atol=RTOL * np.abs(ref["y_hat"]).max())
    return bars


def _linear_cell(shape, rank, kind, layout, calls=2, check=None):
    N, F = shape[0], tuple(shape[1:])
    row = ("lin", shape, rank)
    lay, xkey = _layout(row, layout, N, F)
    with path(kind):
        rv = _lin_run(_device_view(lay), shape, rank, calls)
        ckey = (xkey, kind, calls)
        if ckey not in _CONTIG:
            _CONTIG[ckey] = _lin_run(lay.X.to(DEV), shape, rank, calls)
        rc = _CONTIG[ckey]
    cell = (shape, rank, kind, layout)
    want = expect(lay.P, layout, lay.stride)
    if check is not None:
        check(rv["describe"], rc["describe"])
    _judge(rv, rc, want, _lin_bars(lay.X, shape, rank, xkey), cell)
    return rv, rc


def _cells(rows):
    """[(row..., layout)] for rows of (shape, rank, kinds...)"""
    out = []
    for shape, rank, kinds in rows:
        for kind in kinds:
            for lay in _layouts(shape[0], shape[1:]):
                out.append(pytest.param(shape, rank, kind, lay, id=f"{'x'.join(map(str, shape))}-r{rank}-{kind}-{lay}"))
    return out


LIN_PACKED = [((700, 4, 5), 3, ["auto"]), ((300, 3, 3), 3, ["auto"])]
LIN_FUSED = [((130, 16, 16), 8, ["auto"]), ((200, 100, 100), 4, ["auto"])]
# P % 4 != 0: the fused pass with a partial last quad at CH = 1 and CH > 1; W = 1 rows / cols above one wave
LIN_ODD_P = [((150, 11, 13), 3, ["auto", "twopass"]), ((120, 33, 31), 3, ["auto", "twopass"]),
             ((90, 101, 99), 3, ["auto", "twopass"]), ((60, 127, 129), 3, ["auto", "twopass"])]
LIN_CLUSTER = [((40, 64, 64, 32), 16, ["auto"]), ((77, 45000), 3, ["auto"]), ((2, 200, 332), 4, ["auto"])]
LIN_TWOPASS = [((257, 6, 7, 8, 3), 5, ["twopass"]), ((129, 100, 101), 2, ["twopass"])]


@pytest.mark.parametrize("shape,rank,kind,layout", _cells(LIN_PACKED))
def test_linear_packed(shape, rank, kind, layout):
    """k_linear_packed: every layout next to test_linear_packed_strided_rows' +5 / -3 pads"""
    def check(dv, dc):
        assert " pk=" in dv and " pk=" in dc, (dv, dc)
    _linear_cell(shape, rank, kind, layout, check=check)


@pytest.mark.parametrize("shape,rank,kind,layout", _cells(LIN_FUSED + LIN_ODD_P))
def test_linear_fused(shape, rank, kind, layout):
    """k_linear_fused at an exact fit, a padded P % 4 == 0 row and four P % 4 != 0 rows (the partial last
    quad must come out of the row's own range check, not of a zero coefficient); under twopass the same
    rows through k_rows / k_cols at W = 1"""
    def check(dv, dc):
        for d in (dv, dc):
            assert ("path=fused-1pass" in d and " pk=" not in d) if kind == "auto" else "path=2pass" in d, d
    _linear_cell(shape, rank, kind, layout, check=check)


@pytest.mark.parametrize("layout", _layouts(9, (16, 16)))
def test_linear_fused_prefetch_ring(layout):
    """>= 3 rows per workgroup (N = 3 grid + 1, grid read from the contiguous plan): the prefetch of row
    i + 1 over a stride, in both traversal directions (two consecutive calls walk the rows in opposite
    orders)"""
    from tensor_regression_amd import _engine, _lib
    with path("auto"):
        probe = _engine.Plan(_lib.TR_MODEL_LINEAR, [16, 16], 1, 3, 1, [False, True], None, DEV)
        grid = int(sr.word(probe.describe, "grid"))
        probe.destroy()
    N = 3 * grid + 1
    assert grid >= 1 and N * (256 + 5) * 4 <= 64 * 2**20, (grid, N)

    def check(dv, dc):
        assert "path=fused-1pass" in dv and "path=fused-1pass" in dc and sr.word(dv, "grid") == str(grid), (dv, dc)
    rv, rc = _linear_cell((N, 16, 16), 3, "auto", layout, calls=2, check=check)
    assert len(rv["grad"]) == 2 and len(rc["grad"]) == 2


@pytest.mark.parametrize("shape,rank,kind,layout", _cells(LIN_CLUSTER))
def test_linear_cluster(shape, rank, kind, layout):
    """the cluster pass: 5 slices, a ragged last slice, N below the cluster count; an odd stride turns it
    off (the rows run the two-pass kernels at W = 1)"""
    P = sr.volume(shape[1:])

    def check(dv, dc):
        assert "path=cluster-1pass" in dc, dc
        want_cluster = layout == "one" or sr.row_stride(layout, shape[1:]) % 4 == 0
        assert ("path=cluster-1pass" in dv) == want_cluster, dv
    assert P % 4 == 0
    _linear_cell(shape, rank, kind, layout, check=check)


@pytest.mark.parametrize("shape,rank,kind,layout", _cells(LIN_TWOPASS))
def test_linear_twopass(shape, rank, kind, layout):
    """k_rows / k_cols at W = 4, and at W = 1 under the odd layouts"""
    def check(dv, dc):
        assert "path=2pass" in dv and "path=2pass" in dc and " W=4 " in dc, (dv, dc)
        odd = layout != "one" and sr.row_stride(layout, shape[1:]) % 4 != 0
        assert (" W=1 " in dv) == odd, dv
    _linear_cell(shape, rank, kind, layout, check=check)


# =====================================================================================================
# (b) multinomial
# =====================================================================================================
def _mnl_params(shape, C, rank, xscale=1.0):
    g = torch.Generator().manual_seed(_seed("mnl", shape, C, rank))
    y = torch.randint(0, C, (shape[0],), generator=g)
    y[:C] = torch.arange(C)
    P = sr.volume(shape[1:])
    if xscale == 1.0:  # test_multinomial_sweep_vs_oracle's recipe
        nn = [bool(i % 2 == 0) for i in range(len(shape))]
        sc = 0.3 * min(1.0, (2048.0 / P) ** (1.0 / len(shape)))
        Bcp0 = [torch.randn(d, rank, generator=g) * sc for d in list(shape[1:]) + [C]]
        lam = 0.02
    else:  # test_multinomial_split_body_x_scale's: plain factors scaled against X, no L2 term
        nn = [False] * len(shape)
        sc = 0.3 * min(1.0, (2048.0 / P) ** 0.5)
        fs = xscale ** -0.5
        Bcp0 = [torch.randn(d, rank, generator=g) * sc * fs for d in shape[1:]] + [torch.randn(C, rank, generator=g) * sc]
        lam = 0.0
    cw = torch.rand(C, generator=g) + 0.5
    return nn, Bcp0, cw, y, lam


def _mnl_run(X, shape, C, rank, xscale=1.0, plan=None, calls=2):
    from tensor_regression_amd import _engine, _lib
    nn, Bcp0, cw, y, lam = _mnl_params(shape, C, rank, xscale)
    own = plan is None
    if own:
        plan = _engine.Plan(_lib.TR_MODEL_MULTINOMIAL, list(shape[1:]), C, rank, shape[0], nn, None, DEV)
    try:
        return sr.run_multinomial(plan, X, y[:X.shape[0]].to(DEV), cw.to(DEV), [b.to(DEV) for b in Bcp0],
                                  torch.ones(rank, device=DEV), lam, calls=calls)
    finally:
        if own:
            plan.destroy()


def _mnl_bars(X, shape, C, rank, okey):
    from oracle import cp_oracle
    nn, Bcp0, cw, y, lam = _mnl_params(shape, C, rank)
    N = X.shape[0]
    if okey not in _ORACLE:
        _ORACLE[okey] = cp_oracle.mnl_loss_grad(X, y[:N], Bcp0, np.ones(rank), nn, cw.numpy(), lam)
    ref = _ORACLE[okey]
    dims = list(shape[1:]) + [C]
    nf = sum(d * rank for d in dims)

    def bars(res):
        for grad in res["grad"]:
            dl = grad[nf].item()
            assert abs(dl - ref["data_loss"]) <= RTOL * abs(ref["data_loss"]), (dl, ref["data_loss"])
        assert abs(res["loss"].item() - ref["loss"]) <= RTOL * abs(ref["loss"])
        at = 0
        for d, r in zip(dims, ref["grads"]):
            got = res["gtot"][at:at + d * rank].reshape(d, rank).cpu().numpy()
            assert normwise_rel(got, r) <= RTOL, (normwise_rel(got, r), got.shape)
            at += d * rank
        np.testing.assert_allclose(res["fwd"].cpu().numpy(), ref["probs"], rtol=RTOL, atol=1e-6)
    return bars


# (shape, C, rank, kinds, words the contiguous plan's description must hold, TR_DUO_ANYFILL)
MNL_ROWS = [
    ((257, 64, 128), 4, 8, ["auto"], ["form=rankblock"], False),
    ((100, 128, 64), 10, 8, ["auto"], ["form=rankblock"], False),
    ((300, 64, 64), 10, 8, ["split"], ["form=bf16split", "waves=2"], False),
    ((200, 96, 64), 7, 3, ["auto"], ["form=bf16split", "waves=3"], False),
    ((300, 100, 64), 10, 8, ["auto"], ["form=bf16split", "waves=4"], False),   # padded rows
    ((200, 128, 48), 10, 8, ["auto"], ["form=bf16split"], False),              # padded width
    ((200, 1, 64), 5, 3, ["auto"], ["form=bf16split", "waves=2"], True),       # fewer rows than two waves
    ((80, 128, 128), 10, 8, ["auto"], ["form=bf16split", "waves=8"], False),   # 128-wide
    ((200, 128, 24), 5, 4, ["auto"], ["form=bf16split", "jt=32"], False),      # 32-wide
    ((40, 576, 64), 5, 5, ["auto"], ["form=bf16split", "rowblocks=3"], False),
    ((90, 160, 64), 4, 9, ["auto"], ["form=bf16split", "rk=16", "nbuf=3"], False),
    ((333, 32, 32), 10, 8, ["noduo", "spi1"], ["path=mnl-fused-1pass", "units="], False),  # k_mnl_fused
    ((200, 16, 8), 10, 4, ["twopass", "valu"], ["path=2pass"], False),
    ((97, 5, 7), 16, 3, ["twopass", "valu"], ["path=2pass"], False),           # P = 35
    ((230, 16, 8), 40, 5, ["auto", "valu"], ["path=2pass+wide"], False),       # wide-class MFMA / VALU tiles
    ((99, 5, 7), 33, 2, ["auto"], ["path=2pass+wide"], False),
    ((64, 33), 3, 1, ["auto"], ["path=2pass"], False),                         # one feature mode
]


def _mnl_cells():
    out = []
    for shape, C, rank, kinds, words, anyfill in MNL_ROWS:
        for kind in kinds:
            for lay in _layouts(shape[0], shape[1:]):
                out.append(pytest.param(shape, C, rank, kind, words, anyfill, lay,
                                        id=f"{'x'.join(map(str, shape))}-C{C}-r{rank}-{kind}-{lay}"))
    return out


@pytest.mark.parametrize("shape,C,rank,kind,words,anyfill,layout", _mnl_cells())
def test_multinomial(shape, C, rank, kind, words, anyfill, layout, monkeypatch):
    """k_mnl_duo, every form of k_mnl_bsp, k_mnl_fused, k_rows_mfma / k_rows + k_cols, and the wide-class
    tiles with k_softmax_rows.  The odd layouts switch the factored kernels and the MFMA forward off:
    those cells take the oracle bars."""
    monkeypatch.delenv("TR_DUO_ANYFILL", raising=False)
    if anyfill:
        monkeypatch.setenv("TR_DUO_ANYFILL", "1")
    N, F = shape[0], tuple(shape[1:])
    row = ("mnl", shape, C, rank)
    lay, xkey = _layout(row, layout, N, F)
    with path(kind):
        rv = _mnl_run(_device_view(lay), shape, C, rank)
        ckey = (xkey, kind, anyfill)
        if ckey not in _CONTIG:
            _CONTIG[ckey] = _mnl_run(lay.X.to(DEV), shape, C, rank)
        rc = _CONTIG[ckey]
    for w in words:
        assert w in rc["describe"], (w, rc["describe"])
    if kind == "valu":
        assert "mfma" not in rc["describe"], rc["describe"]
    want = expect(lay.P, layout, lay.stride)
    if want == "oracle":  # no vector path is left on an odd stride
        assert "path=2pass" in rv["describe"] and "mfma" not in rv["describe"] and " W=1 " in rv["describe"], rv["describe"]
    _judge(rv, rc, want, _mnl_bars(lay.X, shape, C, rank, xkey), (shape, C, rank, kind, layout))


@pytest.mark.parametrize("layout", ["pad4", "ovl4", "win"])
@pytest.mark.parametrize("xscale", [3e7, 1e-4])
def test_multinomial_exact_x_form_on_a_view(xscale, layout):
    """k_mnl_bsp's exact X form is chosen from k_x_range's scan of the VIEW (max |x| >= 2^23, or a sample
    rms below 2^-5): a canary that reached the scan would make the range NaN, and a scan of other floats
    would pick another form.  (The odd layouts run no split body, so no scan: not in this test.)"""
    shape, C, rank = (300, 64, 64), 10, 8
    row = ("mnlx", shape, C, rank, xscale)
    lay, xkey = _layout(row, layout, shape[0], shape[1:], draw=lambda n, g: torch.randn(n, generator=g) * xscale)
    with path("split"):
        rv = _mnl_run(_device_view(lay), shape, C, rank, xscale)
        rc = _mnl_run(lay.X.to(DEV), shape, C, rank, xscale)
    assert "form=bf16split" in rc["describe"] and " xform=exact" in rc["describe"], rc["describe"]
    assert " xform=exact" in rv["describe"], rv["describe"]
    _judge(rv, rc, "bitwise", None, (shape, xscale, layout))


@pytest.mark.parametrize("layout", _layouts(37, (6, 7)))
def test_x_range_on_a_view(layout):
    """tr_x_range over each layout: max |x| and min x exactly numpy's over the logical rows, the smallest
    row mean-square (a double sum in another order) to 1e-12"""
    from tensor_regression_amd import _lib
    from tensor_regression_amd._engine import stream_handle
    lib = _lib.load()
    lay, _ = _layout(("xr", 37, (6, 7)), layout, 37, (6, 7))
    Xv = _device_view(lay)
    N, P = lay.N, lay.P
    for nb in (1, min(1024, N)):
        out = torch.full((3 * nb,), float("nan"), dtype=torch.float64, device=DEV)
        _lib.check(lib.tr_x_range(_lib.ptr(Xv), N, P, int(Xv.stride(0)), _lib.ptr(out), nb, stream_handle(0)),
                   "tr_x_range")
        r = out.cpu().numpy()
        assert not np.isnan(r).any(), r
        X = lay.X.reshape(N, P).double().numpy()
        assert r[:nb].max() == np.abs(X).max()
        assert r[2 * nb:].min() == X.min()
        msq = (X * X).mean(axis=1).min()
        assert abs(r[nb:2 * nb].min() - msq) <= 1e-12 * msq, (r[nb:2 * nb].min(), msq)


# =====================================================================================================
# (c) spectral
# =====================================================================================================
def _spec_params(N, W, D, O, Rn, Rs, ncd):
    g = torch.Generator().manual_seed(_seed("spec", N, W, D, O, Rn, Rs, ncd))
    y = torch.randn(N, O, generator=g)
    Bn = [torch.randn(W, Rn, 1, generator=g) * 0.2, torch.randn(D, Rn, 1, generator=g) * 0.2,
          torch.randn(O, Rn, 1, generator=g)]
    Bc = [torch.randn(W, Rs, ncd + 1, generator=g) * 0.2, torch.randn(D, Rs, 1, generator=g) * 0.2,
          torch.randn(O, Rs, 1, generator=g)]
    bias = torch.randn(O, generator=g) * 0.1
    return y, Bn, Bc, bias


def _spec_run(X, case, plan=None, calls=2):
    from tensor_regression_amd import _engine
    N, W, D, O, Rn, Rs, ncd, nn = case
    y, Bn, Bc, bias = _spec_params(N, W, D, O, Rn, Rs, ncd)
    own = plan is None
    if own:
        plan = _engine.SpectralPlan(W, D, O, Rn, Rs, ncd + 1, N, nn, None, DEV)
    try:
        return sr.run_spectral(plan, X, y[:X.shape[0]].to(DEV), [a.to(DEV) for a in Bn], [a.to(DEV) for a in Bc],
                               bias.to(DEV), torch.ones(Rn + Rs, device=DEV), 0.01, calls=calls)
    finally:
        if own:
            plan.destroy()


def _spec_bars(X, case, okey):
    """test_spectral_shapes_vs_closed_form's references: the fp64 closed form, the fp64 predict model and
    the einsum latents"""
    from oracle import cp_oracle
    N, W, D, O, Rn, Rs, ncd, nn = case
    y, Bn, Bc, bias = _spec_params(N, W, D, O, Rn, Rs, ncd)
    n = X.shape[0]
    if okey not in _ORACLE:
        c = cp_oracle.closed_form_spectral(X.numpy(), y[:n].numpy(), [a.numpy() for a in Bn], [a.numpy() for a in Bc],
                                           bias.numpy(), np.ones(Rn + Rs), Rn, nn, 0.01)
        c["predict"] = cp_oracle.spectral_predict(X.double(), [a.double() for a in Bn], [a.double() for a in Bc],
                                                  torch.ones(Rn + Rs, dtype=torch.float64), Rn, nn, bias.double()).numpy()
        sp = lambda a, on: (torch.nn.functional.softplus(a.double(), beta=50, threshold=1) if on else a.double()).numpy()
        c["lat"] = np.einsum('twd,wr,dr->tr', X.double().numpy(), sp(Bn[0][:, :, 0], nn[0]), sp(Bn[1][:, :, 0], nn[1]))
        _ORACLE[okey] = c
    c = _ORACLE[okey]
    sizes = [W * Rn, D * Rn, O * Rn, W * Rs * (ncd + 1), D * Rs, O * Rs]

    def bars(res):
        assert normwise_rel(res["yhat"].cpu().numpy(), c["y_hat"]) <= RTOL
        nf = sum(sizes)
        for grad in res["grad"]:
            dl = grad[nf + O].item()
            assert abs(dl - c["data_loss"]) <= RTOL * abs(c["data_loss"]), (dl, c["data_loss"])
        assert abs(res["loss"].item() - c["loss"]) <= RTOL * abs(c["loss"])
        at = 0
        for sz, ref in zip(sizes, c["grads_n"] + c["grads_c"]):
            if ref.size:
                got = res["gtot"][at:at + sz].cpu().numpy().reshape(ref.shape)
                assert normwise_rel(got, ref) <= RTOL, (normwise_rel(got, ref), ref.shape)
            at += sz
        assert normwise_rel(res["gtot"][at:].cpu().numpy(), c["bias_grad"]) <= 1e-4
        assert normwise_rel(res["fwd"].cpu().numpy(), c["predict"]) <= RTOL
        if Rn:
            assert normwise_rel(res["lat"].cpu().numpy(), c["lat"]) <= RTOL
    return bars


NN0 = [False, False, False]
# (case (N, W, D, n_out, Rn, Rs, n_complex_dim, non_negative), kind, X sign, words of the contiguous description)
SPEC_ROWS = [
    ((12, 256, 129, 2, 8, 8, 1, NN0), "fused", "abs", ["path=slice-1pass"]),
    ((12, 256, 129, 2, 8, 8, 1, NN0), "fused", "signed", ["path=slice-1pass", "xform=signed"]),
    ((10, 256, 100, 3, 3, 5, 1, NN0), "fused", "signed", ["path=slice-1pass"]),   # W D % 4 == 0
    ((10,) + SPEC_SHAPES[1][1:], "fused", "signed", ["1pass"]),
    ((10,) + SPEC_SHAPES[1][1:], "lockstep", "signed", ["path=fused-1pass-mfma"]),   # k_spec_fused's training mode
    ((12,) + SPEC_SHAPES[0][1:], "generic", "signed", ["generic"]),
    ((10,) + SPEC_SHAPES[1][1:], "generic", "signed", ["path=generic-3kernel-mfma"]),
    ((9,) + SPEC_WIDE_SHAPES[1][1:], "generic", "signed", ["path=generic-3kernel-mfma", "vec=1"]),  # W D % 4 == 0
]


def _spec_cells():
    out = []
    for i, (case, kind, sign, words) in enumerate(SPEC_ROWS):
        for lay in _layouts(case[0], case[1:3]):
            out.append(pytest.param(i, lay, id=f"{'x'.join(map(str, case[:7]))}-{kind}-{sign}-{lay}"))
    return out


@pytest.mark.parametrize("i,layout", _spec_cells())
def test_spectral(i, layout):
    """k_spec_slice (its signed X form chosen on a view), k_spec_fused, and the generic kernels in their
    vector (fwd4 / bwd4) and, under odd strides, scalar forms; `win` is stride D.  The raw buffers include
    the predict model's output and the latents on the view."""
    case, kind, sign, words = SPEC_ROWS[i]
    N, W, D = case[:3]
    row = ("spec", case[:7], sign)
    draw = (lambda n, g: torch.randn(n, generator=g).abs()) if sign == "abs" else None
    lay, xkey = _layout(row, layout, N, (W, D), draw=draw)
    with spec_path(kind):
        rv = _spec_run(_device_view(lay), case)
        ckey = (xkey, kind)
        if ckey not in _CONTIG:
            _CONTIG[ckey] = _spec_run(lay.X.to(DEV), case)
        rc = _CONTIG[ckey]
    for w in words:
        assert w in rc["describe"], (w, rc["describe"])
    if sign == "abs":
        assert "xform=signed" not in rc["describe"] and "xform=signed" not in rv["describe"], rv["describe"]
    assert ("xform=signed" in rv["describe"]) == ("xform=signed" in rc["describe"]), rv["describe"]
    want = expect(lay.P, layout, lay.stride)
    if want == "oracle":
        assert sr.word(rv["describe"], "vec") == "0" and sr.word(rc["describe"], "vec") == "1", rv["describe"]
    _judge(rv, rc, want, _spec_bars(lay.X, case, xkey), (case[:7], kind, sign, layout))


# =====================================================================================================
# (d) hierarchical resident fit
# =====================================================================================================
HIER = dict(N=50, F=(8, 12), C=4, rank=3, iters=40)


def _hier_model(X, seed=0):
    from tensor_regression_amd.multinomial_tensor_regression_hierarchical import CP_logistic_regression
    g = torch.Generator().manual_seed(_seed("hier", seed))
    N, C, R = X.shape[0], HIER["C"], HIER["rank"]
    y = torch.randint(0, C, (N,), generator=g)
    y[:C] = torch.arange(C)
    Bcp = [(torch.randn(d, R, generator=g) * 0.3).to(DEV).requires_grad_(True) for d in (*HIER["F"], C)]
    return CP_logistic_regression(X, y.to(DEV), rank=R, Bcp_init=Bcp, device=DEV)


_HIER_FIT = dict(lambda_L2=0.01, max_iter=HIER["iters"], tol=0.0, patience=100, Adam_kwargs={"lr": 0.02})


@pytest.mark.parametrize("layout", ["pad4", "pad5", "win"])
def test_resident_fit_on_a_view(layout):
    """k_mnl_resident reads its rows through x_row_stride: the module hands the view to the kernel as it is
    (asserted: the device X keeps the layout's stride), and the loss history and the final factors are
    bitwise the contiguous copy's"""
    lay, _ = _layout(("hier",), layout, HIER["N"], HIER["F"])
    rv = sr.run_resident(_hier_model(_device_view(lay)), **_HIER_FIT)
    rc = sr.run_resident(_hier_model(lay.X.to(DEV)), **_HIER_FIT)
    assert "fit=resident" in rv["describe"] and "fit=resident" in rc["describe"], rv["describe"]
    assert rv["x_stride"] == lay.stride and rc["x_stride"] == lay.P
    assert len(rv["loss"]) == HIER["iters"] and not sr.has_nan(rv["loss"])
    assert sr.same_bits(rv["loss"], rc["loss"])
    for a, b in zip(rv["factors"], rc["factors"]):
        assert not sr.has_nan(a) and sr.same_bits(a, b)


def test_resident_many_on_views():
    """k_mnl_resident_many with one contiguous member, one pad5 and one win: x_row_stride per member"""
    from tensor_regression_amd.multinomial_tensor_regression_hierarchical import fit_Adam_many
    lays = [_layout(("hier",), lay, HIER["N"], HIER["F"])[0] for lay in ("pad4", "pad5", "win")]
    out = []
    for views in (True, False):
        Xs = [lays[0].X.to(DEV)] + [(_device_view(l) if views else l.X.to(DEV)) for l in lays[1:]]
        models = [_hier_model(X, seed=j) for j, X in enumerate(Xs)]
        report = {}
        fit_Adam_many(models, report=report, **_HIER_FIT)
        assert report["batched"] == [0, 1, 2] and report["alone"] == [], report
        strides = [int(m._device_data()[1].stride(0)) for m in models]
        assert strides == ([lays[0].P, lays[1].stride, lays[2].stride] if views else [lays[0].P] * 3), strides
        out.append(models)
    for mv, mc in zip(*out):
        assert len(mv.loss_running) == HIER["iters"] and not sr.has_nan(np.asarray(mv.loss_running))
        assert sr.same_bits(np.asarray(mv.loss_running), np.asarray(mc.loss_running))
        for a, b in zip(mv.Bcp, mc.Bcp):
            assert not sr.has_nan(a) and sr.same_bits(a, b)


# =====================================================================================================
# (e) one plan moved between strides
# =====================================================================================================
SEQUENCE = ["contig", "pad5", "ovl4", "contig", "pad4", "win", "contig"]


def _moved(row, N, F, make_plan, run, ctx, draw=None):
    """One plan through SEQUENCE: after each step its buffers and strategy words are those of a fresh plan
    given only that layout, and every return to contiguous restores the creation-time text exactly."""
    with ctx:
        plan = make_plan()
        created = plan.describe
        try:
            for step, name in enumerate(SEQUENCE):
                lay, _ = _layout(row, "pad4" if name == "contig" else name, N, F, draw=draw)
                X = lay.X.to(DEV) if name == "contig" else _device_view(lay)
                got = run(X, plan)
                fresh = run(X, None)
                assert sr.strategy_words(got["describe"]) == sr.strategy_words(fresh["describe"]), \
                    (step, name, got["describe"], fresh["describe"])
                bg, bf = sr.buffers(got), sr.buffers(fresh)
                for k in bf:
                    assert not sr.has_nan(bg[k]), (step, name, k)
                    assert sr.same_bits(bg[k], bf[k]), (step, name, k, got["describe"])
                if name == "contig":
                    assert got["describe"] == created, (step, got["describe"], created)
                else:
                    assert (got["describe"] == created) == (sr.strategy_words(got["describe"]) == sr.strategy_words(created))
        finally:
            plan.destroy()


@pytest.mark.parametrize("shape,rank,path_word", [((130, 16, 16), 8, "path=fused-1pass"),
                                                  ((40, 64, 64, 32), 16, "path=cluster-1pass")])
def test_linear_plan_moved_between_strides(shape, rank, path_word):
    from tensor_regression_amd import _engine, _lib
    nn = _lin_params(shape, rank)[0]

    def make():
        p = _engine.Plan(_lib.TR_MODEL_LINEAR, list(shape[1:]), 1, rank, shape[0], nn, None, DEV)
        assert path_word in p.describe, p.describe
        return p
    _moved(("lin", shape, rank), shape[0], tuple(shape[1:]), make,
           lambda X, plan: _lin_run(X, shape, rank, plan=plan), path("auto"))


@pytest.mark.parametrize("shape,C,rank,form", [((100, 128, 64), 10, 8, "form=rankblock"),
                                               ((200, 96, 64), 7, 3, "form=bf16split")])
def test_multinomial_plan_moved_between_strides(shape, C, rank, form):
    from tensor_regression_amd import _engine, _lib
    nn = _mnl_params(shape, C, rank)[0]

    def make():
        p = _engine.Plan(_lib.TR_MODEL_MULTINOMIAL, list(shape[1:]), C, rank, shape[0], nn, None, DEV)
        assert form in p.describe, p.describe
        return p
    _moved(("mnl", shape, C, rank), shape[0], tuple(shape[1:]), make,
           lambda X, plan: _mnl_run(X, shape, C, rank, plan=plan), path("auto"))


def test_spectral_slice_plan_moved_between_strides():
    from tensor_regression_amd import _engine
    case = SPEC_ROWS[1][0]
    N, W, D, O, Rn, Rs, ncd, nn = case

    def make():
        p = _engine.SpectralPlan(W, D, O, Rn, Rs, ncd + 1, N, nn, None, DEV)
        assert "path=slice-1pass" in p.describe, p.describe
        return p

    def run(X, plan):
        res = _spec_run(X, case, plan=plan)
        # the slice kernel's signed form is a property of X, appended behind the plan's own text
        assert res["describe"].endswith(" xform=signed"), res["describe"]
        res["describe"] = res["describe"][:-len(" xform=signed")]
        return res
    _moved(("spec", case[:7], "signed"), N, (W, D), make, run, spec_path("fused"))


def _win_series(T, D, seed):
    g = torch.Generator().manual_seed(_seed("series", T, D, seed))
    return torch.randn(T, D, generator=g).to(DEV), g


def test_linear_model_fit_on_a_window_then_its_copy():
    from tensor_regression_amd import CP_linear_regression, util
    from tensor_regression_amd import standard_tensor_regression as S
    S._plan_cache.clear()
    Xs, g = _win_series(300, 32, 0)
    y = torch.randn(300, generator=g).to(DEV)
    Xw, yw = util.windowed_view(Xs, y, (-8, 8))
    Xm = Xw.contiguous()
    assert Xw.stride(0) == 32 and Xw.shape[1:] == (16, 32)
    kw = dict(lambda_L2=0.01, max_iter=12, tol=0, patience=10, Adam_kwargs={"lr": 0.01})
    models = []
    for first in (Xw, Xm):
        torch.manual_seed(11)
        m = CP_linear_regression(Xw.shape, rank=4, device=DEV)
        m.fit_Adam(first, yw, **kw)
        pv, pm = m.predict(Xw), m.predict(Xm)  # through the model's cached plan: view, then copy
        assert sr.same_bits(pv, pm) and not sr.has_nan(pv)
        m.fit_Adam(Xm, yw, **kw)
        models.append(m)
    a, b = models
    assert len(a.loss_running) == 24 and sr.same_bits(np.asarray(a.loss_running), np.asarray(b.loss_running))
    for u, v in zip(a.Bcp + [a.bias], b.Bcp + [b.bias]):
        assert sr.same_bits(u, v) and not sr.has_nan(u)
    S._plan_cache.clear()


def test_multinomial_model_fit_on_a_window_then_its_copy():
    from tensor_regression_amd import CP_logistic_regression, util
    Xs, g = _win_series(263, 64, 1)
    lab = torch.randint(0, 3, (263,), generator=g)
    lab[:3] = torch.arange(3)
    Xw, lw = util.windowed_view(Xs, lab, (0, 64))
    Xm = Xw.contiguous()
    assert Xw.stride(0) == 64 and Xw.shape == (200, 64, 64)
    kw = dict(lambda_L2=0.01, max_iter=10, tol=0, patience=10, weights=np.array([0.7, 1.0, 1.4]),
              Adam_kwargs={"lr": 0.01})
    models = []
    for first in (Xw, Xm):
        torch.manual_seed(12)
        m = CP_logistic_regression(first, lw.numpy(), rank=2, device=DEV)
        m.fit_Adam(**kw)
        assert "mnl-fused-1pass" in m._plan.describe, m._plan.describe
        pv, pm = m.predict(Xw)[0], m.predict(Xm)[0]
        assert sr.same_bits(pv, pm) and not sr.has_nan(pv)
        m.X = Xm
        m.fit_Adam(**kw)
        models.append(m)
    a, b = models
    assert len(a.loss_running) == 20 and sr.same_bits(np.asarray(a.loss_running), np.asarray(b.loss_running))
    for u, v in zip(a.Bcp, b.Bcp):
        assert sr.same_bits(u, v) and not sr.has_nan(u)


def test_spectral_model_fit_on_a_window_then_its_copy():
    from tensor_regression_amd import util
    from tensor_regression_amd import spectral_tensor_regression as SP
    SP._plan_cache.clear()
    Xs, g = _win_series(223, 16, 2)
    y2 = torch.randn(223, 2, generator=g).to(DEV)
    Xw, yw = util.windowed_view(Xs, y2, (0, 24))
    Xm = Xw.contiguous()
    assert Xw.stride(0) == 16 and Xw.shape == (200, 24, 16)
    kw = dict(lambda_L2=0.01, max_iter=10, tol=0, patience=10, Adam_kwargs={"lr": 0.01})
    models = []
    for first in (Xw, Xm):
        torch.manual_seed(13)
        m = SP.CP_linear_regression(Xw.shape, yw.shape, rank_normal=2, rank_spectral=2, n_complex_dim=1, device=DEV)
        m.fit_Adam(first, yw, **kw)
        pv, pm = m.predict(Xw), m.predict(Xm)
        assert sr.same_bits(pv, pm) and not sr.has_nan(pv)
        assert sr.same_bits(m.predict_latents(Xw), m.predict_latents(Xm))
        m.fit_Adam(Xm, yw, **kw)
        models.append(m)
    a, b = models
    assert len(a.loss_running) == 20 and sr.same_bits(np.asarray(a.loss_running), np.asarray(b.loss_running))
    for u, v in zip(list(a.Bcp_n) + list(a.Bcp_c) + [a.bias], list(b.Bcp_n) + list(b.Bcp_c) + [b.bias]):
        assert sr.same_bits(u, v) and not sr.has_nan(u)
    SP._plan_cache.clear()


def test_misaligned_view_with_an_aligned_stride():
    """X 4 bytes past a 16-byte boundary with stride % 4 == 0: the plan refuses it (TR_E_ARG, the alignment
    message) before any launch; the model API copies it (as_device_rows) and gives the contiguous result."""
    from tensor_regression_amd import CP_linear_regression, _engine, _lib
    from tensor_regression_amd import standard_tensor_regression as S
    shape, rank = (60, 16, 16), 3
    g = torch.Generator().manual_seed(_seed("misaligned"))
    base = torch.randn(60 * 260 + 8, generator=g).to(DEV)
    Xv = torch.as_strided(base, shape, (260, 16, 1), 1)
    assert Xv.data_ptr() % 16 == 4 and Xv.stride(0) % 4 == 0
    with path("auto"):
        plan = _engine.Plan(_lib.TR_MODEL_LINEAR, [16, 16], 1, rank, 60, [False, False], None, DEV)
        arena = torch.zeros(plan.num_params, device=DEV)
        grad = torch.full((plan.num_grads,), 7.0, device=DEV)
        y = torch.zeros(60, device=DEV)
        w = torch.ones(rank, device=DEV)
        with pytest.raises(ValueError, match="16-byte aligned"):
            plan.loss_grad(Xv, y, None, 60.0, arena, w, grad)
        out = torch.full((60,), 7.0, device=DEV)
        with pytest.raises(ValueError, match="16-byte aligned"):
            plan.forward(Xv, arena, w, out=out)
        torch.cuda.synchronize()
        assert bool((grad == 7.0).all()) and bool((out == 7.0).all()), "a kernel ran on the refused X"
        plan.destroy()
        yv = torch.randn(60, generator=g).to(DEV)
        res = []
        for XX in (Xv, Xv.contiguous()):
            assert _engine.as_device_rows(XX, 0).data_ptr() % 16 == 0
            torch.manual_seed(14)
            m = CP_linear_regression(shape, rank=rank, device=DEV)
            m.fit_Adam(XX, yv, lambda_L2=0.01, max_iter=5, tol=0, patience=10, Adam_kwargs={"lr": 0.01})
            res.append((np.asarray(m.loss_running), m.predict(XX)))
        assert sr.same_bits(res[0][0], res[1][0]) and sr.same_bits(res[0][1], res[1][1])
    S._plan_cache.clear()


def test_stride_argument_checks():
    from tensor_regression_amd import _engine, _lib
    lib = _lib.load()
    plan = _engine.Plan(_lib.TR_MODEL_LINEAR, [16, 16], 1, 3, 8, [False, False], None, DEV)
    before = plan.describe
    assert lib.tr_plan_set_x_stride(plan.h, ctypes.c_int64(-1)) < 0
    assert "stride must be >= 0" in lib.tr_last_error().decode()
    assert lib.tr_plan_describe(plan.h).decode() == before
    plan.destroy()
    conv = _engine.ConvPlan(5, 12, 2, 2, 2, 1, 64, [False, False, False], None, DEV)
    before = conv.describe
    assert lib.tr_plan_set_x_stride(conv.h, ctypes.c_int64(11)) < 0
    assert "n_d" in lib.tr_last_error().decode()
    assert lib.tr_plan_set_x_stride(conv.h, ctypes.c_int64(16)) == 0
    assert lib.tr_plan_describe(conv.h).decode() == before  # a conv plan's text names no stride-dependent choice
    conv.destroy()


# =====================================================================================================
# (f) rows more than 2 GiB apart
# =====================================================================================================
def _far_view(X):
    """X (3, *F) placed 2 GiB + 16 B apart in one uninitialised allocation of about 6 GiB, row 0 2 GiB in;
    NaN around every row and at the places a 32-bit byte offset would read rows 1 and 2 from."""
    N, F = X.shape[0], tuple(X.shape[1:])
    P = sr.volume(F)
    assert N == 3
    big = torch.empty(sr.far_total(P), dtype=torch.float32, device=DEV)
    for a, b in sr.far_canary_ranges(P):
        big[a:b] = float("nan")
    for n in range(N):
        at = sr.FAR_OFFSET + n * sr.FAR_STRIDE
        big[at:at + P] = X[n].reshape(-1).to(DEV)
    inner = torch.empty(F).stride()
    Xv = torch.as_strided(big, (N, *F), (sr.FAR_STRIDE, *inner), sr.FAR_OFFSET)
    assert Xv.data_ptr() % 16 == 0 and torch.equal(Xv.cpu(), X)
    return big, Xv


FAR_CASES = ["packed-guard", "fused", "twopass", "bsp", "spectral"]


@pytest.mark.parametrize("case", FAR_CASES)
def test_rows_2gib_apart(case):
    """Row address arithmetic is 64-bit in every kernel read for this test (k_linear_fused: row * xld * 4 in
    int64 into the row descriptor's base; k_rows / k_cols / k_rows_mfma: int64 row * (xld / W); the
    multinomial kernels: X + int64 sample * xld as the scalar base of 32-bit in-sample offsets; the
    spectral kernels: X + int64 n * xld) and k_linear_packed, whose per-lane offset is 32-bit, is guarded:
    the plan hands such rows to k_linear_fused (the named exception: no ` pk=`, and W and the kernel
    differ from the contiguous plan's, so the oracle bars apply)."""
    g = torch.Generator().manual_seed(_seed("far", case))
    try:
        if case in ("packed-guard", "fused", "twopass"):
            shape, rank = ((3, 4, 5), 3) if case == "packed-guard" else ((3, 32, 32), 3)
            X = torch.randn(*shape, generator=g)
            big, Xv = _far_view(X)
            with path("twopass" if case == "twopass" else "auto"):
                rv = _lin_run(Xv, shape, rank, calls=2)
                rc = _lin_run(X.to(DEV), shape, rank, calls=2)
            if case == "packed-guard":
                assert " pk=" in rc["describe"] and " pk=" not in rv["describe"], (rv["describe"], rc["describe"])
                assert "path=fused-1pass" in rv["describe"], rv["describe"]
                _judge(rv, rc, "oracle", _lin_bars(X, shape, rank, ("far", case)), case)
            else:
                assert ("path=fused-1pass" if case == "fused" else "path=2pass") in rv["describe"], rv["describe"]
                _judge(rv, rc, "bitwise", None, case)
        elif case == "bsp":
            shape, C, rank = (3, 64, 64), 3, 2
            X = torch.randn(*shape, generator=g)
            big, Xv = _far_view(X)
            with path("auto"):
                rv = _mnl_run(Xv, shape, C, rank)
                rc = _mnl_run(X.to(DEV), shape, C, rank)
            assert "form=bf16split" in rv["describe"], rv["describe"]
            _judge(rv, rc, "bitwise", None, case)
        else:
            sc = (3, 24, 17, 2, 2, 2, 1, NN0)
            X = torch.randn(3, 24, 17, generator=g)
            big, Xv = _far_view(X)
            with spec_path("fused"):
                rv = _spec_run(Xv, sc)
                rc = _spec_run(X.to(DEV), sc)
            assert "generic" not in rv["describe"], rv["describe"]
            _judge(rv, rc, "bitwise", None, case)
    finally:
        big = Xv = None
        torch.cuda.empty_cache()
