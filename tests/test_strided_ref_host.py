"""CPU checks of tests/strided_ref.py: the layouts are what they claim, the comparison the GPU tests use
(same_bits against the contiguous copy) rejects every mistake a strided row reader can make, the
strategy-word extractor reads the library's description strings, and the alias arithmetic of the
rows-2-GiB-apart case lands where the test puts its canaries."""
import numpy as np
import pytest
import torch

import strided_ref as sr

SHAPES = [(5, (4, 5)), (3, (3, 3)), (4, (16, 16)), (3, (11, 13)), (6, (33,)), (2, (6, 7, 8, 3)), (7, (8, 12)),
          (2, (2, 2))]
CASES = [(lay, N, F) for N, F in SHAPES for lay in sr.LAYOUTS if sr.applies(lay, N, F)]


def test_every_layout_occurs():
    assert {c[0] for c in CASES} == set(sr.LAYOUTS)
    assert not sr.applies("win", 5, (33,)) and not sr.applies("ovl4", 5, (2, 2)) and not sr.applies("ovl3", 5, (3,))
    assert not sr.applies("pad4", 1, (4, 5)) and sr.applies("one", 1, (4, 5))


@pytest.mark.parametrize("layout,N,F", CASES)
def test_layout_is_what_it_claims(layout, N, F):
    from tensor_regression_amd._engine import _rows_contiguous
    lay = sr.build(layout, N, F, seed=3)
    P = sr.volume(F)
    v = sr.view_of(lay)
    assert lay.base.ndim == 1 and lay.base.dtype == torch.float32
    assert tuple(v.shape) == ((1 if layout == "one" else N), *F)
    assert sr.same_bits(v.contiguous(), lay.X) and not sr.has_nan(lay.X)
    assert lay.X.is_contiguous() and lay.X.stride(0) == P  # (a plain clone of an overlapping view is permuted)
    assert _rows_contiguous(v)
    assert v.stride(0) == lay.stride == sr.row_stride(layout, F)
    m = sr.row_mask(lay)
    b = lay.base.numpy()
    assert not np.isnan(b[m]).any(), "a canary inside a row"
    assert np.isnan(b[~m]).all(), "a float outside every row that is no canary"
    before, after = sr.guard_bands(lay)
    assert before >= P and after >= P
    assert m[before] and not m[:before].any() and not m[len(m) - after:].any()
    # where row 0 starts, in a 16-B aligned base
    assert lay.base.data_ptr() % 16 == 0
    assert lay.offset % 4 == (1 if layout == "off1" else 0)
    if layout in ("pad4", "pad5", "off1"):
        assert (~m[before:len(m) - after]).any(), "no gap between the rows"
    if layout in sr.OVERLAPPING:
        assert lay.stride < P
    if layout == "win":  # what util.windowed_view makes of the series
        from tensor_regression_amd import util
        D = sr.volume(F[1:])
        series = lay.base[lay.offset:lay.offset + (N - 1) * D + P].reshape(N + F[0] - 1, *F[1:])
        Xw, _ = util.windowed_view(series, torch.zeros(series.shape[0]), (0, F[0]))
        assert tuple(Xw.shape) == tuple(v.shape) and Xw.stride() == v.stride() and torch.equal(Xw, v)


def test_given_X_is_placed_and_overlapping_layouts_refuse_it():
    X = torch.arange(40, dtype=torch.float32).reshape(2, 4, 5)
    lay = sr.build("pad5", 2, (4, 5), X=X)
    assert torch.equal(sr.view_of(lay), X)
    with pytest.raises(ValueError):
        sr.build("ovl4", 2, (4, 5), X=X)
    with pytest.raises(ValueError):
        sr.build("win", 3, (33,))


def test_draw_shapes_the_values():
    lay = sr.build("win", 4, (8, 5), draw=lambda n, g: torch.randn(n, generator=g).abs() * 3e7)
    assert lay.X.min() >= 0 and lay.X.max() > 1e7


def _contig(lay):
    """The contiguous copy as a layout of its own (stride P, no canaries between the rows)."""
    return lay.X.reshape(-1).numpy(), 0, lay.P


@pytest.mark.parametrize("layout,N,F", CASES)
def test_correct_reader_matches_the_contiguous_copy(layout, N, F):
    lay = sr.build(layout, N, F, seed=5)
    cb, co, cs = _contig(lay)
    got = sr.emulate_reader(lay.base.numpy(), lay.offset, lay.stride, lay.N, lay.P)
    want = sr.emulate_reader(cb, co, cs, lay.N, lay.P)
    assert sr.same_bits(got, want) and not sr.has_nan(got)


@pytest.mark.parametrize("bug", sr.READER_BUGS)
@pytest.mark.parametrize("layout,N,F", CASES)
def test_reader_mistakes_are_rejected(layout, N, F, bug):
    """Each mistake, made on the view only (the contiguous run is the correct reader's), fails the
    comparison wherever it changes what is read; and where the table says it cannot show, it does not."""
    lay = sr.build(layout, N, F, seed=5)
    cb, co, cs = _contig(lay)
    want = sr.emulate_reader(cb, co, cs, lay.N, lay.P)
    got = sr.emulate_reader(lay.base.numpy(), lay.offset, lay.stride, lay.N, lay.P, bug=bug)
    if sr.bug_can_show(bug, lay):
        assert not sr.same_bits(got, want), (bug, layout)
    else:
        assert sr.same_bits(got, want), (bug, layout)


@pytest.mark.parametrize("bug", sr.READER_BUGS)
def test_every_mistake_shows_on_some_layout_and_the_zero_coefficient_one_as_nan(bug):
    shown = [c for c in CASES if sr.bug_can_show(bug, sr.build(*c))]
    assert shown, bug
    if bug == "next_row_quad":  # a canary times a zero coefficient: the NaN the contract forbids
        for c in shown:
            lay = sr.build(*c)
            assert sr.has_nan(sr.emulate_reader(lay.base.numpy(), lay.offset, lay.stride, lay.N, lay.P, bug=bug))


def test_same_bits():
    a = torch.tensor([1.0, float("nan"), 0.0])
    assert sr.same_bits(a, a.clone())
    assert not sr.same_bits(a, torch.tensor([1.0, float("nan"), -0.0]))
    assert not sr.same_bits(a, a.double()) and not sr.same_bits(a, a[:2])
    assert not sr.same_bits(np.float32([1.0]), np.float32([np.nextafter(np.float32(1.0), np.float32(2.0))]))


# description strings as tr_api.hip's format strings print them
DESC_FUSED = ("model=linear K=2 C=1 R=3 P=128 nparams=73 ncu=256 path=fused-1pass T=256 CH=0 grid=2048 W=4 "
              "max_slabs=1024 workspace=1.0MiB pk=32")
DESC_CLUSTER = ("model=linear K=3 C=1 R=16 P=131072 nparams=2561 ncu=256 path=cluster-1pass T=512 CH=14 grid=255 W=4 "
                "max_slabs=32 workspace=18.1MiB S=5 clusters=51 recovered=2pass")
DESC_DUO = ("model=multinomial K=2 C=10 R=8 P=6144 nparams=1360 ncu=256 path=mnl-fused-1pass+mfma-fwd T=0 CH=0 grid=0 "
            "W=4 max_slabs=68 workspace=24.3MiB duo units=96 waves=6 wg/cu=1 nbuf=3 lds=77.5KiB form=bf16split "
            "rowblocks=2 rk=16 jt=32 xform=exact fit=resident")
DESC_MNL = ("model=multinomial K=2 C=10 R=8 P=1024 nparams=720 ncu=256 path=mnl-fused-1pass+wide-mfma T=0 CH=0 grid=0 "
            "W=1 max_slabs=409 workspace=16.9MiB units=64 nbuf=2 lds=40.0KiB")
DESC_SPEC = ("model=spectral W=24 D=17 n_out=2 Rn=2 Rs=3 Cc=2 K=8 nparams=289 ncu=256 "
             "path=slice-1pass-mfma-bf16split(predict:generic) KT=1 S=17 grid=256 lds=152.1KiB vec=1 workspace=0.3MiB "
             "slsp=1 xpieces=2 xform=signed")


def test_strategy_words():
    assert sr.strategy_words(DESC_FUSED) == ("path=fused-1pass", "T=256", "CH=0", "grid=2048", "W=4", "pk=32")
    assert sr.strategy_words(DESC_CLUSTER) == ("path=cluster-1pass", "T=512", "CH=14", "grid=255", "W=4", "S=5",
                                               "clusters=51", "recovered=2pass")
    assert sr.strategy_words(DESC_DUO) == ("path=mnl-fused-1pass+mfma-fwd", "T=0", "CH=0", "grid=0", "W=4", "duo",
                                           "units=96", "waves=6", "wg/cu=1", "nbuf=3", "lds=77.5KiB", "form=bf16split",
                                           "rowblocks=2", "rk=16", "jt=32", "xform=exact", "fit=resident")
    assert sr.strategy_words(DESC_MNL) == ("path=mnl-fused-1pass+wide-mfma", "T=0", "CH=0", "grid=0", "W=1", "units=64",
                                           "nbuf=2", "lds=40.0KiB")
    assert sr.strategy_words(DESC_SPEC) == ("W=24", "path=slice-1pass-mfma-bf16split(predict:generic)", "KT=1", "S=17",
                                            "grid=256", "lds=152.1KiB", "vec=1", "slsp=1", "xpieces=2", "xform=signed")
    # a word that changes is seen; shape, CU count and workspace size are not strategy
    assert sr.strategy_words(DESC_FUSED.replace("W=4", "W=1")) != sr.strategy_words(DESC_FUSED)
    assert sr.strategy_words(DESC_SPEC.replace("vec=1", "vec=0")) != sr.strategy_words(DESC_SPEC)
    assert sr.strategy_words(DESC_FUSED.replace("workspace=1.0MiB", "workspace=9.0MiB").replace("ncu=256", "ncu=64")) \
        == sr.strategy_words(DESC_FUSED)
    assert sr.word(DESC_FUSED, "grid") == "2048" and sr.word(DESC_FUSED, "S") is None and sr.word(DESC_DUO, "form") == "bf16split"


@pytest.mark.parametrize("P", [20, 1024, 4096, 24 * 17])
def test_far_row_aliases(P):
    """Rows 2 GiB + 16 B apart with row 0 2 GiB into the allocation: a byte offset truncated to 32 bits,
    signed or unsigned, still lands inside the allocation, on a canary or on another row's data."""
    s, o = sr.FAR_STRIDE, sr.FAR_OFFSET
    assert 4 * s == (1 << 31) + 16 and 4 * o == 1 << 31
    total = sr.far_total(P)
    assert 5.9 * 2**30 < 4 * total < 6.1 * 2**30
    rows = [(o + n * s, o + n * s + P) for n in range(3)]
    assert rows[-1][1] + P <= total
    assert sr.far_aliases(0) == (o, o)
    assert sr.far_aliases(1) == (4, o + s)            # signed: 16 B into the allocation; unsigned: not truncated
    assert sr.far_aliases(2) == (o + 8, o + 8)        # 2^32 + 32 -> 32 B into row 0
    ranges = sr.far_canary_ranges(P)
    assert sum(b - a for a, b in ranges) <= 12 * P     # a few KiB are written, not 6 GiB

    def is_canary(i):
        return any(a <= i < b for a, b in ranges)

    def in_row(i):
        return any(a <= i < b for a, b in rows)
    for a, b in ranges:
        assert 0 <= a < b <= total
        assert not in_row(a) and not in_row(b - 1), "a canary range inside a row"
    for a, b in rows:  # P canaries on either side of every row
        assert all(is_canary(i) for i in (a - P, a - 1, b, b + P - 1))
    for n in (1, 2):
        for at in sr.far_aliases(n):
            if (at, at + P) in rows:
                continue
            assert 0 <= at and at + P <= total
            for i in (at, at + P // 2, at + P - 1):  # a truncated read meets a canary or another row's data
                assert is_canary(i) or (in_row(i) and not rows[n][0] <= i < rows[n][1])
