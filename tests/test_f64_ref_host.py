"""CPU self-check of the acceptance rule of tests/f64_ref.py, on every sweep case of tests/test_gpu_f64.py
with the same seeds: the rule lets two independent correct fp64 evaluations through (the oracle's closed
form in numpy's own BLAS / pairwise order, and torch autograd in float64), rejects two evaluations that
are contaminated with a single fp32-rounded quantity, and its yardstick stays small."""
import numpy as np
import pytest
import torch

import f64_ref as fr
from oracle import cp_oracle

DRAWS = [(c, s, None) for c, s in fr.SWEEP] + fr.STRIDED
IDS = [f"case{c}-{s}" + ("" if pad is None else f"-pad{pad}") for c, s, pad in DRAWS]


def _args(inp, sp=None):
    return (inp["X"], inp["y"], inp["Bcp"], inp["bias"], inp["w"], inp["nn"], inp["lam"], inp["sp"] if sp is None else sp)


def _with_data_loss(res, inp):
    """closed_form_linear returns the total only: the data loss from its own y_hat, in its own order."""
    e = res["y_hat"] - inp["y"]
    return dict(res, data_loss=np.mean(e * e))


def test_longdouble_is_wider_or_the_fallback_is_in_force():
    if fr.LONGDOUBLE:
        assert np.finfo(np.longdouble).eps <= 2.0 ** -63
    else:
        assert fr.bound(0.0, (4099, 3, 3)) == fr.fallback_bound((4099, 3, 3)) <= fr.CAP


def test_cases_are_the_table():
    """A typo in a shape cannot move a case off its branch silently."""
    assert sorted(fr.CASES) == list(range(1, 24))
    assert [fr.CASES[c][0][1] for c in range(3, 13)] == [63, 64, 65, 127, 128, 129, 192, 193, 256, 257]
    assert fr.non_negative_of(1) == [True, False] and fr.non_negative_of(14) == [False, True, False]
    assert fr.non_negative_of(3) == [True] and fr.non_negative_of(4) == [False]
    assert fr.non_negative_of(11) == [True] and fr.non_negative_of(12) == [False]
    assert len(fr.CASES[23][0]) - 1 == 8 and len(fr.SWEEP) == 27
    for c in fr.CASES:
        inp = fr.make_inputs(c)
        for f, A in enumerate(inp["Bcp"]):
            if inp["nn"][f]:  # a * beta on both sides of the threshold, and the two far entries
                ab = A.reshape(-1) * inp["sp"]["beta"]
                assert ab.min() == -40.0 and ab.max() == 40.0
                mid, thr = ab[1:-1], inp["sp"]["threshold"]
                assert mid.size < 2 or ((mid > thr).any() and (mid < thr).any()), (c, f)


@pytest.mark.parametrize("case,sp,pad", DRAWS, ids=IDS)
def test_rule_admits_correct_fp64_and_rejects_fp32_contamination(case, sp, pad):
    inp, ref, yard = fr.reference_of(case, sp, pad)
    shape = inp["shape"]
    tag = f"case {case} {sp}" + ("" if pad is None else f" pad {pad}")
    if pad is not None:  # the view of the base is the X the references saw
        P = int(np.prod(shape[1:]))
        view = np.lib.stride_tricks.as_strided(inp["base"], (shape[0], P), (8 * (P + pad), 8))
        assert inp["row_stride"] == P + pad and np.array_equal(view.reshape(shape), inp["X"])
    # the yardstick itself
    _, seen = fr.check(tag + " yard", yard, ref, yard, shape, verbose=False)
    for k, e, ey in seen:
        print(f"{tag} {k}: e_yard {ey:.3e}")
        assert ey <= fr.YARD_MAX, (case, k, ey)
    # two independent correct evaluations pass
    cf = _with_data_loss(cp_oracle.closed_form_linear(*_args(inp)), inp)
    bad, _ = fr.check(tag + " closed_form_linear", cf, ref, yard, shape)
    assert not bad, bad
    ag = cp_oracle.linear_loss_grad(*_args(inp), dtype=torch.float64)
    bad, _ = fr.check(tag + " autograd", ag, ref, yard, shape)
    assert not bad, bad
    if not fr.LONGDOUBLE:
        return  # (the fixed fallback bound is not asked to separate contaminations)
    # one fp32-rounded quantity fails: softplus parameters (where a factor is flagged and they are not fp32 numbers)
    if any(inp["nn"]) and sp == "odd":
        c1 = _with_data_loss(cp_oracle.closed_form_linear(*_args(inp, fr.round_softplus32(inp["sp"]))), inp)
        bad, _ = fr.check(tag + " softplus32", c1, ref, yard, shape, verbose=False)
        assert "y_hat" in [b[0] for b in bad] and any(b[0].startswith("grads") for b in bad), bad
    # ... and X.B from float32-rounded B, in every case
    c2 = fr.closed_form_fp64_rounded_dense(*_args(inp))
    bad, _ = fr.check(tag + " dense32", c2, ref, yard, shape, verbose=False)
    assert "y_hat" in [b[0] for b in bad] and "data_loss" in [b[0] for b in bad], bad
