"""CPU: the premises of tests/test_gpu_msda_bwd.py, proved without a GPU (tests/msda_bwd_ref.py holds references, draws and premises).

  * every per-element case: no pixel coordinate within 1/64 of an integer after the nudge, the asserted band shares still >= 0.20, at
    least 30 % of doff and of dvalue non-zero (`row-130` exempt from the dvalue floor by name: 0.12);
  * the two float64 forms' gradients (explicit corners, grid_sample) agree to 1e-12 of each tensor's largest magnitude;
  * the exact cases: the float64 gradients are fp32 numbers on the grids 2^-10 (dvalue, doff) / 2^-12 (dlogits), and every partial
    sum fits 24 bits in any order."""
import pytest
import torch

import msda_bwd_ref as RB
import msda_ref as R

PER_ELEMENT = ('shipped-89', 'q5-of-89', 'm4-d64', 'm8-d16', 'l1-p1', 'l4-p8', 'one-pixel', 'row-130', 'spread-80', 'spread-100')


def _seed(name):
    return 5100 + list(R.CORE_CASES).index(name)


@pytest.mark.parametrize('name', PER_ELEMENT)
def test_premises_and_the_two_float64_forms(name):
    case = R.CORE_CASES[name]
    value, off, logits, ref, dout = RB.draw_core_bwd(case, _seed(name))
    assert dout.shape == (case.B, case.Q, case.M * case.D) and all(t.dtype == torch.float32 for t in (value, off, logits, ref, dout))
    want = RB.reference(case, value, off, logits, ref, dout)
    facts = RB.premises(name, case, off, ref, want)                                # raises PremiseError
    assert facts['min_distance'] >= RB.NEAR and facts['nonzero_doff'] >= 0.3
    other = RB.reference_grid_sample(case, value, off, logits, ref, dout)
    for label, a, b, like in zip(('dvalue', 'doff', 'dlogits'), want, other, (value, off, logits)):
        assert a.shape == b.shape == like.shape and a.dtype == torch.float64
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(a.abs().max())), (name, label)
    if len(case.shapes) * case.P == 1:
        assert not bool(want[2].any())                                             # one point: its softmax weight is the constant 1
    else:
        assert float(want[2].abs().max()) > 1e-3
    yard = RB.yardstick(case, value, off, logits, ref, dout)
    for a, y in zip(want[:2], yard[:2]):
        bound, err = R.bound(a, y)
        assert 0 < err < 1e-2 and bound >= 4 * R.ulp32(a.abs().max())


def test_the_nudge_moves_only_what_is_near_an_integer():
    case = R.CORE_CASES['shipped-89']
    value, off, logits, ref = R.draw_core(case, _seed('shipped-89'))
    moved = RB.nudge(case.shapes, off, ref)
    near = RB.integer_distance(case.shapes, off, ref) < RB.NEAR
    assert torch.equal(moved[~near], off[~near]) and float(RB.integer_distance(case.shapes, moved, ref).min()) >= RB.NEAR
    assert RB.DVALUE_FLOOR_EXEMPT == ('row-130',)
    with pytest.raises(R.PremiseError):
        zero = torch.zeros_like(off)                                                # every point on a pixel centre: distance 0
        RB.premises('shipped-89', case, zero, ref, RB.reference(case, value, zero, logits, ref, torch.ones(case.B, case.Q, case.M * case.D)))


@pytest.mark.parametrize('name', list(R.EXACT_CASES))
def test_exact_cases_backward_is_exact_in_fp32(name):
    case = R.EXACT_CASES[name]
    value, off, logits, ref, dout = RB.draw_exact_bwd(case, 5200 + list(R.EXACT_CASES).index(name))
    want = RB.exact_premise_bwd(name, case, value, off, logits, ref, dout)         # raises PremiseError
    assert [tuple(w.shape) for w in want] == [tuple(t.shape) for t in (value, off, logits)]
    # torch's own fp32 backward is no witness here: its grid_sample coordinates (2 loc - 1, un-normalised again) round, and doff is
    # discontinuous at the integer coordinates these cases hit; the dvalue it scatters with exact weights is
    got = RB.yardstick(case, value, off, logits, ref, dout)
    assert got[0].dtype == torch.float32 and float((got[0].double() - want[0]).abs().max()) <= 1e-3 * float(want[0].abs().max())
    x, _ = R.pixel_coords(case.shapes, off.double(), ref.double())
    assert float((x == x.floor()).double().mean()) > 0.1 and float((x != x.floor()).double().mean()) > 0.3      # integer coordinates AND fractions
    with pytest.raises(R.PremiseError):
        RB.exact_premise_bwd(name, case, value, off, logits, ref, dout + 0.5)
