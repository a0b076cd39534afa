"""CPU: the premises of tests/test_gpu_msda.py, proved without a GPU (tests/msda_ref.py holds references, bound and cases).

  * the explicit-corner float64 core and torch's `grid_sample` composition in float64 agree to 1e-12 on every case: the reference
    the GPU test judges against is mmcv's rule;
  * the band shares of the drawn offsets: per axis >= 20 % of the points in (-1, 0) and in [H - 1, H), >= 20 % out in x with y in,
    > 20 % failing the four comparisons;
  * the exact cases: torch's own CPU fp32 composition — whose summation order is not the kernel's — equals float64 bit for bit."""
import pytest
import torch

import msda_ref as R


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_explicit_corners_agree_with_grid_sample_in_float64(name):
    case = R.CORE_CASES[name]
    value, off, logits, ref = R.draw_core(case, 4100 + list(R.CORE_CASES).index(name))
    assert value.shape == (case.B, sum(h * w for h, w in case.shapes), case.M, case.D) and ref.shape == (case.Q, len(case.shapes), 2)
    assert off.shape == (case.B, case.Q, case.M, len(case.shapes), case.P, 2) and all(t.dtype == torch.float32 for t in (value, off, logits, ref))
    a = R.core_f64(value, case.shapes, off, logits, ref)
    b = R.core_grid_sample(value, case.shapes, off, logits, ref, torch.float64)
    assert a.shape == b.shape == (case.B, case.Q, case.M * case.D)
    assert float((a - b).abs().max()) <= 1e-12, name
    assert float(a.abs().max()) > 0.1                                              # not vacuous
    yard = R.core_grid_sample(value, case.shapes, off, logits, ref, torch.float32)
    bound, err = R.bound(a, yard)
    assert 0 < err < 1e-4 and bound >= 4 * R.ulp32(a.abs().max())


@pytest.mark.parametrize('name', R.BANDS_ASSERTED)
def test_offsets_fill_every_band(name):
    case = R.CORE_CASES[name]
    assert case.shapes == ((2, 3), (4, 5), (7, 9)) and case.Q == 89
    _, off, _, ref = R.draw_core(case, 4100 + list(R.CORE_CASES).index(name))
    shares = R.band_shares(case.shapes, off, ref)
    for k in ('low_x', 'low_y', 'high_x', 'high_y', 'xout_yin', 'fail'):
        assert shares[k] >= 0.20, (k, shares)
    assert shares['fail'] <= 0.70                                                  # ... and enough points still sample something


def test_the_spread_cases_need_the_max_subtraction():
    """+-80 stays inside fp32 (exp(80) = 5.5e34 < 3.4e38) and only thins the sum's headroom; +-100 is the case that a softmax without
    the max subtraction cannot survive: exp(100) is inf in fp32 and inf / inf a NaN"""
    for name, overflows in (('spread-80', False), ('spread-100', True)):
        case = R.CORE_CASES[name]
        _, _, logits, _ = R.draw_core(case, 4100 + list(R.CORE_CASES).index(name))
        assert float(logits.max()) > 0.9 * case.spread and float(logits.min()) < -0.9 * case.spread
        naive = logits.exp() / logits.exp().sum(-1, keepdim=True)
        assert (not torch.isfinite(naive).all()) == overflows, name
        assert torch.isfinite(logits.softmax(-1)).all()


def test_cases_cover_what_they_promise():
    c = R.CORE_CASES
    assert {(v.M, v.D) for v in c.values()} >= {(8, 32), (4, 64), (8, 16)}
    assert {(len(v.shapes), v.P) for v in c.values()} >= {(3, 4), (1, 1), (4, 8)}
    assert any(v.Q != sum(h * w for h, w in v.shapes) for v in c.values()) and any((1, 1) in v.shapes for v in c.values())
    assert any(w >= 130 for v in c.values() for _, w in v.shapes) and any(v.spread >= 80 for v in c.values())
    assert {len(v.shapes) * v.P for v in R.EXACT_CASES.values()} == {1, 2, 4} and {v.D for v in R.EXACT_CASES.values()} == {16, 32, 64}
    assert any(len(v.shapes) > 1 for v in R.EXACT_CASES.values())                  # level starts other than 0


@pytest.mark.parametrize('name', list(R.EXACT_CASES))
def test_exact_cases_fp32_equal_float64(name):
    case = R.EXACT_CASES[name]
    value, off, logits, ref = R.draw_exact(case, 4200 + list(R.EXACT_CASES).index(name))
    want = R.exact_premise(case, value, off, logits, ref)                          # raises PremiseError
    got = R.core_grid_sample(value, case.shapes, off, logits, ref, torch.float32)
    assert got.dtype == torch.float32 and torch.equal(got.double(), want), name
    x, y = R.pixel_coords(case.shapes, off.double(), ref.double())
    assert float(((x > -1) & (x < 0)).double().mean()) > 0.02 and float((x != x.floor()).double().mean()) > 0.3    # borders and fractions occur


def test_a_case_outside_its_premise_fails_as_a_test_bug():
    with pytest.raises(R.PremiseError):
        R.draw_exact(R.ExactCase(1, 8, 32, 1, ((3, 8),)), 1)                       # 3 is no power of two
    with pytest.raises(R.PremiseError):
        R.draw_exact(R.ExactCase(1, 8, 32, 3, ((4, 8),)), 1)                       # L P = 3
    case = R.EXACT_CASES['lp1']
    value, off, logits, ref = R.draw_exact(case, 1)
    with pytest.raises(R.PremiseError):
        R.exact_premise(case, value + 0.5, off, logits, ref)
    with pytest.raises(R.PremiseError):
        R.exact_premise(case, value, off + 1e-3, logits, ref)
    assert R.ulp32(1.0) == 2.0 ** -23 and R.ulp32(3.9) == 2.0 ** -22 and R.ulp32(0.75) == 2.0 ** -24
