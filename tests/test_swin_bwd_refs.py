"""CPU: the premises of tests/test_gpu_swin_bwd.py.  The formulas of include/vkn_wattn_train.h, written out per window in
tests/swin_bwd_ref.py, against float64 autograd of the restatement `swin_ref.core` on every core case, to 1e-12 relative: dqkv, the table,
and the bias gradient in its two parts (pad tokens, real tokens).  And the premise of the addressing test: on the five single-offset
selector cases, with dout zeroed on undecided queries and on queries won by a pad token, every non-zero dv row is exactly one dout row."""
import pytest
import torch

import swin_bwd_ref as G
import swin_ref as R


def _close(got, want, what):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert err <= 1e-12 * max(scale, 1e-300), f'{what}: error {err:.3e} against a largest magnitude of {scale:.3e}'


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_formulas_equal_float64_autograd(name):
    case = R.core_case(name)
    dout = G.seeded_dout(case)
    got, want = G.run_formulas(case, dout), G.autograd_grads(case, dout)
    assert got['dqkv'].shape == case['qkv'].shape and got['dtable'].shape == case['table'].shape
    _close(got['dqkv'], want['dqkv'], f'{name}: dqkv')
    _close(got['dtable'], want['dtable'], f'{name}: dbias_table')
    _close(got['dbias_pad'] + got['dbias_real'], want['dbias_total'], f'{name}: the whole bias gradient')
    C = case['heads'] * R.HD
    if case['qkv_bias'] is None:
        assert not got['dbias_pad'].any() and not want['dbias_pad'].any()
    else:
        _close(got['dbias_pad'], want['dbias_pad'], f'{name}: the pad part of the bias gradient')
    assert not got['dbias_pad'][:C].any() and not want['dbias_pad'][:C].any()            # a pad query is cropped: the q third is exactly zero
    # the real part is the sum of dqkv's rows: what the qkv Linear's backward adds
    _close(got['dbias_real'], want['dqkv'].reshape(-1, 3 * C).sum(0), f'{name}: the real part of the bias gradient')
    pads = (case['H'] % case['window'] != 0 or case['W'] % case['window'] != 0) and case['qkv_bias'] is not None
    assert bool(want['dbias_pad'][C:].any()) == pads, 'a padded case with a bias has a pad part, no other case has'


def test_the_cases_cover_the_pad_part_and_both_arms():
    padded = [n for n, (B, H, W, ws, shift, heads, opt) in R.CORE_CASES.items() if (H % ws or W % ws) and opt.get('bias', True)]
    assert {'pad_both', 'pad_both_shift', 'small_map', 'scores80'} <= set(padded)
    assert R.CORE_CASES['no_bias_padded'][6] == dict(bias=False) and R.CORE_CASES['no_bias_padded'][1] % 7
    assert all(R.CORE_CASES[n][0] * R.CORE_CASES[n][1] * R.CORE_CASES[n][2] <= 2 * 14 * 21 for n in R.CORE_CASES)


@pytest.mark.parametrize('name', G.ADDRESSING_CASES)
def test_addressing_premise(name):
    """float64 autograd, rounded to fp32 (what is below 1e-45 there, exp(-150) and less, is zero): a dv row is zero or one dout row"""
    case, dout = G.addressing_case(name)
    heads = case['heads']
    assert len(R.SELECTOR_CASES[name][6]) == 1
    dv = G.autograd_grads(case, dout)['dqkv'][:, :, :, 2].float().reshape(-1, heads, R.HD)          # [tokens, heads, 32]
    rows = dout.reshape(-1, heads, R.HD)
    live = dv.abs().amax(-1) > 0
    assert int(live.sum()) == G.ADDRESSING_ROWS[name] > 0
    for m in range(heads):
        pool = rows[:, m]
        for r in dv[live[:, m], m]:
            assert int((pool == r).all(-1).sum()) == 1
    # the q and k thirds are far below fp32 there: the addressing test leaves them to the per-element test
    g = G.autograd_grads(case, dout)
    assert g['dqkv'][:, :, :, :2].abs().max().item() < 1e-60 and g['dtable'].abs().max().item() < 1e-60
