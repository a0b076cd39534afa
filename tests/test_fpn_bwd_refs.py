"""CPU: the premises of tests/test_gpu_fpn_bwd.py, asserted on the operands it will use (tests/fpn_bwd_ref.py), and the Python surface
of the block that needs no device: the `fused_backward` keyword and the envelope predicate."""
import inspect
import os
import re

import pytest
import torch
import torch.nn.functional as F

import fpn_bwd_ref as R

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'vkn_fpn_train.h')


@pytest.mark.parametrize('name', list(R.GN_CASES))
def test_unit_cases_stay_clear_of_the_relu_edge(name):
    """every float64 pre-activation of the GroupNorm unit cases has magnitude >= 0.05, with |gamma| >= 0.5 (so that the margin is one
    on xhat as well); the fp32 statistics handed to the kernel are the float64 ones, rounded"""
    c = R.gn_case(name)
    assert float(c['pre'].abs().min()) >= R.UNIT_MARGIN and float(c['gamma'].abs().min()) >= 0.5 and float(c['beta'].abs().min()) >= R.UNIT_MARGIN * 0.999
    B, C, H, W, G = R.GN_CASES[name]
    assert c['r'].dtype == c['dy'].dtype == c['stats'].dtype == torch.float32 and tuple(c['stats'].shape) == (B, G, 2)
    mask = c['pre'] > 0
    assert torch.equal(c['ref']['y'] > 0, mask) and torch.equal(c['f32']['y'] > 0, mask)                  # the fp32 composition sees the same mask
    if C // G * H * W > 1:
        assert 0.2 < float(mask.double().mean()) < 0.8                                                    # both sides of the ReLU are there
    else:
        assert float(c['ref']['dr'].abs().max()) < 1e-12                                                  # a group of one element: dr is 0 (to float64 rounding in autograd)
    # the reference is the formula of include/vkn_fpn_train.h
    m, v = R.group_stats(c['r'].double(), G)
    rstd = (1.0 / torch.sqrt(v + R.EPS)).view(B, G, 1).expand(B, G, C // G).reshape(B, C, 1, 1)
    xh = (c['pre'] - c['beta'].double().view(1, C, 1, 1)) / c['gamma'].double().view(1, C, 1, 1)
    dz = c['dy'].double() * mask
    g = dz * c['gamma'].double().view(1, C, 1, 1)
    grp = lambda t: t.reshape(B, G, -1).mean(2).view(B, G, 1).expand(B, G, C // G).reshape(B, C, 1, 1)    # noqa: E731
    dr = rstd * (g - grp(g) - xh * grp(g * xh))
    assert float((dr - c['ref']['dr']).abs().max()) <= 1e-9 * float(g.abs().max())
    assert float(((dz * xh).sum((0, 2, 3)) - c['ref']['dgamma']).abs().max()) < 1e-9 and float((dz.sum((0, 2, 3)) - c['ref']['dbeta']).abs().max()) < 1e-9


@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_block_cases_stay_clear_of_the_relu_edge(name):
    """the seed taken clears the margin; the bound of every tensor is positive unless the tensor is exactly 0; the case covers what its
    name says (runs, chunks, groups)"""
    c = R.block_case(name)
    B, Cin, Cout, H, W, k, s, G = R.BLOCK_CASES[name]
    assert c['seed'] in R.SEEDS and float(c['pre'].abs().min()) >= R.BLOCK_MARGIN
    assert torch.equal(c['f32']['y'] > 0, c['ref']['y'] > 0)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    assert tuple(c['ref']['y'].shape) == (B, Cout, Ho, Wo) and tuple(c['ref']['dw'].shape) == (Cout, Cin, k, k)
    for key in ('y', 'dx', 'dw', 'dgamma', 'dbeta'):
        b, e32 = R.bound(c['f32'][key], c['ref'][key])
        if float(c['ref'][key].abs().max()) > 1e-9:
            assert 0 < b < 1e-3 * float(c['ref'][key].abs().max()), (key, b)
    if Cout // G * Ho * Wo == 1:
        assert all(float(c['ref'][key].abs().max()) < 1e-10 for key in ('dr', 'dx', 'dw', 'dgamma'))      # 0 to float64 rounding in autograd


def test_the_cases_cover_the_kernel_paths():
    cases = R.BLOCK_CASES.values()
    assert {(k, s) for *_, k, s, _ in cases} == {(3, 1), (3, 2), (1, 1)}
    assert {(ci, co) for _, ci, co, *_ in cases} >= {(32, 32), (32, 64), (64, 32), (96, 32)}
    assert {c[0] for c in cases} == {1, 2, 3}
    runs = lambda c: c[0] * ((c[3] - 1) // c[6] + 1) * (((c[4] - 1) // c[6] + 1 + 63) // 64)              # noqa: E731
    assert min(runs(c) for c in cases) == 1 and any(((c[4] - 1) // c[6] + 1) % 64 == 1 for c in cases) and any(c[4] == 64 and c[6] == 1 for c in cases)
    assert any(co // g == 1 for _, _, co, *_, g in cases) and any(g == 32 and co == 64 for _, _, co, *_, g in cases)
    wo = lambda c: (c[4] - 1) // c[6] + 1                                                                 # noqa: E731
    assert any(c[6] == 2 and wo(c) > 64 for c in cases), 'no stride-2 case crosses the 64-pixel run seam (wgrad ox0 = 64, dgrad tx = 1)'
    max_splits = int(re.search(r'#define\s+VKN_FPN_WGRAD_MAX_SPLITS\s+(\d+)', open(HEADER).read()).group(1))
    assert any(runs(c) > max_splits for c in cases), 'no case has more runs than VKN_FPN_WGRAD_MAX_SPLITS: every split sums one run'
    assert max(c[3] for c in cases) > 5                                                                   # the dgrad grid's y dimension is H
    assert any(H * W > 2048 for _, _, H, W, _ in R.GN_CASES.values())                                     # two runs of the GroupNorm backward's sums
    assert R.DY_SCALES == (1.0, 2.0 ** -20, 2.0 ** 10)


def test_the_float64_reference_is_the_conv_the_header_states():
    """dw and dx of include/vkn_fpn_train.h, written out as sums, against autograd at stride 2 (odd sizes)"""
    torch.manual_seed(5)
    x, w, dr = torch.randn(1, 2, 5, 7, dtype=torch.float64), torch.randn(3, 2, 3, 3, dtype=torch.float64), torch.randn(1, 3, 3, 4, dtype=torch.float64)
    xx, ww = x.clone().requires_grad_(), w.clone().requires_grad_()
    dx, dw = torch.autograd.grad(F.conv2d(xx, ww, None, 2, 1), (xx, ww), dr)
    mine_w, mine_x = torch.zeros_like(w), torch.zeros_like(x)
    for co in range(3):
        for ci in range(2):
            for ky in range(3):
                for kx in range(3):
                    for y in range(3):
                        for xo in range(4):
                            iy, ix = 2 * y + ky - 1, 2 * xo + kx - 1
                            if 0 <= iy < 5 and 0 <= ix < 7:
                                mine_w[co, ci, ky, kx] += dr[0, co, y, xo] * x[0, ci, iy, ix]
                                mine_x[0, ci, iy, ix] += dr[0, co, y, xo] * w[co, ci, ky, kx]
    assert float((mine_w - dw).abs().max()) < 1e-12 and float((mine_x - dx).abs().max()) < 1e-12


def test_fused_backward_is_an_extra_keyword_with_a_default(vkn):
    cls = vkn.semantic_fpn.SemanticFPNWrapper
    p = inspect.signature(cls.__init__).parameters
    assert list(p)[-1] == 'fused_backward' and p['fused_backward'].default is False
    plain = R.fpn_module(vkn, 1, torch.float32)
    fused = R.fpn_module(vkn, 1, torch.float32, fused_backward=True)
    assert plain.fused_backward is False and fused.fused_backward is True
    assert list(plain.state_dict()) == list(fused.state_dict())                                           # no new key
    xs, _ = R.fpn_inputs(1)
    assert not fused.train_fused_ok(xs)                                                                   # CPU tensors: forward_torch as today
    a, b = fused([x.clone().requires_grad_() for x in xs]), fused.forward_torch(xs)
    assert all(torch.equal(u, v) for u, v in zip(a, b))
    fits = vkn.ops.conv_gn_relu_fits
    assert fits(32, 512, 3, 2, 32) and fits(96, 32, 1, 1, 8) and not fits(48, 32, 3, 1, 8) and not fits(32, 544, 3, 1, 32)
    assert not fits(32, 32, 1, 2, 8) and not fits(32, 32, 5, 1, 8) and not fits(32, 32, 3, 1, 5)
    assert callable(vkn.autograd.ConvGNReLUFn.apply) and all(hasattr(vkn.ops, n) for n in ('gn_relu_apply', 'gn_relu_bwd', 'conv_wgrad', 'conv_dgrad'))


def test_module_case_clears_the_margin_in_every_layer(vkn):
    c = R.fpn_case(vkn)
    assert c['pre_min'] >= R.BLOCK_MARGIN and c['seed'] in R.SEEDS
    assert len(c['ref']) == 2 + 4 + 3 * 9 and set(c['ref']) == set(c['f32'])
    for k in c['ref']:
        assert float(c['ref'][k].abs().max()) > 0 and 0 < R.bound(c['f32'][k], c['ref'][k])[0] < 1e-3 * float(c['ref'][k].abs().max()), k


@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv_cases_have_positive_bounds_and_stay_out_of_the_block_cases(name):
    """the multi-run conv-only cases: Gaussian operands of SEEDS[0], every bound positive and below 1e-3 of its tensor; they are the
    first two shapes of exact_cases.FPN_BWD_PINS and no entry of BLOCK_CASES"""
    import exact_cases as ec
    c = R.conv_case(name)
    shape = R.CONV_CASES[name]
    B, Cin, Cout, H, W, k, s = shape
    assert shape == list(ec.FPN_BWD_PINS)[list(R.CONV_CASES).index(name)] and name not in R.BLOCK_CASES
    assert all(shape != b[:7] for b in R.BLOCK_CASES.values())
    assert c['seed'] == R.SEEDS[0] and tuple(c['ref']['conv_dw'].shape) == (Cout, Cin, k, k) and tuple(c['ref']['conv_dx'].shape) == (B, Cin, H, W)
    for key in ('conv_dw', 'conv_dx'):
        b, e32 = R.bound(c['f32'][key], c['ref'][key])
        assert 0 < b < 1e-3 * float(c['ref'][key].abs().max()), (key, b)
