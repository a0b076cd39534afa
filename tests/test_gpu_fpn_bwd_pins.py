"""GPU: the two MFMA gradients of the FPN block's convolution (csrc/vkn_fpn_bwd.hip: k_conv_wgrad, k_conv_dgrad; include/vkn_fpn_train.h)
where tests/test_gpu_fpn_bwd.py does not reach, and the in-place forms the header promises.

tests/test_gpu_fpn_bwd.py judges each tensor by its maximum on shapes at which every split of the weight gradient owns ONE 64-pixel
run, no stride-2 output row is wider than a run and no image has more than 5 rows.  Here:

1. Bit for bit (`torch.equal` with float64 autograd of F.conv2d), x, w and dr integers in [-3, 3] (exact_cases.FPN_BWD_PINS): splits of
   the weight gradient that sum 3, 4 and 5 runs across rows and frames, full and ragged runs alternating; the stride-2 seam (wgrad
   ox0 = 64, dgrad tx = 1 in both column parities); the 1x1 kernel; the shipped 256 channels; more runs than VKN_FPN_WGRAD_MAX_SPLITS and
   33 image rows.  Any summation order gives these bits, so there is no tolerance at 512 channels either.
2. Low halves, still exact (exact_cases.FPN_BWD_LOW): one operand of 13-bit integers against one in {-1, 0, 1}, either way round, for
   both kernels.  The kernels drop lo * lo, which is zero here; a lost or misplaced low half of either operand fails bit for bit.
3. Float operands at the first two shapes of 1 (fpn_bwd_ref.CONV_CASES): Gaussian x, w, dr, the unchanged rule `bound` (8 x the error of
   torch's fp32 autograd against float64, at least 4 ulps) at the three upstream scales.
4. In place, through raw ctypes out of the sentinel arena: vkn_gn_relu_bwd_f32 with dr == dy and vkn_gn_relu_apply_f32 with y == r give
   the bits of the out-of-place calls (no other test runs either form).
Premises (sum |terms| < 2^24, exact splits, low-half share, the split structure read back from the library) are asserted on the CPU by
tests/test_exact_premise.py and tests/test_fpn_bwd_refs.py.

Measured on an MI355X (profiles/fpn_bwd_margins.json): all of 1, 2 and 4 hold bit for bit.  3: err / bound is 0.033 (dw) and 0.653 (dx) at
the stride-1 shape — the largest ratio of the backward's record, dx of the conv alone at 288 -> 160 channels had 0.43 —, 0.030 and
0.073 at stride 2; the same at the three upstream scales, bit for bit.  The rule carries to 512 channels as it stands.
What these tests see that tests/test_gpu_fpn_bwd.py at its cases before this module does not, tried with one-line breaks of
csrc/vkn_fpn_bwd.hip that change values only (not committed); the old module stayed green under all three:
  * a split that stops after its first run: all five cases of 1 and both shapes of 3 fail, with the 33 x 65 case now in BLOCK_CASES;
  * the wgrad patch column one off where S == 2 and ox0 > 0: the stride-2 case of 1, the `wgrad-dr` and `wgrad-x` variants of 2 (their
    stride-2 shape has Wo = 65), the stride-2 shape of 3 and the 9 x 131 case now in BLOCK_CASES fail;
  * the dgrad halo column one off where S == 2 and tx > 0: the same, with the `dgrad-dr` and `dgrad-w` variants."""
import ctypes

import pytest
import torch

import exact_cases as ec
import fpn_bwd_ref as R
from abi_arena import Arena, frozen
from helpers import record_margins
from test_gpu_exact import _diff, _finish

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PINS = list(ec.FPN_BWD_PINS)


def _cuda(*ts):
    return [t.to(DEV) for t in ts]


def _image_t(vkn, w):
    """the prepared image of the flipped, channel-transposed weight: vkn_conv_dgrad_f32's A operand"""
    return vkn.ops.conv_prepare(w.flip(2, 3).transpose(0, 1).contiguous())


# ------------------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize('i', range(len(PINS)), ids=[ec.fpn_bwd_id(s) for s in PINS])
def test_conv_wgrad_and_dgrad_bit_for_bit(vkn, i):
    shape = PINS[i]
    B, Cin, Cout, H, W, k, s = shape
    d = ec.conv_bwd_case(shape, 3800 + i)                       # (premise, non-vacuity, empty low halves: asserted in there)
    x, w, dr = _cuda(d['x'], d['w'], d['dr'])
    with frozen(x, w, dr):
        dw = vkn.ops.conv_wgrad(dr, x, k, s)
        dx = vkn.ops.conv_dgrad(dr, _image_t(vkn, w), Cin, H, W, k, s)
    name = ec.fpn_bwd_id(shape)
    _finish(vkn, [f for f in (_diff(f'wgrad {name} [co, ci, ky, kx]', dw, d['dw']), _diff(f'dgrad {name} [b, ci, y, x]', dx, d['dx'])) if f])


# ------------------------------------------------------------------------------------------------------------ 2. low halves
@pytest.mark.parametrize('variant', ec.FPN_BWD_LOW_VARIANTS)
def test_conv_gradients_keep_the_low_halves_bit_for_bit(vkn, variant):
    kernel, which = variant.split('-')
    fails = []
    for j, shape in enumerate(ec.FPN_BWD_LOW):
        B, Cin, Cout, H, W, k, s = shape
        d = ec.conv_bwd_low_case(shape, variant, 3900 + 4 * j + ec.FPN_BWD_LOW_VARIANTS.index(variant))
        x, w, dr = _cuda(d['x'], d['w'], d['dr'])
        if kernel == 'wgrad':
            got = vkn.ops.conv_wgrad(dr, x, k, s)
        else:
            got = vkn.ops.conv_dgrad(dr, _image_t(vkn, w), Cin, H, W, k, s)
        fails.append(_diff(f'{ec.fpn_bwd_id(shape, variant)} (low share {d["low_share"]:.2f})', got, d['out']))
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------ 3. float operands
@pytest.mark.parametrize('scale', R.DY_SCALES)
@pytest.mark.parametrize('name', list(R.CONV_CASES))
def test_conv_gradients_where_a_split_sums_many_runs(vkn, name, scale):
    """the rule of tests/test_gpu_fpn_bwd.py, unchanged: per tensor, max-abs error of gradient / scale <= max(8 x the error of torch's
    fp32 autograd, 4 ulps)"""
    c = R.conv_case(name)
    B, Cin, Cout, H, W, k, s = R.CONV_CASES[name]
    x, w, dr = _cuda(c['x'], c['w'], c['dy'] * scale)
    with frozen(x, w, dr):
        got = dict(conv_dw=vkn.ops.conv_wgrad(dr, x, k, s), conv_dx=vkn.ops.conv_dgrad(dr, _image_t(vkn, w), Cin, H, W, k, s))
    vkn.ops.workspace_status(DEV)
    ratios, fails = {}, []
    for key in ('conv_dw', 'conv_dx'):
        b, e32 = R.bound(c['f32'][key], c['ref'][key])
        e = R.err(got[key] / scale, c['ref'][key])
        ratios[key] = e / b
        print(f'FPNBWD conv[{name}-{scale:g}] {key}: kernel {e:.3e} fp32 autograd {e32:.3e} bound {b:.3e} ratio {e / b:.3f}')
        if not e <= b:
            fails.append((key, e, b))
    record_margins(f'test_gpu_fpn_bwd_pins::conv[{name}-{scale:g}]', ratios)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------------------ 4. in place
def _bits(t):
    return t.detach().contiguous().reshape(-1).view(torch.int32).cpu()


def test_gn_relu_bwd_and_apply_in_place(vkn):
    """include/vkn_fpn_train.h: dr "may be dy", y "may be r".  Two runs of VKN_FPN_BWD_RUN_PX pixels per (frame, channel), the second
    ragged: the first launch's sums read all of dy before the elementwise pass overwrites it."""
    name = '2x32x33x63-g8'
    c = R.gn_case(name)
    B, C, H, W, G = R.GN_CASES[name]
    assert H * W > vkn._lib.FPN_TRAIN['VKN_FPN_BWD_RUN_PX']
    L = vkn._lib.lib()
    r, stats, gamma, beta, dy = _cuda(c['r'], c['stats'], c['gamma'], c['beta'], c['dy'])
    nb = L.vkn_gn_relu_bwd_workspace_bytes(B, C, H, W, G)
    assert nb
    A = Arena(DEV)
    y, dr, dgamma, dbeta = A.out((B, C, H, W), name='y'), A.out((B, C, H, W), name='dr'), A.out((C,), name='dgamma'), A.out((C,), name='dbeta')
    y_io, dr_io = A.out((B, C, H, W), name='y == r'), A.out((B, C, H, W), name='dr == dy')
    dgamma2, dbeta2 = A.out((C,), name='dgamma in place'), A.out((C,), name='dbeta in place')
    ws = [A.ws(nb, name=f'ws{i}') for i in range(2)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731
    for wsr in ws:
        wsr.bytes[:256].zero_()                                                # the caller's part: a clear status header
    y_io.t.copy_(r)
    dr_io.t.copy_(dy)
    torch.cuda.synchronize()
    with torch.cuda.device(DEV), frozen(r, stats, gamma, beta, dy):
        assert L.vkn_gn_relu_apply_f32(p(r), p(stats), p(gamma), p(beta), G, y.ptr, B, C, H, W, None) == 0
        assert L.vkn_gn_relu_apply_f32(y_io.ptr, p(stats), p(gamma), p(beta), G, y_io.ptr, B, C, H, W, None) == 0
        assert L.vkn_gn_relu_bwd_f32(p(dy), p(r), p(stats), p(gamma), p(beta), G, dr.ptr, dgamma.ptr, dbeta.ptr, B, C, H, W, ws[0].ptr, nb, None) == 0
        assert L.vkn_gn_relu_bwd_f32(dr_io.ptr, p(r), p(stats), p(gamma), p(beta), G, dr_io.ptr, dgamma2.ptr, dbeta2.ptr, B, C, H, W, ws[1].ptr, nb, None) == 0
    A.check(name)
    assert all(int(wsr.bytes[:4].view(torch.int32)) == 0 for wsr in ws)        # no range bit
    assert torch.equal(_bits(y_io.t), _bits(y.t)) and torch.equal(y.t.cpu() > 0, c['pre'] > 0)
    assert torch.equal(_bits(dr_io.t), _bits(dr.t)) and torch.equal(_bits(dgamma2.t), _bits(dgamma.t)) and torch.equal(_bits(dbeta2.t), _bits(dbeta.t))
    assert not torch.equal(_bits(dr.t), _bits(dy)) and bool((y.t != r).any())  # (the calls did something)
    for key, got in (('y', y.t), ('dr', dr.t), ('dgamma', dgamma.t), ('dbeta', dbeta.t)):  # ... and it is the block's backward
        assert R.err(got, c['ref'][key]) <= R.bound(c['f32'][key], c['ref'][key])[0], key
