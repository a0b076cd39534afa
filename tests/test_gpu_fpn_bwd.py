"""GPU: the backward of one conv + GroupNorm + ReLU block (include/vkn_fpn_train.h, csrc/vkn_fpn_bwd.hip), `autograd.ConvGNReLUFn`
and `SemanticFPNWrapper(fused_backward=True)`.

Reference, bound and inputs are those of tests/fpn_bwd_ref.py (tests/test_fpn_bwd_refs.py asserts their premises on the CPU): float64
autograd of the torch composition; per tensor, max-abs error <= max(8 x the error of torch's fp32 composition against that float64,
4 fp32 ulps of the tensor's largest magnitude); every pre-activation clear of the ReLU edge.  Every gradient test runs at upstream
scales 1, 2^-20 and 2^10 and judges gradient / scale by the bound of scale 1: an operand staged without its power of two has no bits
left at 2^-20.  The ratios err / bound go to the margins record (profiles/fpn_bwd_margins.json holds a run's).

Measured on an MI355X (that file): the largest ratio err / bound is 0.43 (dx of the convolution alone at 288 -> 160 channels), 0.30 for dr
of the GroupNorm backward, 0.26 for the block's y; every ratio is the same at the three upstream scales, bit for bit — the power of two
per tensor is exact.  The wrapper's 33 tensors lie within 0.2 of their bounds.  The two cases added with
tests/test_gpu_fpn_bwd_pins.py — 33 rows of 65 pixels (66 runs in 64 splits) and 5 x 66 outputs at stride 2 — stay below 0.15: conv alone
dw 0.028 / 0.036, dx 0.142 / 0.083; block y 0.114 / 0.144, dx 0.143 / 0.098, dw 0.034 / 0.046.  The 112 records of the cases before them
came out bit for bit as recorded."""
import ctypes

import pytest
import torch

import fpn_bwd_ref as R
from abi_arena import Arena, frozen
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_WORKSPACE, E_ALIGN, E_RANGE = -3, -5, -6


def _cuda(*ts):
    return [t.to(DEV) for t in ts]


def _judge(test_id, got, case, keys, scale=1.0):
    """every tensor of `got` (divided by the upstream scale) inside its bound; records err / bound"""
    ratios, fails = {}, []
    for k in keys:
        b, e32 = R.bound(case['f32'][k], case['ref'][k])
        e = R.err(got[k] / scale if scale != 1.0 and k != 'y' else got[k], case['ref'][k])
        ratios[k] = e / b
        print(f'FPNBWD {test_id} {k}: kernel {e:.3e} fp32 composition {e32:.3e} bound {b:.3e} ratio {e / b:.3f}')
        if not e <= b:
            fails.append((k, e, b))
    record_margins(f'test_gpu_fpn_bwd::{test_id}', ratios)
    assert not fails, fails


# ------------------------------------------------------------------------------------------------ GroupNorm + ReLU, forward and backward
@pytest.mark.parametrize('scale', R.DY_SCALES)
@pytest.mark.parametrize('name', list(R.GN_CASES))
def test_gn_relu_apply_and_bwd(vkn, name, scale):
    c = R.gn_case(name)
    r, stats, gamma, beta, dy = _cuda(c['r'], c['stats'], c['gamma'], c['beta'], c['dy'] * scale)
    with frozen(r, stats, gamma, beta, dy):
        y = vkn.ops.gn_relu_apply(r, stats, gamma, beta)
        dr, dgamma, dbeta = vkn.ops.gn_relu_bwd(dy, r, stats, gamma, beta)
    vkn.ops.workspace_status(DEV)
    assert torch.equal(y.cpu() > 0, c['pre'] > 0)
    B, C, H, W, G = R.GN_CASES[name]
    if C // G * H * W == 1:
        assert not dr.any() and not dgamma.any()                              # a group of one element: exactly 0
    _judge(f'gn[{name}-{scale:g}]', dict(y=y, dr=dr, dgamma=dgamma, dbeta=dbeta), c, ('y', 'dr', 'dgamma', 'dbeta'), scale)


# ------------------------------------------------------------------------------------------------ the two convolution gradients alone
@pytest.mark.parametrize('scale', R.DY_SCALES)
@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_conv_wgrad_and_dgrad(vkn, name, scale):
    """dw and dx of the convolution alone, the case's upstream gradient taken as the gradient of the RAW conv output: the MFMA kernels
    without the GroupNorm backward before them (reference: float64 autograd of F.conv2d, keys `conv_dw`, `conv_dx`)"""
    c = R.block_case(name)
    B, Cin, Cout, H, W, k, s, G = R.BLOCK_CASES[name]
    x, w, dr = _cuda(c['x'], c['w'], c['dy'] * scale)
    with frozen(x, w, dr):
        dw = vkn.ops.conv_wgrad(dr, x, k, s)
        dx = vkn.ops.conv_dgrad(dr, vkn.ops.conv_prepare(w.flip(2, 3).transpose(0, 1).contiguous()), Cin, H, W, k, s)
    vkn.ops.workspace_status(DEV)
    assert tuple(dw.shape) == (Cout, Cin, k, k) and tuple(dx.shape) == (B, Cin, H, W)
    _judge(f'conv[{name}-{scale:g}]', dict(conv_dw=dw, conv_dx=dx), c, ('conv_dw', 'conv_dx'), scale)


# ------------------------------------------------------------------------------------------------ the block as an autograd function
def _block(vkn, c, scale, need_dx=True):
    x, w, gamma, beta, dy = _cuda(c['x'], c['w'], c['gamma'], c['beta'], c['dy'] * scale)
    leaves = [t.requires_grad_() for t in (x, w, gamma, beta)]
    if not need_dx:
        x.requires_grad_(False)
    y = vkn.autograd.ConvGNReLUFn.apply(x, w, gamma, beta, c['G'], c['stride'])
    grads = torch.autograd.grad(y, leaves if need_dx else leaves[1:], dy)
    return y.detach(), grads


@pytest.mark.parametrize('scale', R.DY_SCALES)
@pytest.mark.parametrize('name', list(R.BLOCK_CASES))
def test_block_forward_and_backward(vkn, name, scale):
    c = R.block_case(name)
    y, (dx, dw, dgamma, dbeta) = _block(vkn, c, scale)
    vkn.ops.workspace_status(DEV)
    B, Cin, Cout, H, W, k, s, G = R.BLOCK_CASES[name]
    if Cout // G * y.shape[2] * y.shape[3] == 1:
        assert not dx.any() and not dw.any() and not dgamma.any()             # groups of one element: dr is exactly 0, and so is what follows
    _judge(f'block[{name}-{scale:g}]', dict(y=y, dx=dx, dw=dw, dgamma=dgamma, dbeta=dbeta), c, ('y', 'dx', 'dw', 'dgamma', 'dbeta'), scale)


def test_block_is_deterministic_and_skips_dx(vkn):
    """two backward calls on the same inputs are bitwise equal; without a gradient for x the function returns none and the others
    are the same bits"""
    c = R.block_case('k3s1-32to32-3x65-g8-B3')
    y1, g1 = _block(vkn, c, 1.0)
    y2, g2 = _block(vkn, c, 1.0)
    assert torch.equal(y1, y2) and all(torch.equal(a, b) for a, b in zip(g1, g2))
    y3, g3 = _block(vkn, c, 1.0, need_dx=False)
    assert torch.equal(y1, y3) and len(g3) == 3 and all(torch.equal(a, b) for a, b in zip(g1[1:], g3))
    calls = []
    orig = vkn.ops.conv_dgrad
    vkn.ops.conv_dgrad = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        _block(vkn, c, 1.0, need_dx=False)
        assert not calls
        _block(vkn, c, 1.0)
        assert calls == [1]
    finally:
        vkn.ops.conv_dgrad = orig


def test_non_finite_gradient_sets_the_range_bit(vkn):
    """an inf in dy: VKN_STATUS_RANGE, `ops.workspace_status` raises once and is clear afterwards"""
    c = R.block_case('k3s1-32to32-3x7-g8')
    vkn.ops.workspace_status(DEV)
    x, w, gamma, beta, dy = _cuda(c['x'], c['w'], c['gamma'], c['beta'], c['dy'].clone())
    mask = (c['ref']['y'] > 0).to(DEV)
    b0, c0, h0, w0 = mask.nonzero()[0].tolist()
    dy[b0, c0, h0, w0] = float('inf')                                          # where the ReLU passes it on
    y = vkn.autograd.ConvGNReLUFn.apply(x.requires_grad_(), w.requires_grad_(), gamma.requires_grad_(), beta.requires_grad_(), c['G'], c['stride'])
    vkn.ops.workspace_status(DEV)                                              # the forward is clean
    torch.autograd.grad(y, (x, w, gamma, beta), dy)
    with pytest.raises(vkn.VknError) as e:
        vkn.ops.workspace_status(DEV)
    assert e.value.code == E_RANGE
    vkn.ops.workspace_status(DEV)
    # each entry on its own
    r, stats = vkn.ops.conv_gn(x.detach(), vkn.ops.conv_prepare(w.detach()), w.shape[0], 3, 1, c['G'])
    bad = torch.full_like(r, float('nan'))
    for call in (lambda: vkn.ops.gn_relu_bwd(dy, r, stats, gamma.detach(), beta.detach()), lambda: vkn.ops.conv_wgrad(bad, x.detach(), 3, 1),
                 lambda: vkn.ops.conv_wgrad(r, torch.full_like(x, float('inf')).detach(), 3, 1),
                 lambda: vkn.ops.conv_dgrad(bad, vkn.ops.conv_prepare(w.detach().flip(2, 3).transpose(0, 1).contiguous()), 32, 3, 7, 3, 1)):
        call()
        with pytest.raises(vkn.VknError):
            vkn.ops.workspace_status(DEV)
    vkn.ops.workspace_status(DEV)


# ------------------------------------------------------------------------------------------------ the wrapper
def _module_run(mod, xs, gs):
    ins = [x.to(DEV).requires_grad_() for x in xs]
    outs = mod(ins)
    params = [p for _, p in sorted(mod.named_parameters())]
    grads = torch.autograd.grad(outs, ins + params, [g.to(DEV) for g in gs])
    res = {f'out{i}': o.detach() for i, o in enumerate(outs)}
    res.update({f'd_p{i + 2}': g for i, g in enumerate(grads[:4])})
    res.update({'d_' + n: g for (n, _), g in zip(sorted(mod.named_parameters()), grads[4:])})
    return res


def _gpu_module(vkn, seed, **kw):
    mod = R.fpn_module(vkn, seed, torch.float32, **kw).to(DEV)
    h, w = R.FPN_CFG['sizes'][3]
    cpu_pos = R.fpn_module(vkn, seed, torch.float32).positional_map(1, h, w, torch.device('cpu'))
    mod._pos_cache[(h, w, str(torch.device(DEV)))] = cpu_pos.contiguous().to(DEV)      # the reference's own fp32 sines, not the device's
    return mod


def test_wrapper_end_to_end(vkn):
    """[out, aux], the four input gradients and all 27 parameter gradients of `fused_backward=True` against the float64 composition"""
    c = R.fpn_case(vkn)
    mod = _gpu_module(vkn, c['seed'], fused_backward=True)
    calls = []
    orig = vkn.autograd.conv_gn_relu
    vkn.autograd.conv_gn_relu = lambda *a, **k: calls.append(1) or orig(*a, **k)
    try:
        got = _module_run(mod, c['xs'], c['gs'])
    finally:
        vkn.autograd.conv_gn_relu = orig
    vkn.ops.workspace_status(DEV)
    assert len(calls) == 9 and set(got) == set(c['ref'])
    _judge('wrapper', got, c, sorted(c['ref']))


def test_wrapper_outside_the_envelope_takes_forward_torch(vkn):
    """Cin = 48 is outside the envelope: under the flag the module runs `forward_torch` and the fused op is never called"""
    C = 48
    mod = vkn.semantic_fpn.SemanticFPNWrapper(C, C, C, 0, 3, cat_coors_level=3, upsample_times=2, num_aux_convs=1,
                                              norm_cfg=dict(type='GN', num_groups=8), fused_backward=True).to(DEV)
    gen = torch.Generator().manual_seed(3)
    xs = [torch.randn((1, C, h, w), generator=gen).to(DEV).requires_grad_() for h, w in R.FPN_CFG['sizes']]
    assert not mod.train_fused_ok(xs)

    def boom(*a, **k):
        raise AssertionError('the fused block was called outside its envelope')
    orig = vkn.autograd.conv_gn_relu
    vkn.autograd.conv_gn_relu = boom
    try:
        torch.manual_seed(0)
        a = mod(xs)
        b = mod.forward_torch(xs)
    finally:
        vkn.autograd.conv_gn_relu = orig
    assert all(u.requires_grad and torch.equal(u, v) for u, v in zip(a, b))


def test_wrapper_default_is_unchanged(vkn):
    """`fused_backward=False`: outputs and gradients are `forward_torch`'s, bit for bit, on the same device"""
    c = R.fpn_case(vkn)
    mod = _gpu_module(vkn, c['seed'])
    assert mod.fused_backward is False
    det = torch.backends.cudnn.deterministic
    torch.backends.cudnn.deterministic = True
    try:
        got = _module_run(mod, c['xs'], c['gs'])
        fwd, mod.forward = mod.forward, mod.forward_torch
        want = _module_run(mod, c['xs'], c['gs'])
        mod.forward = fwd
    finally:
        torch.backends.cudnn.deterministic = det
    assert all(torch.equal(got[k], want[k]) for k in want)


# ------------------------------------------------------------------------------------------------ buffer contract
@pytest.mark.parametrize('name', ['k3s1-64to32-3x65-g8', 'k3s2-32to32-5x67-g8', 'k1s1-32to64-3x65-g32'])
def test_buffer_contract(vkn, name):
    """every writing entry through raw ctypes: outputs and workspaces of exactly the stated sizes out of the sentinel arena, inputs
    frozen; then the VKN_E_WORKSPACE (one byte short) and VKN_E_ALIGN gates, which write nothing"""
    c = R.block_case(name)
    B, Cin, Cout, H, W, k, s, G = R.BLOCK_CASES[name]
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    L = vkn._lib.lib()
    x, w, gamma, beta, dy = _cuda(c['x'], c['w'], c['gamma'], c['beta'], c['dy'])
    r, stats = vkn.ops.conv_gn(x, vkn.ops.conv_prepare(w), Cout, k, s, G)
    img_t = vkn.ops.conv_prepare(w.flip(2, 3).transpose(0, 1).contiguous())
    torch.cuda.synchronize()
    nb = (L.vkn_gn_relu_bwd_workspace_bytes(B, Cout, Ho, Wo, G), L.vkn_conv_wgrad_workspace_bytes(B, Cin, H, W, Cout, k, s),
          L.vkn_conv_dgrad_workspace_bytes(B, Cout, H, W, s))
    assert all(nb)
    A = Arena(DEV)
    y, dr = A.out((B, Cout, Ho, Wo), name='y'), A.out((B, Cout, Ho, Wo), name='dr')
    dgamma, dbeta = A.out((Cout,), name='dgamma'), A.out((Cout,), name='dbeta')
    dw, dx = A.out((Cout, Cin, k, k), name='dw'), A.out((B, Cin, H, W), name='dx')
    ws = [A.ws(n, name=f'ws{i}') for i, n in enumerate(nb)]
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731
    for wsr in ws:
        wsr.bytes[:256].zero_()                                                # the caller's part: a clear status header
    with torch.cuda.device(DEV), frozen(x, w, gamma, beta, dy, r, stats, img_t):
        assert L.vkn_gn_relu_apply_f32(p(r), p(stats), p(gamma), p(beta), G, y.ptr, B, Cout, Ho, Wo, None) == 0
        assert L.vkn_gn_relu_bwd_f32(p(dy), p(r), p(stats), p(gamma), p(beta), G, dr.ptr, dgamma.ptr, dbeta.ptr, B, Cout, Ho, Wo, ws[0].ptr, nb[0], None) == 0
        torch.cuda.synchronize()
        drt = dr.t.clone()
        assert L.vkn_conv_wgrad_f32(p(drt), p(x), dw.ptr, B, Cin, H, W, Cout, k, s, ws[1].ptr, nb[1], None) == 0
        assert L.vkn_conv_dgrad_f32(p(drt), p(img_t), dx.ptr, B, Cin, H, W, Cout, k, s, ws[2].ptr, nb[2], None) == 0
    A.check(name)
    assert all(int(wsr.bytes[:4].view(torch.int32)) == 0 for wsr in ws)        # no range bit
    _judge(f'contract[{name}]', dict(y=y.t, dr=dr.t, dgamma=dgamma.t, dbeta=dbeta.t, dw=dw.t, dx=dx.t), c, ('y', 'dr', 'dgamma', 'dbeta', 'dw', 'dx'))
    # the gates: nothing is written
    B2 = Arena(DEV)
    o = [B2.out(t.shape, name=f'o{i}', full=False) for i, t in enumerate((dr.t, dgamma.t, dbeta.t, dw.t, dx.t))]
    w2 = [B2.ws(n, name=f'ws{i}') for i, n in enumerate(nb)]
    with torch.cuda.device(DEV):
        for short, skew, want in ((1, 0, E_WORKSPACE), (0, 8, E_ALIGN)):
            q = lambda rng: ctypes.c_void_p(rng.addr + skew)                   # noqa: E731
            assert L.vkn_gn_relu_bwd_f32(p(dy), p(r), p(stats), p(gamma), p(beta), G, o[0].ptr, o[1].ptr, o[2].ptr, B, Cout, Ho, Wo, q(w2[0]), nb[0] - short, None) == want
            assert L.vkn_conv_wgrad_f32(p(drt), p(x), o[3].ptr, B, Cin, H, W, Cout, k, s, q(w2[1]), nb[1] - short, None) == want
            assert L.vkn_conv_dgrad_f32(p(drt), p(img_t), o[4].ptr, B, Cin, H, W, Cout, k, s, q(w2[2]), nb[2] - short, None) == want
        assert L.vkn_gn_relu_apply_f32(p(r), p(stats), p(gamma), p(beta), G, ctypes.c_void_p(o[0].addr + 8), B, Cout, Ho, Wo, None) == E_ALIGN
    torch.cuda.synchronize()
    assert not any('stray' in m for m in B2.problems()) and all(bool((rng.bytes.view(torch.int32) == 0x7FC0BEEF).all()) for rng in o)
