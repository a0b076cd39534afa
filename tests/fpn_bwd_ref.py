"""CPU side of tests/test_gpu_fpn_bwd.py: the cases, their operands, the float64 references and the bounds of the backward of one
conv + GroupNorm + ReLU block (include/vkn_fpn_train.h).  Plain module; tests/test_fpn_bwd_refs.py asserts its premises without a GPU.

Reference: float64 autograd of the torch composition F.conv2d -> F.group_norm -> relu on the CPU.
Bound (the rule of tests/test_gpu_track_loss.py), per tensor, max-abs: 8 x the error of torch's own fp32 composition against the same
float64 on the same inputs, at least 4 fp32 ulps of the tensor's largest magnitude.  The 8 covers another summation order over up to
B Ho Wo terms and the 2^-22 operand resolution of the f16 split.  It is computed here, from the reference arithmetic alone.

ReLU edge: a pre-activation within rounding of zero flips the mask and moves the gradients by whole terms.  The GroupNorm unit cases
build r so that every float64 pre-activation gamma xhat + beta has magnitude >= 0.05 with |gamma| >= 0.5 (`bounded_r`); the block and
module cases take the first seed of `SEEDS` whose float64 pre-activations all have magnitude >= 1e-5 (fp32 rounding of a
pre-activation of unit scale is below 1e-6).  A condition on the inputs, not a tolerance."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

EPS = 1e-5
SEEDS = tuple(range(7100, 7116))
UNIT_MARGIN, BLOCK_MARGIN = 0.05, 1e-5
DY_SCALES = (1.0, 2.0 ** -20, 2.0 ** 10)

# name: (B, Cin, Cout, H, W, k, stride, groups)
BLOCK_CASES = {
    'k3s1-32to32-3x7-g8': (2, 32, 32, 3, 7, 3, 1, 8),             # under one 64-pixel run
    'k3s1-32to64-2x64-g32': (2, 32, 64, 2, 64, 3, 1, 32),         # exactly one run per row; Cin < Cout; 32 groups of 2
    'k3s1-64to32-3x65-g8': (2, 64, 32, 3, 65, 3, 1, 8),           # one run + 1; Cin > Cout, two chunks
    'k3s1-96to32-2x64-g8': (2, 96, 32, 2, 64, 3, 1, 8),           # three chunks
    'k3s1-32to32-1x1-g32': (2, 32, 32, 1, 1, 3, 1, 32),           # groups of ONE element: dr, dx, dw exactly 0
    'k3s2-32to32-5x67-g8': (2, 32, 32, 5, 67, 3, 2, 8),           # -> 3 x 34, odd sizes
    'k3s2-64to32-4x64-g8': (2, 64, 32, 4, 64, 3, 2, 8),           # -> 2 x 32
    'k3s2-32to32-1x1-g8': (2, 32, 32, 1, 1, 3, 2, 8),             # -> 1 x 1
    'k1s1-32to64-3x65-g32': (2, 32, 64, 3, 65, 1, 1, 32),
    'k1s1-32to32-3x7-g32': (2, 32, 32, 3, 7, 1, 1, 32),           # groups of one channel
    'k3s1-32to32-1x64-g8-B1': (1, 32, 32, 1, 64, 3, 1, 8),        # ONE pixel run in all: one split of the weight gradient
    'k3s1-32to32-3x65-g8-B3': (3, 32, 32, 3, 65, 3, 1, 8),        # 18 runs, every second one ragged
    'k3s1-288to160-3x7-g32': (2, 288, 160, 3, 7, 3, 1, 32),       # past 256 input and 128 output channels: a second workgroup column in both gradients
    'k3s2-160to288-5x9-g32': (2, 160, 288, 5, 9, 3, 2, 32),       # ... the other way round, at stride 2; all four waves of the input gradient
    'k1s1-256to256-2x3-g32': (1, 256, 256, 2, 3, 1, 1, 32),       # the shipped channel count
    'k3s1-32to32-33x65-g8-B1': (1, 32, 32, 33, 65, 3, 1, 8),      # 66 runs: more than VKN_FPN_WGRAD_MAX_SPLITS, two splits sum two runs; 33 rows
    'k3s2-32to32-9x131-g8': (2, 32, 32, 9, 131, 3, 2, 8),         # -> 5 x 66: the 64-pixel seam at stride 2 through GroupNorm, wgrad and dgrad
}
# name: (B, Cin, Cout, H, W, k, stride): the convolution's two gradients alone where a split of the weight gradient sums 4 or 5 runs
# (tests/exact_cases.py: FPN_BWD_PINS pins the same shapes bit for bit on integers).  No GroupNorm, no ReLU edge: no seed search.  Kept
# out of BLOCK_CASES: 512 -> 512 channels have no seed clear of the ReLU edge, and tools/convtile_ab.py hashes BLOCK_CASES only.
CONV_CASES = {
    'k3s1-512to512-3x65-B3': (3, 512, 512, 3, 65, 3, 1),          # 18 runs in 4 splits of 4, 5, 4, 5; full and one-pixel runs alternate
    'k3s2-512to512-5x131-B3': (3, 512, 512, 5, 131, 3, 2),        # -> 3 x 66: every second run is the 2-pixel run behind the seam
}
# name: (B, C, H, W, groups)
GN_CASES = {
    '2x32x3x7-g8': (2, 32, 3, 7, 8),
    '2x32x1x1-g32': (2, 32, 1, 1, 32),                            # groups of one element: dr exactly 0
    '2x64x3x65-g32': (2, 64, 3, 65, 32),
    '2x32x33x63-g8': (2, 32, 33, 63, 8),                          # 2079 pixels: two runs of VKN_FPN_BWD_RUN_PX, the second ragged
    '1x32x2x64-g8': (1, 32, 2, 64, 8),
    '3x32x3x7-g32': (3, 32, 3, 7, 32),
}
FPN_CFG = dict(C=32, groups=8, B=2, sizes=((16, 24), (8, 12), (4, 6), (2, 3)))


def _signed(gen, shape, lo, hi):
    mag = lo + (hi - lo) * torch.rand(shape, generator=gen, dtype=torch.float64)
    return mag * (torch.randint(0, 2, shape, generator=gen).to(torch.float64) * 2 - 1)


def ulp_floor(t64, ulps=4):
    return ulps * float(np.spacing(np.float32(t64.abs().max().item())))


def bound(t32, t64):
    """(bound, error of the fp32 composition) of one tensor"""
    e32 = float((t32.double() - t64).abs().max()) if t64.numel() else 0.0
    return max(8 * e32, ulp_floor(t64)), e32


def err(got, t64):
    return float((got.detach().double().cpu() - t64).abs().max()) if t64.numel() else 0.0


def group_stats(r64, G):
    """(mean, var) per (frame, group) in float64, biased variance as nn.GroupNorm"""
    B = r64.shape[0]
    v = r64.reshape(B, G, -1)
    return v.mean(2), v.var(2, unbiased=False)


def preact(r64, gamma64, beta64, G):
    m, v = group_stats(r64, G)
    B, C = r64.shape[:2]
    xh = ((r64.reshape(B, G, -1) - m[..., None]) / torch.sqrt(v[..., None] + EPS)).reshape(r64.shape)
    return gamma64.view(1, C, 1, 1) * xh + beta64.view(1, C, 1, 1)


# ---------------------------------------------------------------------------------------------- GroupNorm + ReLU unit cases
def bounded_r(y_target, gamma, beta, G, margin=UNIT_MARGIN):
    """fp32 r whose float64 pre-activations gamma xhat(r) + beta all have magnitude >= margin.  Starts from z = (y_target - beta) / gamma
    (shifted and scaled: xhat does not see it) and moves the few elements that the group's own standardisation brought under the
    margin back out, until none is left."""
    B, C = y_target.shape[:2]
    ga, be = gamma.view(1, C, 1, 1), beta.view(1, C, 1, 1)
    r = (1.3 * (y_target - be) / ga + 0.7).float().double()
    for _ in range(200):
        y = preact(r, gamma, beta, G)
        bad = y.abs() < margin * 1.02
        if not bad.any():
            return r.float()
        m, v = group_stats(r, G)
        shape = (B, G) + (1,) * 3
        cpg = C // G
        mm = m.view(shape).expand(B, G, cpg, *r.shape[2:]).reshape(r.shape)
        sd = torch.sqrt(v + EPS).view(shape).expand(B, G, cpg, *r.shape[2:]).reshape(r.shape)
        want = torch.where(y >= 0, torch.full_like(y, 2 * margin), torch.full_like(y, -2 * margin))
        r = torch.where(bad, ((want - be) / ga) * sd + mm, r).float().double()
    raise AssertionError('bounded_r did not settle')


@functools.lru_cache(maxsize=None)
def gn_case(name):
    """operands (fp32) + float64 reference + fp32 composition of one GroupNorm + ReLU case, upstream gradient at scale 1"""
    B, C, H, W, G = GN_CASES[name]
    gen = torch.Generator().manual_seed(4200 + sorted(GN_CASES).index(name))
    gamma, beta = _signed(gen, (C,), 0.5, 1.5), _signed(gen, (C,), UNIT_MARGIN, 0.5)
    r = bounded_r(_signed(gen, (B, C, H, W), UNIT_MARGIN, 1.5), gamma, beta, G)
    gamma, beta = gamma.float(), beta.float()
    dy = torch.randn((B, C, H, W), generator=gen, dtype=torch.float64).float()
    m, v = group_stats(r.double(), G)
    stats = torch.stack([m, 1.0 / torch.sqrt(v + EPS)], 2).float()            # what vkn_conv_gn_f32 hands over: (mean, rstd) in fp32
    out = dict(r=r, gamma=gamma, beta=beta, dy=dy, stats=stats, G=G)
    for key, dt in (('ref', torch.float64), ('f32', torch.float32)):
        rr, gg, bb = (t.detach().to(dt).clone().requires_grad_() for t in (r, gamma, beta))
        y = F.group_norm(rr, G, gg, bb, EPS).relu()
        dr, dg, db = torch.autograd.grad(y, (rr, gg, bb), dy.to(dt))
        out[key] = dict(y=y.detach(), dr=dr, dgamma=dg, dbeta=db)
    out['pre'] = preact(r.double(), gamma.double(), beta.double(), G)
    return out


# ---------------------------------------------------------------------------------------------- block cases
def _block_operands(shape, seed):
    B, Cin, Cout, H, W, k, s, G = shape
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn((B, Cin, H, W), generator=gen, dtype=torch.float64).float()
    w = (0.05 * torch.randn((Cout, Cin, k, k), generator=gen, dtype=torch.float64)).float()
    gamma, beta = _signed(gen, (Cout,), 0.5, 1.5).float(), (0.3 * torch.randn((Cout,), generator=gen, dtype=torch.float64)).float()
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    dy = torch.randn((B, Cout, Ho, Wo), generator=gen, dtype=torch.float64).float()
    return x, w, gamma, beta, dy


def _compose(x, w, gamma, beta, G, s, dt):
    xx, ww, gg, bb = (t.detach().to(dt).clone().requires_grad_() for t in (x, w, gamma, beta))
    r = F.conv2d(xx, ww, None, s, w.shape[-1] // 2)
    return (xx, ww, gg, bb), r, F.group_norm(r, G, gg, bb, EPS).relu()


@functools.lru_cache(maxsize=None)
def block_case(name):
    """operands of the first seed of SEEDS whose float64 pre-activations all clear BLOCK_MARGIN (a group of ONE element has
    pre-activation beta: the same condition), the float64 reference and the fp32 composition, upstream gradient at scale 1"""
    shape = BLOCK_CASES[name]
    G, s = shape[7], shape[6]
    for seed in SEEDS:
        x, w, gamma, beta, dy = _block_operands(shape, seed)
        leaves, r, y = _compose(x, w, gamma, beta, G, s, torch.float64)
        pre = preact(r.detach(), gamma.double(), beta.double(), G)
        if float(pre.abs().min()) >= BLOCK_MARGIN:
            break
    else:
        raise AssertionError(f'{name}: no seed of {SEEDS} clears the ReLU margin')
    out = dict(x=x, w=w, gamma=gamma, beta=beta, dy=dy, G=G, stride=s, k=shape[5], seed=seed, pre=pre)
    for key, dt in (('ref', torch.float64), ('f32', torch.float32)):
        leaves, r, y = _compose(x, w, gamma, beta, G, s, dt)
        dr, = torch.autograd.grad(y, r, dy.to(dt), retain_graph=True)
        dx, dw, dg, db = torch.autograd.grad(y, leaves, dy.to(dt))
        out[key] = dict(y=y.detach(), dr=dr, dx=dx, dw=dw, dgamma=dg, dbeta=db, r=r.detach())
        leaves, r, _ = _compose(x, w, gamma, beta, G, s, dt)
        out[key]['conv_dx'], out[key]['conv_dw'] = torch.autograd.grad(r, leaves[:2], dy.to(dt))       # the convolution alone, dy as the gradient of r
    return out


@functools.lru_cache(maxsize=None)
def conv_case(name):
    """Gaussian operands as `_block_operands` draws them (seed SEEDS[0]), the float64 autograd of F.conv2d and torch's fp32 one: keys
    `conv_dw`, `conv_dx`, judged by `bound` like the block cases'"""
    shape = CONV_CASES[name]
    s = shape[6]
    x, w, _, _, dy = _block_operands(shape + (32,), SEEDS[0])
    out = dict(x=x, w=w, dy=dy, stride=s, k=shape[5], seed=SEEDS[0])
    for key, dt in (('ref', torch.float64), ('f32', torch.float32)):
        xx, ww = (t.detach().to(dt).clone().requires_grad_() for t in (x, w))
        dx, dw = torch.autograd.grad(F.conv2d(xx, ww, None, s, shape[5] // 2), (xx, ww), dy.to(dt))
        out[key] = dict(conv_dx=dx, conv_dw=dw)
    return out


# ---------------------------------------------------------------------------------------------- the whole wrapper
def fpn_module(vkn, seed, dtype, fused_backward=False, C=None):
    """a `SemanticFPNWrapper` of the shipped structure at FPN_CFG's size with seeded parameters (GroupNorm affines away from 1 / 0)"""
    C = C or FPN_CFG['C']
    m = vkn.semantic_fpn.SemanticFPNWrapper(C, C, C, 0, 3, positional_encoding=dict(type='SinePositionalEncoding', num_feats=C // 2, normalize=True),
                                            cat_coors_level=3, upsample_times=2, num_aux_convs=1, norm_cfg=dict(type='GN', num_groups=FPN_CFG['groups']),
                                            fused_backward=fused_backward)
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in sorted(m.named_parameters()):
            if name.endswith('conv.weight'):
                p.copy_(0.05 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
            elif name.endswith('gn.weight'):
                p.copy_(_signed(gen, p.shape, 0.5, 1.5))
            else:
                p.copy_(0.3 * torch.randn(p.shape, generator=gen, dtype=torch.float64))
    return m.to(dtype)


def fpn_inputs(seed):
    gen = torch.Generator().manual_seed(seed + 1)
    B, C = FPN_CFG['B'], FPN_CFG['C']
    xs = [torch.randn((B, C, h, w), generator=gen, dtype=torch.float64).float() for h, w in FPN_CFG['sizes']]
    gs = [torch.randn((B, C) + FPN_CFG['sizes'][1], generator=gen, dtype=torch.float64).float() for _ in range(2)]
    return xs, gs


def _fpn_run(mod, xs, gs, dt, pre=None):
    hooks = []
    if pre is not None:
        for m in mod.modules():
            if isinstance(m, torch.nn.GroupNorm):
                hooks.append(m.register_forward_hook(lambda _m, _i, o: pre.append(float(o.detach().abs().min()))))
    ins = [x.detach().to(dt).clone().requires_grad_() for x in xs]
    outs = mod.forward_torch(ins)
    for h in hooks:
        h.remove()
    params = [p for _, p in sorted(mod.named_parameters())]
    grads = torch.autograd.grad(outs, ins + params, [g.to(dt) for g in gs])
    res = {f'out{i}': o.detach() for i, o in enumerate(outs)}
    res.update({f'd_p{i + 2}': g for i, g in enumerate(grads[:4])})
    res.update({'d_' + n: g for (n, _), g in zip(sorted(mod.named_parameters()), grads[4:])})
    return res


@functools.lru_cache(maxsize=None)
def fpn_case(vkn):
    """the first seed of SEEDS whose float64 pre-activations (the outputs of every GroupNorm) all clear BLOCK_MARGIN"""
    for seed in SEEDS:
        xs, gs = fpn_inputs(seed)
        pre = []
        ref = _fpn_run(fpn_module(vkn, seed, torch.float64), xs, gs, torch.float64, pre)
        if min(pre) >= BLOCK_MARGIN:
            break
    else:
        raise AssertionError(f'no seed of {SEEDS} clears the ReLU margin in every layer')
    f32 = _fpn_run(fpn_module(vkn, seed, torch.float32), xs, gs, torch.float32)
    return dict(seed=seed, xs=xs, gs=gs, ref=ref, f32=f32, pre_min=min(pre))
