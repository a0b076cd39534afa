"""References, bound and cases of the deformable-attention neck's tests (tests/test_msda_refs.py proves their premises on the CPU;
tests/test_gpu_msda.py and tests/test_msdeform_decoder.py use them).  Independent of the package: nothing here imports it.

  * `core_f64`: the sampling core of include/vkn_msda.h in float64, written with explicit corner indexing (no grid_sample);
  * `core_grid_sample`: the same core as torch's composition on `F.grid_sample` (mmcv's `multi_scale_deformable_attn_pytorch`), in any
    dtype: in float64 it must agree with `core_f64` to 1e-12, in fp32 it is the YARDSTICK of the per-element bound;
  * `decoder_f64`: the whole forward of knet/det/msdeformattn_decoder.py:165-275 from a state dict, in float64 on functional torch ops,
    with the attention / layer / FFN of mmcv 1.x restated (the reference's own Python imports an mmdet class whose source is not at
    hand, so no fixture can be generated from it);
  * the bound: max-abs error against float64 <= max(8 x the error of torch's fp32 composition against the same float64, 4 fp32 ulps of
    the tensor's largest magnitude) — the repository's rule for a re-ordered fp32 sum (tests/test_gpu_fpn_bwd.py);
  * the case tables.

Bands of a sampled pixel coordinate y on a level of height H (x, W likewise): LOW (-1, 0) — the upper corner row lies outside; HIGH
[H - 1, H) — the lower one does; OUT y <= -1 or y >= H — the point fails the four comparisons and contributes nothing; IN [0, H - 1).
`draw_core` draws every coordinate's band first (LOW 0.24, HIGH 0.24, IN 0.20, OUT 0.32), independently per axis, so that per axis at
least 20 % of the points lie in LOW and 20 % in HIGH, at least 20 % of the points are OUT in x with y inside, and more than 20 % fail
the test altogether; `band_shares` measures it."""
import collections
import math

import numpy as np
import torch
import torch.nn.functional as F

CoreCase = collections.namedtuple('CoreCase', 'B Q M D P shapes spread')      # spread: half-width of the raw logits

LV3 = ((2, 3), (4, 5), (7, 9))
CORE_CASES = {
    'shipped-89': CoreCase(2, 89, 8, 32, 4, LV3, 2.0),                        # Q = S = 89
    'q5-of-89': CoreCase(2, 5, 8, 32, 4, LV3, 2.0),                           # Q != S
    'm4-d64': CoreCase(2, 89, 4, 64, 4, LV3, 2.0),
    'm8-d16': CoreCase(2, 89, 8, 16, 4, LV3, 2.0),
    'l1-p1': CoreCase(2, 20, 8, 32, 1, ((4, 5),), 2.0),
    'l4-p8': CoreCase(2, 90, 8, 32, 8, ((1, 1),) + LV3, 2.0),                 # with the 1 x 1 level in front: every start index moves
    'one-pixel': CoreCase(2, 7, 8, 32, 4, ((1, 1),), 2.0),
    'row-130': CoreCase(1, 33, 8, 32, 4, ((3, 130),), 2.0),                   # a row longer than any plausible tile
    'spread-80': CoreCase(2, 89, 8, 32, 4, LV3, 80.0),                        # exp(80) = 5.5e34: the sum's last decades of fp32
    'spread-100': CoreCase(1, 89, 8, 32, 4, LV3, 100.0),                      # exp(100) overflows a softmax that skips the max subtraction
}
BANDS_ASSERTED = ('shipped-89', 'm4-d64', 'm8-d16', 'spread-80', 'spread-100')             # the cases on the three levels 2x3, 4x5, 7x9 with Q = 89

ExactCase = collections.namedtuple('ExactCase', 'B M D P shapes')              # Q = the pixels of the first level
EXACT_CASES = {
    'lp1': ExactCase(2, 8, 32, 1, ((4, 8),)),
    'lp2-levels': ExactCase(2, 8, 32, 1, ((4, 8), (2, 4))),
    'lp2-points': ExactCase(1, 4, 64, 2, ((8, 4),)),
    'lp4': ExactCase(2, 8, 32, 2, ((8, 16), (4, 4))),
    'lp4-d16': ExactCase(1, 8, 16, 1, ((8, 8), (4, 4), (2, 2), (1, 1))),
    'lp4-one-level': ExactCase(1, 8, 32, 4, ((2, 16),)),
}

MODULE_CASES = {
    'narrow': dict(feat_channels=64, num_heads=4, in_channels=[32, 64, 96, 128], num_layers=2, sizes=((16, 24), (8, 12), (4, 6), (2, 3)), B=1),
    'shipped': dict(feat_channels=256, num_heads=8, in_channels=[256, 512, 1024, 2048], num_layers=6,
                    sizes=((8, 12), (4, 6), (2, 3), (1, 2)), B=2),
}


class PremiseError(AssertionError):
    """a case does not have the property its test relies on: a bug of the test, not of the code under test"""


# ---------------------------------------------------------------------------------------------------------------- the core
def _starts(shapes):
    out, s = [], 0
    for h, w in shapes:
        out.append(s)
        s += h * w
    return out, s


def pixel_coords(shapes, off, ref):
    """(x, y) [B, Q, M, L, P] in pixels of each level, in the dtype of `off` / `ref`: loc = ref + off / (W, H), x = loc.x W - 0.5"""
    wh = torch.tensor([[w, h] for h, w in shapes], dtype=off.dtype)
    loc = ref[None, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    xy = loc * wh[None, None, None, :, None, :] - 0.5
    return xy[..., 0], xy[..., 1]


def core_f64(value, shapes, off, logits, ref):
    """value [B, S, M, D], off [B, Q, M, L, P, 2], logits [B, Q, M, L P], ref [Q, L, 2] -> [B, Q, M D] in float64, every corner indexed
    explicitly: a point counts if y > -1, x > -1, y < H, x < W, a corner if it lies inside the level."""
    value, off, logits, ref = (t.double() for t in (value, off, logits, ref))
    B, S, M, D = value.shape
    _, Q, _, L, P, _ = off.shape
    w = torch.softmax(logits - logits.max(-1, keepdim=True)[0], -1).view(B, Q, M, L, P)
    x, y = pixel_coords(shapes, off, ref)
    starts, total = _starts(shapes)
    assert total == S
    out = torch.zeros(B, Q, M, D, dtype=torch.float64)
    bi = torch.arange(B).view(B, 1, 1, 1).expand(B, Q, M, P)
    mi = torch.arange(M).view(1, 1, M, 1).expand(B, Q, M, P)
    for l, (H, W) in enumerate(shapes):
        xl, yl = x[:, :, :, l], y[:, :, :, l]                                                    # [B, Q, M, P]
        ok = (yl > -1) & (xl > -1) & (yl < H) & (xl < W)
        xs, ys = torch.where(ok, xl, torch.zeros_like(xl)), torch.where(ok, yl, torch.zeros_like(yl))
        x0, y0 = torch.floor(xs), torch.floor(ys)
        lw, lh = xs - x0, ys - y0
        x0, y0 = x0.long(), y0.long()
        acc = torch.zeros(B, Q, M, P, D, dtype=torch.float64)
        for dy, dx, wt in ((0, 0, (1 - lh) * (1 - lw)), (0, 1, (1 - lh) * lw), (1, 0, lh * (1 - lw)), (1, 1, lh * lw)):
            yy, xx = y0 + dy, x0 + dx
            inside = ok & (yy >= 0) & (yy <= H - 1) & (xx >= 0) & (xx <= W - 1)
            idx = starts[l] + yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)
            v = value[bi, idx, mi]                                                                 # [B, Q, M, P, D]
            acc += torch.where(inside[..., None], v * wt[..., None], torch.zeros_like(v))
        out += (acc * w[:, :, :, l, :, None]).sum(3)
    return out.view(B, Q, M * D)


def core_grid_sample(value, shapes, off, logits, ref, dtype=torch.float32):
    """torch's composition (mmcv's `multi_scale_deformable_attn_pytorch` behind the attention's own softmax and location arithmetic)"""
    value, off, logits, ref = (t.to(dtype) for t in (value, off, logits, ref))
    B, S, M, D = value.shape
    _, Q, _, L, P, _ = off.shape
    w = logits.softmax(-1).view(B, Q, M, L, P)
    wh = torch.tensor([[w_, h_] for h_, w_ in shapes], dtype=dtype)
    loc = ref[None, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
    grids = 2 * loc - 1
    sampled = []
    for l, v in enumerate(value.split([h * w_ for h, w_ in shapes], dim=1)):
        H, W = shapes[l]
        v = v.flatten(2).transpose(1, 2).reshape(B * M, D, H, W)
        g = grids[:, :, :, l].transpose(1, 2).flatten(0, 1)
        sampled.append(F.grid_sample(v, g, mode='bilinear', padding_mode='zeros', align_corners=False))
    ww = w.transpose(1, 2).reshape(B * M, 1, Q, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * ww).sum(-1).view(B, M * D, Q)
    return out.transpose(1, 2).contiguous()


def pixel_centres(shapes, Q=None):
    """ref [Q, L, 2]: the (x, y) pixel centres of the concatenated levels, normalised, the same for every l — the decoder's reference
    points (knet/det/msdeformattn_decoder.py:198-202, 230-231); with `Q` the first Q of them"""
    pts = [torch.stack([(torch.arange(w, dtype=torch.float64).repeat(h) + 0.5) / w,
                        (torch.arange(h, dtype=torch.float64).repeat_interleave(w) + 0.5) / h], -1) for h, w in shapes]
    ref = torch.cat(pts, 0)[:Q]
    return ref[:, None].repeat(1, len(shapes), 1).float()


_BAND_P = (0.24, 0.24, 0.20, 0.32)      # LOW, HIGH, IN, OUT


def _draw_axis(n, band, rng):
    """pixel coordinates [.., L-th axis of size n] by band; a 1-pixel axis has no IN band: LOW instead"""
    u = rng.random(band.shape)
    side = rng.random(band.shape) < 0.5
    low, high = -1 + 0.98 * u + 0.01, (n - 1) + 0.98 * u + 0.01
    inner = u * (n - 1) if n > 1 else low
    outer = np.where(side, -1.0 - 2.5 * u, n + 2.5 * u)
    return np.select([band == 0, band == 1, band == 2], [low, high, inner], outer)


def draw_core(case, seed):
    """fp32 inputs of a core case: value ~ N(0, 1), logits uniform in [-spread, spread], ref = the levels' pixel centres (the first Q),
    offsets that put every point into its drawn band"""
    rng = np.random.default_rng(seed)
    B, Q, M, D, P, shapes = case.B, case.Q, case.M, case.D, case.P, case.shapes
    L, (_, S) = len(shapes), _starts(shapes)
    value = torch.from_numpy(rng.standard_normal((B, S, M, D)).astype(np.float32))
    logits = torch.from_numpy(rng.uniform(-case.spread, case.spread, (B, Q, M, L * P)).astype(np.float32))
    ref = pixel_centres(shapes)
    ref = ref[torch.from_numpy(rng.permutation(ref.shape[0])[:Q]).sort()[0]] if Q < ref.shape[0] else ref[:Q]
    if ref.shape[0] < Q:                                                      # more queries than pixels: random reference points
        extra = torch.from_numpy(rng.random((Q - ref.shape[0], 1, 2)).astype(np.float32)).repeat(1, L, 1)
        ref = torch.cat([ref, extra], 0)
    off = np.zeros((B, Q, M, L, P, 2), dtype=np.float64)
    for l, (H, W) in enumerate(shapes):
        for axis, n in ((0, W), (1, H)):
            band = rng.choice(4, size=(B, Q, M, P), p=_BAND_P)
            coord = _draw_axis(n, band, rng)
            off[:, :, :, l, :, axis] = coord + 0.5 - ref[None, :, None, l, None, axis].double().numpy() * n
    return value, torch.from_numpy(off.astype(np.float32)), logits, ref.contiguous()


def band_shares(shapes, off, ref):
    """the shares of the points (float64 evaluation of the fp32 inputs) per band: low_x, low_y, high_x, high_y, fail (the point fails
    the four comparisons), xout_yin"""
    x, y = pixel_coords(shapes, off.double(), ref.double())
    H = torch.tensor([h for h, _ in shapes], dtype=torch.float64).view(1, 1, 1, -1, 1)
    W = torch.tensor([w for _, w in shapes], dtype=torch.float64).view(1, 1, 1, -1, 1)
    xin, yin = (x > -1) & (x < W), (y > -1) & (y < H)
    share = lambda m: float(m.double().mean())                                # noqa: E731
    return dict(low_x=share(xin & (x < 0)), low_y=share(yin & (y < 0)), high_x=share(xin & (x >= W - 1)), high_y=share(yin & (y >= H - 1)),
                fail=share(~(xin & yin)), xout_yin=share(~xin & yin))


def draw_exact(case, seed):
    """integer values |v| <= 64, power-of-two level sizes, reference points at the pixel centres of the first level, offsets in
    multiples of 1/4 pixel in [-3, 3], equal logits over L P in {1, 2, 4}: every product and sum of the core is exact in fp32"""
    rng = np.random.default_rng(seed)
    B, M, D, P, shapes = case.B, case.M, case.D, case.P, case.shapes
    L, (_, S) = len(shapes), _starts(shapes)
    if L * P not in (1, 2, 4) or any(h & (h - 1) or w & (w - 1) for h, w in shapes):
        raise PremiseError(f'{case}: L P must be 1, 2 or 4 and every level size a power of two')
    H0, W0 = shapes[0]
    Q = H0 * W0
    value = torch.from_numpy(rng.integers(-64, 65, (B, S, M, D)).astype(np.float32))
    off = torch.from_numpy((rng.integers(-12, 13, (B, Q, M, L, P, 2)) / 4.0).astype(np.float32))
    logits = torch.full((B, Q, M, L * P), float(rng.integers(-3, 4)), dtype=torch.float32)
    ref = pixel_centres(shapes[:1])[:, :1].repeat(1, L, 1).contiguous()
    return value, off, logits, ref


def exact_premise(case, value, off, logits, ref):
    """what makes a case exact, from the actual operands: every coordinate a multiple of 2^-6 below 2^10, every value an integer of at
    most 64, every softmax weight 1 / (L P): each term weight x value is then a multiple of 2^-14 below 2^7 and a sum of 4 L P <= 16
    of them needs at most 25 - 1 bits ... asserted directly: the float64 result is a multiple of 2^-14 below 2^10 (24 bits)"""
    x, y = pixel_coords(case.shapes, off.double(), ref.double())
    for c in (x, y):
        if not torch.equal(c * 64, (c * 64).round()) or float(c.abs().max()) >= 1024:
            raise PremiseError(f'{case}: a pixel coordinate is not a multiple of 1/64')
    if not torch.equal(value, value.round()) or float(value.abs().max()) > 64:
        raise PremiseError(f'{case}: values are not integers of at most 64')
    if float(logits.max() - logits.min()) != 0.0:
        raise PremiseError(f'{case}: logits are not equal')
    out = core_f64(value, case.shapes, off, logits, ref)
    if not torch.equal(out * 2 ** 14, (out * 2 ** 14).round()) or float(out.abs().max()) >= 2 ** 10:
        raise PremiseError(f'{case}: the float64 result does not fit 24 bits')
    if not torch.equal(out.float().double(), out):
        raise PremiseError(f'{case}: the float64 result is not an fp32 number')
    if float((out != 0).double().mean()) < 0.3:
        raise PremiseError(f'{case}: vacuous, {float((out != 0).double().mean()):.2f} of the outputs are non-zero')
    return out


# ---------------------------------------------------------------------------------------------------------------- the bound
def ulp32(magnitude):
    return 2.0 ** (math.floor(math.log2(max(float(magnitude), 2.0 ** -126))) - 23)


def bound(ref64, yard32):
    """max(8 x max |yard32 - ref64|, 4 fp32 ulps of max |ref64|)"""
    yard = float((yard32.detach().cpu().double() - ref64).abs().max())
    return max(8.0 * yard, 4.0 * ulp32(ref64.abs().max())), yard


def judge(got, ref64, yard32):
    """(error, bound, error / bound, yardstick's error) of one tensor"""
    err = float((got.detach().cpu().double() - ref64).abs().max())
    b, yard = bound(ref64, yard32)
    return err, b, err / b, yard


# ---------------------------------------------------------------------------------------------------------------- the decoder
def sine_encoding_f64(h, w, num_feats=128, temperature=10000, scale=2 * math.pi, eps=1e-6):
    """mmdet 2.18 `SinePositionalEncoding(normalize=True)` of an all-valid [h, w] mask -> [2 num_feats, h, w] (pos_y, then pos_x)"""
    y = torch.arange(1, h + 1, dtype=torch.float64).view(h, 1).expand(h, w) / (h + eps) * scale
    x = torch.arange(1, w + 1, dtype=torch.float64).view(1, w).expand(h, w) / (w + eps) * scale
    dim_t = temperature ** (2 * (torch.arange(num_feats, dtype=torch.float64) // 2) / num_feats)
    px, py = x[:, :, None] / dim_t, y[:, :, None] / dim_t
    px = torch.stack((px[:, :, 0::2].sin(), px[:, :, 1::2].cos()), dim=3).flatten(2)
    py = torch.stack((py[:, :, 0::2].sin(), py[:, :, 1::2].cos()), dim=3).flatten(2)
    return torch.cat((py, px), dim=2).permute(2, 0, 1)


def _conv_module(sd, prefix, x, groups, padding=0, relu=False):
    x = F.conv2d(x, sd[prefix + '.conv.weight'], sd.get(prefix + '.conv.bias'), padding=padding)
    x = F.group_norm(x, groups, sd[prefix + '.gn.weight'], sd[prefix + '.gn.bias'], eps=1e-5)
    return x.relu() if relu else x


def decoder_f64(state_dict, feats, num_heads=8, num_points=4, num_outs=3, num_groups=32):
    """The decoder's forward in float64 from a state dict in the reference's key names -> the reference's tuple
    (mask_feature, then the multi-scale features from high to low resolution)."""
    sd = {k: v.detach().cpu().double() for k, v in state_dict.items()}
    feats = [f.detach().cpu().double() for f in feats]
    n_in = len(feats)
    L, C = sd['level_encoding.weight'].shape
    n_layers = 1 + max(int(k.split('.')[2]) for k in sd if k.startswith('encoder.layers.'))
    M, P = num_heads, num_points
    B = feats[0].shape[0]
    shapes, xs, poss = [], [], []
    for i in range(L):
        f = feats[n_in - i - 1]
        h, w = f.shape[-2:]
        shapes.append((h, w))
        xs.append(_conv_module(sd, f'input_convs.{i}', f, num_groups).flatten(2).transpose(1, 2))            # [B, hw, C]
        poss.append((sd['level_encoding.weight'][i].view(-1, 1, 1) + sine_encoding_f64(h, w, C // 2)).flatten(1).t())
    x, pos = torch.cat(xs, 1), torch.cat(poss, 0)                                                             # [B, Q, C], [Q, C]
    pts =[torch.stack([(torch.arange(w, dtype=torch.float64).repeat(h) + 0.5) / w,
                        (torch.arange(h, dtype=torch.float64).repeat_interleave(w) + 0.5) / h], -1) for h, w in shapes]
    ref = torch.cat(pts, 0)[:, None].repeat(1, L, 1)                                                          # float64 all the way
    Q = x.shape[1]
    for n in range(n_layers):
        a, f = f'encoder.layers.{n}.attentions.0.', f'encoder.layers.{n}.ffns.0.layers.'
        q = x + pos
        value = F.linear(x, sd[a + 'value_proj.weight'], sd[a + 'value_proj.bias']).view(B, Q, M, C // M)
        off = F.linear(q, sd[a + 'sampling_offsets.weight'], sd[a + 'sampling_offsets.bias']).view(B, Q, M, L, P, 2)
        logits = F.linear(q, sd[a + 'attention_weights.weight'], sd[a + 'attention_weights.bias']).view(B, Q, M, L * P)
        core = core_f64(value, shapes, off, logits, ref)
        x = x + F.linear(core, sd[a + 'output_proj.weight'], sd[a + 'output_proj.bias'])
        x = F.layer_norm(x, (C,), sd[f'encoder.layers.{n}.norms.0.weight'], sd[f'encoder.layers.{n}.norms.0.bias'], 1e-5)
        hid = F.linear(x, sd[f + '0.0.weight'], sd[f + '0.0.bias']).relu()
        x = x + F.linear(hid, sd[f + '1.weight'], sd[f + '1.bias'])
        x = F.layer_norm(x, (C,), sd[f'encoder.layers.{n}.norms.1.weight'], sd[f'encoder.layers.{n}.norms.1.bias'], 1e-5)
    outs = [o.transpose(1, 2).reshape(B, C, h, w) for o, (h, w) in zip(x.split([h * w for h, w in shapes], dim=1), shapes)]
    for i in range(n_in - L - 1, -1, -1):
        cur = _conv_module(sd, f'lateral_convs.{i}', feats[i], num_groups)
        y = cur + F.interpolate(outs[-1], size=cur.shape[-2:], mode='bilinear', align_corners=False)
        outs.append(_conv_module(sd, f'output_convs.{i}', y, num_groups, padding=1, relu=True))
    res = outs[:num_outs]
    res.append(F.conv2d(outs[-1], sd['mask_feature.weight'], sd['mask_feature.bias']))
    res.reverse()
    return tuple(res)


def expected_keys(num_layers=6, num_encoder_levels=3, num_fpn_levels=1):
    keys = ['level_encoding.weight', 'mask_feature.weight', 'mask_feature.bias']
    for i in range(num_encoder_levels):
        keys += [f'input_convs.{i}.conv.weight', f'input_convs.{i}.conv.bias', f'input_convs.{i}.gn.weight', f'input_convs.{i}.gn.bias']
    for i in range(num_fpn_levels):
        for part in ('lateral_convs', 'output_convs'):
            keys += [f'{part}.{i}.conv.weight', f'{part}.{i}.gn.weight', f'{part}.{i}.gn.bias']
    for n in range(num_layers):
        for lin in ('sampling_offsets', 'attention_weights', 'value_proj', 'output_proj'):
            keys += [f'encoder.layers.{n}.attentions.0.{lin}.weight', f'encoder.layers.{n}.attentions.0.{lin}.bias']
        for lin in ('0.0', '1'):
            keys += [f'encoder.layers.{n}.ffns.0.layers.{lin}.weight', f'encoder.layers.{n}.ffns.0.layers.{lin}.bias']
        for k in (0, 1):
            keys += [f'encoder.layers.{n}.norms.{k}.weight', f'encoder.layers.{n}.norms.{k}.bias']
    return sorted(keys)


def module_cfg(case, base):
    """the neck dict of a module case: the shipped dict `base` at the case's widths"""
    import copy
    cfg = copy.deepcopy(base)
    c, heads = case['feat_channels'], case['num_heads']
    cfg.update(in_channels=list(case['in_channels']), feat_channels=c, out_channels=c)
    cfg['encoder']['num_layers'] = case['num_layers']
    layer = cfg['encoder']['transformerlayers']
    layer['attn_cfgs'].update(embed_dims=c, num_heads=heads)
    layer['ffn_cfgs'].update(embed_dims=c)
    cfg['positional_encoding']['num_feats'] = c // 2
    return cfg


def randomise(module, seed):
    """parameters that exercise every term: the decoder's own init leaves the offsets' weight and the attention weights at zero"""
    gen = torch.Generator().manual_seed(seed)
    with torch.no_grad():
        for name, p in module.named_parameters():
            if name.endswith('sampling_offsets.bias'):
                p.add_(torch.randn(p.shape, generator=gen) * 0.5)
            elif name.endswith('sampling_offsets.weight'):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.05)
            elif name.endswith('attention_weights.weight'):
                p.copy_(torch.randn(p.shape, generator=gen) * 0.1)
            elif name.endswith(('gn.weight', 'norms.0.weight', 'norms.1.weight')):
                p.copy_(1 + 0.2 * torch.randn(p.shape, generator=gen))
            elif name.endswith('.bias'):
                p.add_(torch.randn(p.shape, generator=gen) * 0.1)


def module_inputs(case, seed):
    gen = torch.Generator().manual_seed(seed)
    return [torch.randn((case['B'], c, h, w), generator=gen) for c, (h, w) in zip(case['in_channels'], case['sizes'])]
