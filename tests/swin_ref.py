"""The Swin backbone's lines (swin/swin_transformer.py) restated for the tests, literally: the pad, the two rolls, the window partition and
its reverse, the gathered relative-position bias and the painted mask are FORMED as tensors, as the reference forms them, in the dtype of
the inputs (float64 for the yardstick).  Nothing here shares the index arithmetic of csrc/vkn_swin.hip or imports the package's swin.py.
Also the case builders of tests/test_gpu_swin.py and tests/test_swin_refs.py.

Two entry levels:
  * `core(qkv, qkv_bias, table, ...)`: from the rows of the qkv Linear on the tokens as they are, [B, H, W, 3, heads, hd].  The reference
    pads BEFORE that Linear, so a pad token's row is the Linear's bias: the pad is filled with it.  Returns the output in the tokens' order
    and, per query, what the selector tests need (the lead of its best score, the winner's v row, whether the winner is a pad token,
    the regions of both).
  * `block`, `layer`, `backbone`: from a state dict (the reference's keys) and the input, every Linear / LayerNorm / GELU in torch."""
import math

import torch
import torch.nn.functional as F

MASK = -100.0


def partition(x, ws):
    B, H, W, C = x.shape
    x = x.view(B, H // ws, ws, W // ws, ws, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, ws, ws, C)


def reverse(windows, ws, H, W):
    B = int(windows.shape[0] / (H * W / ws / ws))
    x = windows.view(B, H // ws, W // ws, ws, ws, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def rel_index(ws):
    """relative_position_index of a ws x ws window, built as WindowAttention.__init__ builds it"""
    coords = torch.stack(torch.meshgrid([torch.arange(ws), torch.arange(ws)], indexing='ij'))
    flat = torch.flatten(coords, 1)
    rel = (flat[:, :, None] - flat[:, None, :]).permute(1, 2, 0).contiguous()
    rel[:, :, 0] += ws - 1
    rel[:, :, 1] += ws - 1
    rel[:, :, 0] *= 2 * ws - 1
    return rel.sum(-1)


def painted_regions(Hp, Wp, ws, shift):
    """img_mask of BasicLayer.forward: [Hp, Wp] of region counts 0..8"""
    img = torch.zeros((1, Hp, Wp, 1))
    slices = (slice(0, -ws), slice(-ws, -shift), slice(-shift, None))
    cnt = 0
    for h in slices:
        for w in slices:
            img[:, h, w, :] = cnt
            cnt += 1
    return img


def painted_mask(H, W, ws, shift, dtype):
    Hp, Wp = int(math.ceil(H / ws)) * ws, int(math.ceil(W / ws)) * ws
    mw = partition(painted_regions(Hp, Wp, ws, shift), ws).view(-1, ws * ws)
    m = mw.unsqueeze(1) - mw.unsqueeze(2)
    return m.masked_fill(m != 0, float(MASK)).masked_fill(m == 0, float(0.0)).to(dtype=dtype)


def attend(qkv_windows, table, ws, heads, scale, mask):
    """WindowAttention.forward between its two Linears.  qkv_windows [B nW, N, 3 C] -> (x [B nW, N, C], scores [B nW, heads, N, N])"""
    B_, N, C3 = qkv_windows.shape
    C = C3 // 3
    qkv = qkv_windows.reshape(B_, N, 3, heads, C // heads).permute(2, 0, 3, 1, 4)
    q, k, v = qkv[0], qkv[1], qkv[2]
    q = q * scale
    attn = q @ k.transpose(-2, -1)
    bias = table[rel_index(ws).view(-1).to(table.device)].view(N, N, -1).permute(2, 0, 1).contiguous()
    attn = attn + bias.unsqueeze(0)
    if mask is not None:
        nW = mask.shape[0]
        attn = attn.view(B_ // nW, nW, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)
        attn = attn.view(-1, heads, N, N)
    scores = attn
    attn = torch.softmax(attn, dim=-1)
    return (attn @ v).transpose(1, 2).reshape(B_, N, C), scores


def _windows_of(x, ws, shift):
    """[B, Hp, Wp, C] -> rolled and partitioned [B nW, N, C]"""
    if shift > 0:
        x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
    return partition(x, ws).view(-1, ws * ws, x.shape[-1])


def _map_of(windows, ws, shift, Hp, Wp, H, W):
    """the way back: reverse, roll back, crop -> [B, H, W, C]"""
    x = reverse(windows.reshape(-1, ws, ws, windows.shape[-1]), ws, Hp, Wp)
    if shift > 0:
        x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
    return x[:, :H, :W, :].contiguous()


def core(qkv, qkv_bias, table, heads, ws, shift, scale, details=False):
    """qkv [B, H, W, 3, heads, hd], qkv_bias [3 heads hd] or None, table [(2 ws - 1)^2, heads] -> out [B, H, W, heads hd] in qkv's
    dtype.  With details: also a dict of per-query tensors in the tokens' order, [B, H, W, heads] unless said:
    lead (best score minus second best), winner_v [B, H, W, heads hd] (the v row of the best key), winner_pad, winner_region, winner_slot
    (the winner's place y ws + x in the window), region and slot [B, H, W] (the query's painted region on the rolled map, 0 everywhere
    when shift = 0, and its place in its window)."""
    B, H, W = qkv.shape[:3]
    hd = qkv.shape[-1]
    C = heads * hd
    rows = qkv.reshape(B, H, W, 3 * C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(rows, (0, 0, 0, pad_r, 0, pad_b))
    _, Hp, Wp, _ = x.shape
    live = F.pad(torch.ones((B, H, W, 1), dtype=qkv.dtype, device=qkv.device), (0, 0, 0, pad_r, 0, pad_b))
    if qkv_bias is not None:                                    # the Linear on a zero row: its bias
        x = x + (1 - live) * qkv_bias.to(qkv.dtype).view(1, 1, 1, -1)
    mask = painted_mask(H, W, ws, shift, qkv.dtype).to(qkv.device) if shift > 0 else None
    windows = _windows_of(x, ws, shift)
    y, scores = attend(windows, table, ws, heads, scale, mask)
    out = _map_of(y, ws, shift, Hp, Wp, H, W)
    if not details:
        return out
    N = ws * ws
    top2 = scores.topk(min(2, N), dim=-1)
    lead = (top2.values[..., 0] - top2.values[..., 1]) if N > 1 else torch.full_like(top2.values[..., 0], float('inf'))
    win = top2.indices[..., 0]                                                   # [B nW, heads, N]
    v = windows.reshape(-1, N, 3, heads, hd)[:, :, 2]                            # [B nW, N, heads, hd]
    wv = torch.gather(v.permute(0, 2, 1, 3), 2, win.unsqueeze(-1).expand(-1, -1, -1, hd))      # [B nW, heads, N, hd]
    pads = _windows_of(1 - live, ws, shift)[..., 0]                              # [B nW, N]
    regions = painted_regions(Hp, Wp, ws, shift) if shift > 0 else torch.zeros((1, Hp, Wp, 1))
    reg = partition(regions.to(qkv.device).expand(B, -1, -1, -1).contiguous(), ws).view(-1, N)      # painted on the ROLLED map: no roll
    wpad = torch.gather(pads.unsqueeze(1).expand(-1, heads, -1), 2, win)
    wreg = torch.gather(reg.unsqueeze(1).expand(-1, heads, -1), 2, win)
    back = lambda t: _map_of(t, ws, shift, Hp, Wp, H, W)                        # noqa: E731
    return out, dict(lead=back(lead.permute(0, 2, 1)), winner_v=back(wv.permute(0, 2, 1, 3).reshape(-1, N, C)),
                     winner_pad=back(wpad.permute(0, 2, 1)) > 0, winner_region=back(wreg.permute(0, 2, 1)).long(),
                     winner_slot=back(win.permute(0, 2, 1).to(qkv.dtype)).long(), region=back(reg.unsqueeze(-1))[..., 0].long(),
                     slot=back(torch.arange(N, dtype=qkv.dtype, device=qkv.device).expand(win.shape[0], N).unsqueeze(-1))[..., 0].long())


# ------------------------------------------------------------------------------------------------ module level, from a state dict
def _ln(x, sd, p):
    return F.layer_norm(x, (x.shape[-1],), sd[p + '.weight'], sd[p + '.bias'], 1e-5)


def _lin(x, sd, p):
    return F.linear(x, sd[p + '.weight'], sd.get(p + '.bias'))


def block(sd, p, x, H, W, heads, ws, shift, mask):
    """SwinTransformerBlock.forward in eval mode.  x [B, H W, C]; `p` the block's key prefix (with its dot)"""
    B, L, C = x.shape
    shortcut = x
    x = _ln(x, sd, p + 'norm1').view(B, H, W, C)
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
    _, Hp, Wp, _ = x.shape
    windows = _windows_of(x, ws, shift)
    table = sd[p + 'attn.relative_position_bias_table']
    y, _ = attend(_lin(windows, sd, p + 'attn.qkv'), table, ws, heads, (C // heads) ** -0.5, mask if shift > 0 else None)
    y = _lin(y, sd, p + 'attn.proj')
    x = _map_of(y, ws, shift, Hp, Wp, H, W).view(B, H * W, C)
    x = shortcut + x
    return x + _lin(F.gelu(_lin(_ln(x, sd, p + 'norm2'), sd, p + 'mlp.fc1')), sd, p + 'mlp.fc2')


def merge(sd, p, x, H, W):
    """PatchMerging.forward"""
    B, L, C = x.shape
    x = x.view(B, H, W, C)
    if (H % 2 == 1) or (W % 2 == 1):
        x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
    x = torch.cat([x[:, 0::2, 0::2, :], x[:, 1::2, 0::2, :], x[:, 0::2, 1::2, :], x[:, 1::2, 1::2, :]], -1).view(B, -1, 4 * C)
    return F.linear(_ln(x, sd, p + 'norm'), sd[p + 'reduction.weight'])


def layer(sd, p, x, H, W, depth, heads, ws, downsample):
    """BasicLayer.forward -> (x_out, x_down or x_out, Wh, Ww)"""
    shift = ws // 2
    mask = painted_mask(H, W, ws, shift, x.dtype).to(x.device)
    for i in range(depth):
        x = block(sd, f'{p}blocks.{i}.', x, H, W, heads, ws, 0 if i % 2 == 0 else shift, mask)
    if downsample:
        return x, merge(sd, p + 'downsample.', x, H, W), (H + 1) // 2, (W + 1) // 2
    return x, x, H, W


def backbone(sd, img, embed_dims, depths, num_heads, ws=7, patch=4, out_indices=(0, 1, 2, 3)):
    """SwinTransformerDIY.forward (patch_norm on, no absolute position embedding) -> tuple of [B, C_i, H_i, W_i]"""
    _, _, H, W = img.shape
    if W % patch != 0:
        img = F.pad(img, (0, patch - W % patch))
    if H % patch != 0:
        img = F.pad(img, (0, 0, 0, patch - H % patch))
    x = F.conv2d(img, sd['patch_embed.proj.weight'], sd['patch_embed.proj.bias'], stride=patch)
    Wh, Ww = x.shape[2], x.shape[3]
    x = _ln(x.flatten(2).transpose(1, 2), sd, 'patch_embed.norm')
    outs = []
    for i, depth in enumerate(depths):
        H, W = Wh, Ww
        x_out, x, Wh, Ww = layer(sd, f'layers.{i}.', x, H, W, depth, num_heads[i], ws, i < len(depths) - 1)
        if i in out_indices:
            C = embed_dims * 2 ** i
            outs.append(_ln(x_out, sd, f'norm{i}').view(-1, H, W, C).permute(0, 3, 1, 2).contiguous())
    return tuple(outs)


# ------------------------------------------------------------------------------------------------ cases
HD = 32
# name -> B, H, W, window, shift, heads, options
CORE_CASES = {
    'one_window': (1, 7, 7, 7, 0, 1, {}),
    'nine_regions': (2, 14, 14, 7, 3, 2, {}),
    'pad_both': (1, 10, 17, 7, 0, 3, {}),
    'pad_both_shift': (1, 10, 17, 7, 3, 3, {}),
    'small_map': (1, 5, 5, 7, 3, 1, {}),
    'window4': (1, 8, 12, 4, 2, 2, {}),
    'window8_full_wave': (1, 16, 8, 8, 4, 2, {}),
    'window2': (1, 5, 6, 2, 1, 2, {}),
    'heads6': (1, 7, 7, 7, 0, 6, {}),
    'heads33': (1, 7, 7, 7, 3, 33, {}),
    'heads5_partial_group': (1, 7, 7, 7, 3, 5, {}),           # no divisor in 2..4: the last workgroup has one live wave of four
    'heads7_partial_group': (1, 8, 12, 4, 2, 7, {}),
    'no_bias_padded': (1, 10, 17, 7, 3, 2, dict(bias=False)),
    'scores80': (1, 10, 17, 7, 3, 2, dict(gain=9.0)),
    'max_tokens': (2, 14, 21, 7, 3, 1, {}),
}
# selector cases: q = 0, the table -400 but at the chosen offsets of the KEY from the query, (y_j - y_i, x_j - x_i)
SELECTOR_CASES = {
    'sel_nine_regions': (2, 14, 14, 7, 3, 2, {(0, 1): 0.0}),
    'sel_pad_shift': (1, 10, 17, 7, 3, 3, {(0, -1): 0.0}),      # the LEFT neighbour: the roll puts the pad columns left of tokens 0..2
    'sel_pad_noshift': (1, 10, 17, 7, 0, 1, {(0, 1): 0.0}),
    'sel_small_map': (1, 5, 5, 7, 3, 1, {(0, 1): 0.0}),
    'sel_window4': (1, 8, 12, 4, 2, 2, {(0, 1): 0.0}),
    'sel_two_offsets': (2, 14, 14, 7, 3, 2, {(0, 1): 0.0, (1, 0): -50.0}),
    'sel_two_offsets_w2': (1, 4, 6, 2, 1, 2, {(0, 1): 0.0, (1, 0): -50.0}),      # window 2: half of the queries have one of the two keys only
}
DECIDED_LEAD = 150.0          # exp(-150) is 0 in fp32: the softmax of such a query is exactly one-hot


def core_case(name, seed=0):
    """-> dict(qkv fp32 [B, H, W, 3, heads, 32], qkv_bias fp32 or None, table fp32, B, H, W, heads, window, shift, scale)"""
    B, H, W, ws, shift, heads, opt = CORE_CASES[name]
    g = torch.Generator().manual_seed(1000 + seed + sum(map(ord, name)))
    gain = opt.get('gain', 1.0)
    qkv = torch.randn((B, H, W, 3, heads, HD), generator=g)
    qkv[:, :, :, :2] *= gain               # q, k of magnitude `gain`: scores of magnitude gain^2 (32 products of variance gain^4, times 32^-0.5)
    bias = torch.randn((3 * heads * HD,), generator=g) * gain if opt.get('bias', True) else None
    table = torch.randn(((2 * ws - 1) ** 2, heads), generator=g)
    return dict(qkv=qkv, qkv_bias=bias, table=table, B=B, H=H, W=W, heads=heads, window=ws, shift=shift, scale=HD ** -0.5)


def selector_case(name, seed=0):
    B, H, W, ws, shift, heads, offsets = SELECTOR_CASES[name]
    g = torch.Generator().manual_seed(2000 + seed + sum(map(ord, name)))
    qkv = torch.randn((B, H, W, 3, heads, HD), generator=g)
    qkv[:, :, :, 0] = 0
    bias = torch.randn((3 * heads * HD,), generator=g)
    bias[:heads * HD] = 0                                                       # a pad token's q: it is never a query, zero all the same
    table = torch.full(((2 * ws - 1) ** 2, heads), -400.0)
    for (dy, dx), value in offsets.items():
        table[(-dy + ws - 1) * (2 * ws - 1) - dx + ws - 1] = value
    return dict(qkv=qkv, qkv_bias=bias, table=table, B=B, H=H, W=W, heads=heads, window=ws, shift=shift, scale=HD ** -0.5)


def run_core(case, dtype=torch.float64, device='cpu', details=False):
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)      # noqa: E731
    return core(to(case['qkv']), to(case['qkv_bias']), to(case['table']), case['heads'], case['window'], case['shift'], case['scale'], details)


def random_state(module, seed, spread=0.5):
    """a state dict with every parameter random (LayerNorm weights around 1), in place of the near-zero initialisation: fp32 tensors"""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, v in module.state_dict().items():
        if not v.dtype.is_floating_point:
            sd[k] = v.clone()
        elif k.endswith('.weight') and v.dim() == 1:
            sd[k] = 1 + 0.2 * torch.randn(v.shape, generator=g)
        elif v.dim() >= 2 and 'table' not in k:
            sd[k] = torch.randn(v.shape, generator=g) * (spread / math.sqrt(v[0].numel()) * 2)
        else:
            sd[k] = torch.randn(v.shape, generator=g) * spread
    return sd


def bound(err, ref_err, magnitude):
    """the project's accuracy rule: err <= max(8 x the fp32 torch composition's own error, 4 fp32 ulps of the largest magnitude);
    -> (limit, err / limit)"""
    ulp = 2.0 ** (math.floor(math.log2(magnitude)) - 23) if magnitude > 0 else 0.0
    limit = max(8.0 * ref_err, 4.0 * ulp)
    return limit, err / limit
