"""`SwinTransformerDIY`, the backbone of the reference's Swin-B / Swin-L configs (swin/swin_transformer.py), with the window attention of
every block as ONE HIP kernel (include/vkn_swin.h).

Constructor keywords, defaults, state-dict keys (the persistent buffer `attn.relative_position_index` included), `_freeze_stages`,
`train()`, `init_weights(None)` and the output tuple are the reference's.  What differs is inside `SwinTransformerBlock.forward`: under
the conditions of `fused_path` the pad, the two rolls, the window partition and its reverse, the `qkv` permute, the bias gather, the mask
add, the softmax and the crop are `ops.swin_window_attention` on the rows of `attn.qkv(norm1(x))` as they lie.  Everywhere else
`forward_torch` runs, the reference's composition op for op: it is what trains by default and what runs on the CPU.  With `fused='train'`
a block that needs a gradient keeps the kernel and differentiates it through `autograd.swin_window_attention`, whose backward is a second
HIP kernel (include/vkn_wattn_train.h) that recomputes the softmax instead of saving it.

The Linears, LayerNorms, the GELU MLP, `PatchEmbed` and `PatchMerging` are torch modules.  `timm` is not needed: `DropPath`, `to_2tuple`
and `trunc_normal_` are the few lines below.  Loading a published Swin checkpoint `strict=True` is the decisive check of the key names.
"""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F
import torch.utils.checkpoint as checkpoint

from . import autograd, ops
from .registry import register_backbone

trunc_normal_ = nn.init.trunc_normal_
# Whether a block takes the HIP kernel by default where it may.  The rule: on, if the table of tools/swin_ab.py shows the fused span faster
# than the torch span at every shipped stage shape by more than the tool's spread; otherwise off.  profiles/swin_ab.txt: faster at all 64
# shapes, torch / fused between 1.42 and 3.30 with spreads of at most 11 % on the fused arm.
FUSED_DEFAULT = True


def to_2tuple(v):
    return tuple(v) if isinstance(v, (tuple, list)) else (v, v)


class DropPath(nn.Module):
    """Stochastic depth: a whole sample's residual branch is dropped with probability `drop_prob`, the rest scaled by 1 / keep."""

    def __init__(self, drop_prob=0.):
        super().__init__()
        self.drop_prob = drop_prob

    def forward(self, x):
        if self.drop_prob == 0. or not self.training:
            return x
        keep = 1 - self.drop_prob
        mask = x.new_empty((x.shape[0],) + (1,) * (x.dim() - 1)).bernoulli_(keep)
        return x * mask.div_(keep)


class Mlp(nn.Module):
    def __init__(self, in_features, hidden_features=None, out_features=None, act_layer=nn.GELU, drop=0.):
        super().__init__()
        self.fc1 = nn.Linear(in_features, hidden_features or in_features)
        self.act = act_layer()
        self.fc2 = nn.Linear(hidden_features or in_features, out_features or in_features)
        self.drop = nn.Dropout(drop)

    def forward(self, x):
        return self.drop(self.fc2(self.drop(self.act(self.fc1(x)))))


def window_partition(x, window_size):
    """[B, H, W, C] -> [B nW, window_size, window_size, C]"""
    B, H, W, C = x.shape
    x = x.view(B, H // window_size, window_size, W // window_size, window_size, C)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(-1, window_size, window_size, C)


def window_reverse(windows, window_size, H, W):
    """[B nW, window_size, window_size, C] -> [B, H, W, C]"""
    B = windows.shape[0] // ((H // window_size) * (W // window_size))
    x = windows.view(B, H // window_size, W // window_size, window_size, window_size, -1)
    return x.permute(0, 1, 3, 2, 4, 5).contiguous().view(B, H, W, -1)


def relative_position_index(window_size):
    """[Wh Ww, Wh Ww] int64: the row of the bias table for (query i, key j)"""
    wh, ww = window_size
    yx = torch.stack(torch.meshgrid(torch.arange(wh), torch.arange(ww), indexing='ij')).flatten(1)        # [2, Wh Ww]
    d = (yx[:, :, None] - yx[:, None, :]).permute(1, 2, 0)
    return (d[..., 0] + wh - 1) * (2 * ww - 1) + d[..., 1] + ww - 1


class WindowAttention(nn.Module):
    """W-MSA / SW-MSA on windows that the caller has cut: x [B nW, Wh Ww, C], mask [nW, Wh Ww, Wh Ww] or None"""

    def __init__(self, dim, window_size, num_heads, qkv_bias=True, qk_scale=None, attn_drop=0., proj_drop=0.):
        super().__init__()
        self.dim, self.window_size, self.num_heads = dim, window_size, num_heads
        self.scale = qk_scale or (dim // num_heads) ** -0.5
        self.relative_position_bias_table = nn.Parameter(torch.zeros((2 * window_size[0] - 1) * (2 * window_size[1] - 1), num_heads))
        self.register_buffer('relative_position_index', relative_position_index(window_size))
        self.qkv = nn.Linear(dim, dim * 3, bias=qkv_bias)
        self.attn_drop = nn.Dropout(attn_drop)
        self.proj = nn.Linear(dim, dim)
        self.proj_drop = nn.Dropout(proj_drop)
        trunc_normal_(self.relative_position_bias_table, std=.02)
        self.softmax = nn.Softmax(dim=-1)

    def forward(self, x, mask=None):
        B_, N, C = x.shape
        q, k, v = self.qkv(x).reshape(B_, N, 3, self.num_heads, C // self.num_heads).permute(2, 0, 3, 1, 4).unbind(0)
        attn = (q * self.scale) @ k.transpose(-2, -1)
        bias = self.relative_position_bias_table[self.relative_position_index.view(-1)].view(N, N, -1)
        attn = attn + bias.permute(2, 0, 1).contiguous().unsqueeze(0)
        if mask is not None:
            nW = mask.shape[0]
            attn = (attn.view(B_ // nW, nW, self.num_heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, self.num_heads, N, N)
        attn = self.attn_drop(self.softmax(attn))
        return self.proj_drop(self.proj((attn @ v).transpose(1, 2).reshape(B_, N, C)))


class SwinTransformerBlock(nn.Module):
    def __init__(self, dim, num_heads, window_size=7, shift_size=0, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., act_layer=nn.GELU, norm_layer=nn.LayerNorm, fused=None):
        super().__init__()
        self.dim, self.num_heads, self.window_size, self.shift_size, self.mlp_ratio = dim, num_heads, window_size, shift_size, mlp_ratio
        assert 0 <= self.shift_size < self.window_size, 'shift_size must in 0-window_size'
        # fused: None = FUSED_DEFAULT, True / False, or 'train' = True and, where a gradient is needed, the kernel with its HIP backward
        self.fused_backward = isinstance(fused, str) and fused == 'train'
        if isinstance(fused, str) and not self.fused_backward:
            raise ValueError(f"fused must be None, True, False or 'train', not {fused!r}")
        self.fused = FUSED_DEFAULT if fused is None else bool(fused)
        self.norm1 = norm_layer(dim)
        self.attn = WindowAttention(dim, window_size=to_2tuple(window_size), num_heads=num_heads, qkv_bias=qkv_bias, qk_scale=qk_scale,
                                    attn_drop=attn_drop, proj_drop=drop)
        self.drop_path = DropPath(drop_path) if drop_path > 0. else nn.Identity()
        self.norm2 = norm_layer(dim)
        self.mlp = Mlp(in_features=dim, hidden_features=int(dim * mlp_ratio), act_layer=act_layer, drop=drop)
        self.H = self.W = None
        self.last_path = None                      # 'fused', 'fused_train' or 'torch': what the last forward took

    def needs_grad(self, x):
        return torch.is_grad_enabled() and (x.requires_grad or any(p.requires_grad for p in self.attn.parameters()) or self.norm1.weight.requires_grad)

    def fused_path(self, x, train=False):
        """Whether this call may run the HIP kernel: the flag, CUDA fp32, nothing to differentiate, no attention dropout at work, and
        the shape inside the envelope of include/vkn_swin.h.  `train`: the same question with a gradient allowed."""
        if not (self.fused and x.is_cuda and x.dtype == torch.float32) or torch.is_autocast_enabled():      # (autocast: the Linears hand out fp16)
            return False
        if not train and self.needs_grad(x):
            return False
        if self.training and self.attn.attn_drop.p > 0:
            return False
        if self.dim % self.num_heads or any(p.dtype != torch.float32 for p in self.attn.parameters()):
            return False
        return ops.swin_window_attention_supported(x.shape[0], self.H, self.W, self.num_heads, self.window_size, self.shift_size,
                                                   head_dim=self.dim // self.num_heads)

    def fused_train_path(self, x):
        """Whether this call runs the kernel WITH its HIP backward: `fused='train'`, a gradient is needed (that alone turned `fused_path`
        down), and the backward's envelope (include/vkn_wattn_train.h) holds the shape."""
        if not (self.fused_backward and self.needs_grad(x) and self.fused_path(x, train=True)):
            return False
        return ops.swin_window_attention_bwd_supported(x.shape[0], self.H, self.W, self.num_heads, self.window_size, self.shift_size,
                                                       head_dim=self.dim // self.num_heads)

    def attention_fused(self, x, train=False):
        """norm1's output [B, H W, C] -> the attention branch before the residual: qkv Linear, the kernel, proj.  `train`: the kernel
        as an autograd function; the Linears stay torch autograd."""
        a = self.attn
        core = autograd.swin_window_attention if train else ops.swin_window_attention
        y = core(a.qkv(x), a.qkv.bias, a.relative_position_bias_table, self.H, self.W, self.num_heads, self.window_size, self.shift_size, a.scale)
        return a.proj_drop(a.proj(y))

    def attention_torch(self, x, mask_matrix):
        """The same span as the reference composes it: pad, roll, partition, attend, reverse, roll back, crop"""
        B, L, C = x.shape
        H, W, ws, shift = self.H, self.W, self.window_size, self.shift_size
        x = x.view(B, H, W, C)
        pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
        x = F.pad(x, (0, 0, 0, pad_r, 0, pad_b))
        _, Hp, Wp, _ = x.shape
        if shift > 0:
            x = torch.roll(x, shifts=(-shift, -shift), dims=(1, 2))
            if mask_matrix is None:                # a shifted block is never attended without its mask: painted here when none was handed in
                mask_matrix = shift_attention_mask(H, W, ws, shift, x.device, x.dtype)
        windows = window_partition(x, ws).view(-1, ws * ws, C)
        windows = self.attn(windows, mask=mask_matrix if shift > 0 else None)
        x = window_reverse(windows.view(-1, ws, ws, C), ws, Hp, Wp)
        if shift > 0:
            x = torch.roll(x, shifts=(shift, shift), dims=(1, 2))
        if pad_r > 0 or pad_b > 0:
            x = x[:, :H, :W, :].contiguous()
        return x.view(B, H * W, C)

    def forward_torch(self, x, mask_matrix):
        assert x.shape[1] == self.H * self.W, 'input feature has wrong size'
        self.last_path = 'torch'
        x = x + self.drop_path(self.attention_torch(self.norm1(x), mask_matrix))
        return x + self.drop_path(self.mlp(self.norm2(x)))

    def forward(self, x, mask_matrix):
        train = False
        if not self.fused_path(x):
            train = self.fused_train_path(x)
            if not train:
                return self.forward_torch(x, mask_matrix)
        assert x.shape[1] == self.H * self.W, 'input feature has wrong size'
        self.last_path = 'fused_train' if train else 'fused'
        x = x + self.drop_path(self.attention_fused(self.norm1(x), train))
        return x + self.drop_path(self.mlp(self.norm2(x)))


class PatchMerging(nn.Module):
    def __init__(self, dim, norm_layer=nn.LayerNorm):
        super().__init__()
        self.dim = dim
        self.reduction = nn.Linear(4 * dim, 2 * dim, bias=False)
        self.norm = norm_layer(4 * dim)

    def forward(self, x, H, W):
        B, L, C = x.shape
        assert L == H * W, 'input feature has wrong size'
        x = x.view(B, H, W, C)
        if H % 2 or W % 2:
            x = F.pad(x, (0, 0, 0, W % 2, 0, H % 2))
        x = torch.cat([x[:, 0::2, 0::2], x[:, 1::2, 0::2], x[:, 0::2, 1::2], x[:, 1::2, 1::2]], -1).view(B, -1, 4 * C)
        return self.reduction(self.norm(x))


def shift_attention_mask(H, W, window_size, shift_size, device=None, dtype=torch.float32):
    """[nW, ws ws, ws ws] of 0 / -100 for the padded H x W map, painted as `BasicLayer.forward` paints it"""
    Hp, Wp = int(np.ceil(H / window_size)) * window_size, int(np.ceil(W / window_size)) * window_size
    img_mask = torch.zeros((1, Hp, Wp, 1), device=device)
    slices = (slice(0, -window_size), slice(-window_size, -shift_size), slice(-shift_size, None))
    cnt = 0
    for h in slices:
        for w in slices:
            img_mask[:, h, w, :] = cnt
            cnt += 1
    mw = window_partition(img_mask, window_size).view(-1, window_size * window_size)
    diff = mw.unsqueeze(1) - mw.unsqueeze(2)
    return diff.masked_fill(diff != 0, float(-100.0)).masked_fill(diff == 0, float(0.0)).to(dtype=dtype)


class BasicLayer(nn.Module):
    def __init__(self, dim, depth, num_heads, window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0., attn_drop=0.,
                 drop_path=0., norm_layer=nn.LayerNorm, downsample=None, with_cp=False, fused=None):
        super().__init__()
        self.window_size, self.shift_size, self.depth, self.with_cp = window_size, window_size // 2, depth, with_cp
        self.blocks = nn.ModuleList([
            SwinTransformerBlock(dim=dim, num_heads=num_heads, window_size=window_size, shift_size=0 if i % 2 == 0 else window_size // 2,
                                 mlp_ratio=mlp_ratio, qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop, attn_drop=attn_drop,
                                 drop_path=drop_path[i] if isinstance(drop_path, list) else drop_path, norm_layer=norm_layer, fused=fused)
            for i in range(depth)])
        self.downsample = downsample(dim=dim, norm_layer=norm_layer) if downsample is not None else None

    def forward(self, x, H, W):
        for blk in self.blocks:
            blk.H, blk.W = H, W
        # the painted mask is only what `forward_torch` reads (the kernel computes the regions): it is painted once, for the first shifted
        # block that takes the composition on the `x` that reaches IT — a block's output may need a gradient where the layer's input did not
        attn_mask = None
        for blk in self.blocks:
            if attn_mask is None and blk.shift_size > 0 and not blk.fused_path(x) and not blk.fused_train_path(x):
                attn_mask = shift_attention_mask(H, W, self.window_size, self.shift_size, x.device, x.dtype)
            x = checkpoint.checkpoint(blk, x, attn_mask, use_reentrant=False) if self.with_cp else blk(x, attn_mask)
        if self.downsample is not None:
            return x, H, W, self.downsample(x, H, W), (H + 1) // 2, (W + 1) // 2
        return x, H, W, x, H, W


class PatchEmbed(nn.Module):
    def __init__(self, patch_size=4, in_chans=3, embed_dims=96, norm_layer=None):
        super().__init__()
        self.patch_size, self.in_chans, self.embed_dims = to_2tuple(patch_size), in_chans, embed_dims
        self.proj = nn.Conv2d(in_chans, embed_dims, kernel_size=self.patch_size, stride=self.patch_size)
        self.norm = norm_layer(embed_dims) if norm_layer is not None else None

    def forward(self, x):
        _, _, H, W = x.size()
        ph, pw = self.patch_size
        if W % pw:
            x = F.pad(x, (0, pw - W % pw))
        if H % ph:
            x = F.pad(x, (0, 0, 0, ph - H % ph))
        x = self.proj(x)
        if self.norm is not None:
            Wh, Ww = x.size(2), x.size(3)
            x = self.norm(x.flatten(2).transpose(1, 2)).transpose(1, 2).view(-1, self.embed_dims, Wh, Ww)
        return x


@register_backbone
class SwinTransformerDIY(nn.Module):
    """The reference's keywords and defaults; `fused` (None = `FUSED_DEFAULT`, True, False, or 'train': the kernel also where a gradient
    is needed, with its HIP backward) is this package's one addition."""

    def __init__(self, pretrain_img_size=224, patch_size=4, in_chans=3, embed_dims=96, depths=[2, 2, 6, 2], num_heads=[3, 6, 12, 24],
                 window_size=7, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop_rate=0., attn_drop_rate=0., drop_path_rate=0.2,
                 norm_layer=nn.LayerNorm, use_abs_pos_embed=False, patch_norm=True, out_indices=(0, 1, 2, 3), frozen_stages=-1,
                 with_cp=False, output_img=False, pretrained=None, fused=None):
        super().__init__()
        self.output_img, self.pretrain_img_size, self.num_layers, self.embed_dims = output_img, pretrain_img_size, len(depths), embed_dims
        self.ape, self.patch_norm, self.out_indices, self.frozen_stages, self.pretrained = use_abs_pos_embed, patch_norm, out_indices, frozen_stages, pretrained
        self.window_size = window_size
        self.patch_embed = PatchEmbed(patch_size=patch_size, in_chans=in_chans, embed_dims=embed_dims, norm_layer=norm_layer if patch_norm else None)
        if self.ape:
            size, patch = to_2tuple(pretrain_img_size), to_2tuple(patch_size)
            self.absolute_pos_embed = nn.Parameter(torch.zeros(1, embed_dims, size[0] // patch[0], size[1] // patch[1]))
            trunc_normal_(self.absolute_pos_embed, std=.02)
        self.pos_drop = nn.Dropout(p=drop_rate)
        dpr = [v.item() for v in torch.linspace(0, drop_path_rate, sum(depths))]           # the stochastic-depth decay rule
        self.layers = nn.ModuleList([
            BasicLayer(dim=int(embed_dims * 2 ** i), depth=depths[i], num_heads=num_heads[i], window_size=window_size, mlp_ratio=mlp_ratio,
                       qkv_bias=qkv_bias, qk_scale=qk_scale, drop=drop_rate, attn_drop=attn_drop_rate,
                       drop_path=dpr[sum(depths[:i]):sum(depths[:i + 1])], norm_layer=norm_layer,
                       downsample=PatchMerging if i < self.num_layers - 1 else None, with_cp=with_cp, fused=fused)
            for i in range(self.num_layers)])
        self.num_features = [int(embed_dims * 2 ** i) for i in range(self.num_layers)]
        for i in out_indices:
            self.add_module(f'norm{i}', norm_layer(self.num_features[i]))
        self._freeze_stages()

    def _freeze_stages(self):
        if self.frozen_stages >= 0:
            self.patch_embed.eval()
            for p in self.patch_embed.parameters():
                p.requires_grad = False
        if self.frozen_stages >= 1 and self.ape:
            self.absolute_pos_embed.requires_grad = False
        if self.frozen_stages >= 2:
            self.pos_drop.eval()
            for i in range(0, self.frozen_stages - 1):
                self.layers[i].eval()
                for p in self.layers[i].parameters():
                    p.requires_grad = False

    def init_weights(self, pretrained=None):
        if pretrained is None and self.pretrained is not None:
            pretrained = self.pretrained
        if pretrained is not None and not isinstance(pretrained, str):
            raise TypeError('pretrained must be a str or None')

        def _init(m):
            if isinstance(m, nn.Linear):
                trunc_normal_(m.weight, std=.02)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)
            elif isinstance(m, nn.LayerNorm):
                nn.init.constant_(m.bias, 0)
                nn.init.constant_(m.weight, 1.0)
        self.apply(_init)
        if isinstance(pretrained, str):
            self.load_pretrained(pretrained)

    def load_pretrained(self, path):
        """A plain `torch.load` state dict (or one under 'state_dict' / 'model'), loaded non-strictly.  A bias table of another window
        size is NOT interpolated as the reference's loader does: that raises."""
        sd = torch.load(path, map_location='cpu')
        for key in ('state_dict', 'model'):
            if isinstance(sd, dict) and isinstance(sd.get(key), dict):
                sd = sd[key]
        sd = {(k[len('backbone.'):] if k.startswith('backbone.') else k): v for k, v in sd.items()}
        own = self.state_dict()
        for k, v in sd.items():
            if k.endswith('relative_position_bias_table') and k in own and tuple(v.shape) != tuple(own[k].shape):
                raise NotImplementedError(f'{k}: checkpoint table {tuple(v.shape)} for another window size than {self.window_size} '
                                          f'({tuple(own[k].shape)}); interpolating bias tables on load is not built')
        return self.load_state_dict(sd, strict=False)

    def forward(self, x):
        image = x
        x = self.patch_embed(x)
        Wh, Ww = x.size(2), x.size(3)
        if self.ape:
            x = x + F.interpolate(self.absolute_pos_embed, size=(Wh, Ww), mode='bicubic')
        x = self.pos_drop(x.flatten(2).transpose(1, 2))
        outs = []
        for i, layer in enumerate(self.layers):
            x_out, H, W, x, Wh, Ww = layer(x, Wh, Ww)
            if i in self.out_indices:
                x_out = getattr(self, f'norm{i}')(x_out)
                outs.append(x_out.view(-1, H, W, self.num_features[i]).permute(0, 3, 1, 2).contiguous())
        if self.output_img:
            outs.insert(0, image)
        return tuple(outs)

    def train(self, mode=True):
        super().train(mode)
        self._freeze_stages()
        return self
