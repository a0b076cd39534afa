"""`MSDeformAttnPixelDecoder` — drop-in for the reference's deformable-attention neck (knet/det/msdeformattn_decoder.py:18-275): same
ctor kwargs and defaults, module tree, state-dict keys (mmcv 1.x / mmdet 2.18 names: `ConvModule` -> `conv` / `gn`,
`DetrTransformerEncoder` -> `layers`, `BaseTransformerLayer` -> `attentions` / `ffns` / `norms`, `FFN` -> `layers.0.0` / `layers.1`)
and return value.  The four shipped `*deformable*` configs give it one dict: six post-norm layers of
MultiScaleDeformableAttention(256, 8 heads, 3 levels, 4 points) -> LN -> FFN(256 -> 1024 ReLU -> 256) -> LN, no dropout.

Two forward paths, in the manner of `SemanticFPNWrapper`:
  * `forward_torch`: the torch composition of the module's own layers, the sampling core on `F.grid_sample`.  Differentiable; taken
    whenever a gradient is needed, on CPU tensors, in another dtype than fp32 or outside the kernel's envelope.
  * `forward_fused`: the encoder batch-first on [B Q][C] rows through this library: per layer one `vkn_linear_f32` for offsets and
    logits together, one for `value_proj`, the sampling core `vkn_msda_sample_f32` (include/vkn_msda.h), `output_proj`,
    `vkn_layernorm_act_fwd_f32` with the residual, the FFN as two linears, the second LayerNorm.  The 1x1 `input_convs` (Cin up to
    2048), the lateral / output convs and `mask_feature` stay torch ops.
With `fused_backward=True` (an extra keyword, off by default) the sampling core inside `forward_torch` is `autograd.msda_sample` when
a gradient is needed: forward `vkn_msda_sample_f32`, backward `vkn_msda_sample_bwd_f32` (include/vkn_msda_train.h), deterministic
and free of float atomics; the Linears, LayerNorms, convs and transposes around it stay torch autograd.
Whatever no shipped config uses raises NotImplementedError at construction.
"""
import math

import torch
import torch.nn as nn
import torch.nn.functional as F

from . import autograd, ops
from .registry import NECKS
from .semantic_fpn import SinePositionalEncoding


def _unsupported(what):
    raise NotImplementedError(f'MSDeformAttnPixelDecoder {what} is not built (no shipped config uses it)')


def _get(cfg, key, default=None):
    return cfg.get(key, default) if isinstance(cfg, dict) else getattr(cfg, key, default)


class _ConvModule(nn.Module):
    """mmcv `ConvModule(cin, cout, k, padding, bias, norm_cfg=GN, act_cfg)`: conv -> GN (-> ReLU), mmcv's attribute names"""

    def __init__(self, cin, cout, k, padding, bias, num_groups, relu):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=1, padding=padding, bias=bias)
        self.gn = nn.GroupNorm(num_groups, cout)
        self.with_activation = bool(relu)
        if relu:
            self.activate = nn.ReLU()

    def forward(self, x):
        x = self.gn(self.conv(x))
        return self.activate(x) if self.with_activation else x


def msda_core_torch(value, spatial_shapes, sampling_locations, attention_weights):
    """mmcv's `multi_scale_deformable_attn_pytorch`: value [B, S, M, D], sampling_locations [B, Q, M, L, P, 2] normalised,
    attention_weights [B, Q, M, L, P] -> [B, Q, M D]."""
    B, _, M, D = value.shape
    _, Q, _, L, P, _ = sampling_locations.shape
    value_list = value.split([int(h) * int(w) for h, w in spatial_shapes], dim=1)
    grids = 2 * sampling_locations - 1
    sampled = []
    for lvl, (h, w) in enumerate(spatial_shapes):
        value_l = value_list[lvl].flatten(2).transpose(1, 2).reshape(B * M, D, int(h), int(w))
        grid_l = grids[:, :, :, lvl].transpose(1, 2).flatten(0, 1)                                   # [B M, Q, P, 2]
        sampled.append(F.grid_sample(value_l, grid_l, mode='bilinear', padding_mode='zeros', align_corners=False))
    weights = attention_weights.transpose(1, 2).reshape(B * M, 1, Q, L * P)
    out = (torch.stack(sampled, dim=-2).flatten(-2) * weights).sum(-1).view(B, M * D, Q)
    return out.transpose(1, 2).contiguous()


class MultiScaleDeformableAttention(nn.Module):
    """mmcv 1.x `MultiScaleDeformableAttention` (mmcv/ops/multi_scale_deform_attn.py) for the decoder's call: seq-first, all-valid
    padding mask, 2-d reference points.  `forward` is the torch composition; the decoder's fused path reads the parameters.
    `fused_backward` (an attribute the decoder sets, no ctor argument): when a gradient is needed on CUDA fp32 tensors inside the
    core's envelope, the sampling core runs as `autograd.msda_sample` on the raw offsets and logits."""

    def __init__(self, embed_dims=256, num_heads=8, num_levels=4, num_points=4, im2col_step=64, dropout=0.1, batch_first=False,
                 norm_cfg=None, init_cfg=None):
        super().__init__()
        if embed_dims % num_heads != 0:
            raise ValueError(f'embed_dims must be divisible by num_heads, but got {embed_dims} and {num_heads}')
        if dropout:
            _unsupported(f'attention dropout={dropout!r}')
        if batch_first:
            _unsupported('batch_first=True')
        if norm_cfg is not None:
            _unsupported(f'attention norm_cfg={norm_cfg!r}')
        self.embed_dims, self.num_heads, self.num_levels, self.num_points = embed_dims, num_heads, num_levels, num_points
        self.im2col_step, self.batch_first = im2col_step, batch_first
        self.fused_backward = False
        self.sampling_offsets = nn.Linear(embed_dims, num_heads * num_levels * num_points * 2)
        self.attention_weights = nn.Linear(embed_dims, num_heads * num_levels * num_points)
        self.value_proj = nn.Linear(embed_dims, embed_dims)
        self.output_proj = nn.Linear(embed_dims, embed_dims)
        self.init_weights()

    def init_weights(self):
        """offsets: weight 0, bias the per-head direction grid scaled by the point index; attention weights 0; xavier on the projections"""
        nn.init.constant_(self.sampling_offsets.weight, 0.)
        thetas = torch.arange(self.num_heads, dtype=torch.float32) * (2.0 * math.pi / self.num_heads)
        grid = torch.stack([thetas.cos(), thetas.sin()], -1)
        grid = (grid / grid.abs().max(-1, keepdim=True)[0]).view(self.num_heads, 1, 1, 2).repeat(1, self.num_levels, self.num_points, 1)
        for i in range(self.num_points):
            grid[:, :, i, :] *= i + 1
        with torch.no_grad():
            self.sampling_offsets.bias.copy_(grid.view(-1))
        nn.init.constant_(self.attention_weights.weight, 0.)
        nn.init.constant_(self.attention_weights.bias, 0.)
        for proj in (self.value_proj, self.output_proj):
            nn.init.xavier_uniform_(proj.weight)
            nn.init.constant_(proj.bias, 0.)

    def forward(self, query, query_pos, reference_points, spatial_shapes):
        """query, query_pos [Q, B, C]; reference_points [Q, L, 2] (shared by the batch); spatial_shapes [(H_l, W_l)] -> [Q, B, C]"""
        identity = query
        value = query
        query = query + query_pos
        Q, B, C = query.shape
        M, L, P = self.num_heads, self.num_levels, self.num_points
        value = self.value_proj(value.permute(1, 0, 2)).view(B, Q, M, C // M)
        query = query.permute(1, 0, 2)
        raw_offsets, raw_logits = self.sampling_offsets(query), self.attention_weights(query)
        if self._fused_backward_ok(value, raw_offsets, raw_logits, reference_points, spatial_shapes):
            core = autograd.msda_sample(value.reshape(B, Q, C), spatial_shapes, raw_offsets.reshape(B * Q, -1), raw_logits.reshape(B * Q, -1),
                                        reference_points.contiguous(), M, P)
            return self.output_proj(core).permute(1, 0, 2) + identity
        offsets = raw_offsets.view(B, Q, M, L, P, 2)
        weights = raw_logits.view(B, Q, M, L * P).softmax(-1).view(B, Q, M, L, P)
        normalizer = query.new_tensor([[int(w), int(h)] for h, w in spatial_shapes])
        locations = reference_points[None, :, None, :, None, :] + offsets / normalizer[None, None, None, :, None, :]
        out = self.output_proj(msda_core_torch(value, spatial_shapes, locations, weights)).permute(1, 0, 2)
        return out + identity


    def _fused_backward_ok(self, value, raw_offsets, raw_logits, reference_points, spatial_shapes):
        """the flag, a gradient to compute, CUDA fp32 operands, the envelope of the core and of its backward"""
        ts = (value, raw_offsets, raw_logits)
        if not (self.fused_backward and torch.is_grad_enabled() and any(t.requires_grad for t in ts)):
            return False
        if not all(t.is_cuda and t.dtype == torch.float32 for t in ts + (reference_points,)):
            return False
        B, Q, M, D = value.shape
        L, P = self.num_levels, self.num_points
        if len(spatial_shapes) != L or tuple(reference_points.shape) != (Q, L, 2) or not ops.msda_fits(M, D, L, P):
            return False
        return ops.msda_bwd_workspace_bytes(spatial_shapes, B, Q, M, D, P) > 0


class _FFN(nn.Module):
    """mmcv 1.x `FFN(num_fcs=2, ReLU, no dropout, add_identity)`: layers = Sequential(Sequential(Linear, ReLU, Dropout), Linear, Dropout)"""

    def __init__(self, embed_dims, feedforward_channels):
        super().__init__()
        self.embed_dims, self.feedforward_channels = embed_dims, feedforward_channels
        self.layers = nn.Sequential(nn.Sequential(nn.Linear(embed_dims, feedforward_channels), nn.ReLU(inplace=True), nn.Dropout(0.)),
                                    nn.Linear(feedforward_channels, embed_dims), nn.Dropout(0.))

    def forward(self, x):
        return x + self.layers(x)


_FFN_DEFAULTS = dict(type='FFN', embed_dims=256, feedforward_channels=1024, num_fcs=2, ffn_drop=0., act_cfg=dict(type='ReLU', inplace=True))


class _EncoderLayer(nn.Module):
    """mmcv 1.x `BaseTransformerLayer(operation_order=('self_attn', 'norm', 'ffn', 'norm'))` with one attention and one FFN"""

    def __init__(self, attn_cfgs=None, ffn_cfgs=None, operation_order=None, norm_cfg=dict(type='LN'), init_cfg=None, batch_first=False,
                 **deprecated):
        super().__init__()
        if isinstance(ffn_cfgs, (list, tuple)):
            _unsupported('a list of ffn_cfgs')
        ffn = dict(_FFN_DEFAULTS if ffn_cfgs is None else ffn_cfgs)
        for old, new in (('feedforward_channels', 'feedforward_channels'), ('ffn_dropout', 'ffn_drop'), ('ffn_num_fcs', 'num_fcs')):
            if old in deprecated:                                  # the deprecated layer-level arguments of mmcv 1.x
                ffn[new] = deprecated.pop(old)
        if deprecated:
            _unsupported(f'transformer layer arguments {sorted(deprecated)}')
        if operation_order is None or tuple(operation_order) != ('self_attn', 'norm', 'ffn', 'norm'):
            _unsupported(f'operation_order={operation_order!r}')
        if batch_first:
            _unsupported('batch_first=True')
        if norm_cfg is None or _get(norm_cfg, 'type') != 'LN':
            _unsupported(f'transformer norm_cfg={norm_cfg!r} (LN only)')
        if isinstance(attn_cfgs, (list, tuple)):
            if len(attn_cfgs) != 1:
                _unsupported(f'{len(attn_cfgs)} attentions per layer')
            attn_cfgs = attn_cfgs[0]
        attn = dict(attn_cfgs or {})
        if attn.pop('type', None) != 'MultiScaleDeformableAttention':
            _unsupported(f'attention type {_get(attn_cfgs, "type")!r}')
        if ffn.get('type', 'FFN') != 'FFN' or ffn.get('num_fcs', 2) != 2 or _get(ffn.get('act_cfg', dict(type='ReLU')), 'type') != 'ReLU':
            _unsupported(f'ffn_cfgs={ffn!r} (FFN with ReLU and num_fcs=2 only)')
        if ffn.get('ffn_drop', 0.) or ffn.get('dropout', 0.) or ffn.get('dropout_layer') is not None:
            _unsupported('FFN dropout > 0')
        if not ffn.get('add_identity', True):
            _unsupported('FFN add_identity=False')
        self.batch_first, self.pre_norm = False, False
        self.operation_order = ('self_attn', 'norm', 'ffn', 'norm')
        self.attentions = nn.ModuleList([MultiScaleDeformableAttention(**attn)])
        self.embed_dims = self.attentions[0].embed_dims
        if ffn.get('embed_dims', self.embed_dims) != self.embed_dims:
            raise ValueError(f'FFN embed_dims {ffn["embed_dims"]} != attention embed_dims {self.embed_dims}')
        self.ffns = nn.ModuleList([_FFN(self.embed_dims, ffn.get('feedforward_channels', 1024))])
        self.norms = nn.ModuleList([nn.LayerNorm(self.embed_dims, eps=_get(norm_cfg, 'eps', 1e-5)) for _ in range(2)])

    def forward(self, query, query_pos, reference_points, spatial_shapes):
        query = self.norms[0](self.attentions[0](query, query_pos, reference_points, spatial_shapes))
        return self.norms[1](self.ffns[0](query))


class _Encoder(nn.Module):
    """mmdet 2.18 `DetrTransformerEncoder`: `num_layers` copies of one layer config; post-norm order, so no `post_norm` module"""

    def __init__(self, transformerlayers=None, num_layers=None, post_norm_cfg=dict(type='LN'), init_cfg=None):
        super().__init__()
        if isinstance(transformerlayers, (list, tuple)):
            _unsupported('a list of transformerlayers')
        layer = dict(transformerlayers or {})
        if layer.pop('type', None) != 'BaseTransformerLayer':
            _unsupported(f'transformer layer type {_get(transformerlayers, "type")!r}')
        if not num_layers or num_layers < 1:
            raise ValueError(f'num_layers={num_layers!r}')
        self.num_layers = int(num_layers)
        self.layers = nn.ModuleList([_EncoderLayer(**layer) for _ in range(self.num_layers)])
        self.embed_dims, self.pre_norm, self.post_norm = self.layers[0].embed_dims, False, None

    def forward(self, query, query_pos, reference_points, spatial_shapes):
        for layer in self.layers:
            query = layer(query, query_pos, reference_points, spatial_shapes)
        return query


_ENCODER_DEFAULT = dict(
    type='DetrTransformerEncoder', num_layers=6,
    transformerlayers=dict(
        type='BaseTransformerLayer',
        attn_cfgs=dict(type='MultiScaleDeformableAttention', embed_dims=256, num_heads=8, num_levels=3, num_points=4, im2col_step=64,
                       dropout=0.0, batch_first=False, norm_cfg=None, init_cfg=None),
        feedforward_channels=1024, ffn_dropout=0.0, operation_order=('self_attn', 'norm', 'ffn', 'norm')),
    init_cfg=None)


class MSDeformAttnPixelDecoder(nn.Module):
    """knet/det/msdeformattn_decoder.py:18-275.  `fused` (an extra keyword) = False keeps every call on `forward_torch`;
    `fused_backward` (another) = True gives `forward_torch` the library's sampling core with its HIP backward where a gradient is needed."""

    def __init__(self, in_channels=[256, 512, 1024, 2048], strides=[4, 8, 16, 32], feat_channels=256, out_channels=256, num_outs=3,
                 return_one_list=True, norm_cfg=dict(type='GN', num_groups=32), act_cfg=dict(type='ReLU'), encoder=_ENCODER_DEFAULT,
                 positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True), init_cfg=None, fused=True,
                 fused_backward=False):
        super().__init__()
        self.fused, self.fused_backward = bool(fused), bool(fused_backward)
        if norm_cfg is None or _get(norm_cfg, 'type') != 'GN':
            _unsupported(f'norm_cfg={norm_cfg!r} (GN only)')
        if act_cfg is None or _get(act_cfg, 'type') != 'ReLU':
            _unsupported(f'act_cfg={act_cfg!r} (ReLU only)')
        if _get(positional_encoding, 'type', 'SinePositionalEncoding') != 'SinePositionalEncoding':
            _unsupported(f'positional_encoding type {_get(positional_encoding, "type")!r}')
        enc = dict(encoder)
        if enc.pop('type', None) != 'DetrTransformerEncoder':
            _unsupported(f'encoder type {_get(encoder, "type")!r}')
        self.in_channels, self.strides = list(in_channels), list(strides)
        self.feat_channels, self.out_channels = feat_channels, out_channels
        self.num_input_levels = len(in_channels)
        self.return_one_list = return_one_list
        self.encoder = _Encoder(**enc)
        self.num_encoder_levels = self.encoder.layers[0].attentions[0].num_levels
        for layer in self.encoder.layers:
            layer.attentions[0].fused_backward = self.fused_backward
        assert self.num_encoder_levels >= 1, 'num_levels in attn_cfgs must be at least one'
        if self.num_encoder_levels > self.num_input_levels:
            raise ValueError(f'{self.num_encoder_levels} encoder levels from {self.num_input_levels} inputs')
        if self.encoder.embed_dims != feat_channels:
            raise ValueError(f'encoder embed_dims {self.encoder.embed_dims} != feat_channels {feat_channels}')
        g = _get(norm_cfg, 'num_groups', 32)
        # from top to down (low to high resolution), :84-97
        self.input_convs = nn.ModuleList([_ConvModule(in_channels[i], feat_channels, 1, 0, True, g, False)
                                          for i in range(self.num_input_levels - 1, self.num_input_levels - self.num_encoder_levels - 1, -1)])
        pe = {k: v for k, v in dict(positional_encoding).items() if k != 'type'}
        self.postional_encoding = SinePositionalEncoding(**pe)           # (the reference's spelling; it holds no parameter)
        if 2 * self.postional_encoding.num_feats != feat_channels:
            raise ValueError(f'positional encoding of {2 * self.postional_encoding.num_feats} channels for feat_channels {feat_channels}')
        self.level_encoding = nn.Embedding(self.num_encoder_levels, feat_channels)
        # fpn for the rest features that didn't pass in encoder, :107-131
        self.lateral_convs, self.output_convs = nn.ModuleList(), nn.ModuleList()
        self.use_bias = False
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):
            self.lateral_convs.append(_ConvModule(in_channels[i], feat_channels, 1, 0, False, g, False))
            self.output_convs.append(_ConvModule(feat_channels, feat_channels, 3, 1, False, g, True))
        self.mask_feature = nn.Conv2d(feat_channels, out_channels, kernel_size=1, stride=1, padding=0)
        self.num_outs = num_outs
        self._shape_cache = {}
        self._prep = None

    def init_weights(self):
        """:139-163"""
        for i in range(self.num_encoder_levels):
            nn.init.xavier_uniform_(self.input_convs[i].conv.weight, gain=1)
            nn.init.constant_(self.input_convs[i].conv.bias, 0)
        for m in [c.conv for c in list(self.lateral_convs) + list(self.output_convs)] + [self.mask_feature]:      # caffe2_xavier_init
            nn.init.kaiming_uniform_(m.weight, a=1, mode='fan_in', nonlinearity='leaky_relu')
            if m.bias is not None:
                nn.init.constant_(m.bias, 0)
        nn.init.normal_(self.level_encoding.weight, 0, 1)
        for p in self.encoder.parameters():
            if p.dim() > 1:
                nn.init.xavier_normal_(p)
        for layer in self.encoder.layers:
            for attn in layer.attentions:
                attn.init_weights()

    # ------------------------------------------------------------------------------------------------------------------
    def _level_shapes(self, feats):
        return [tuple(int(v) for v in feats[self.num_input_levels - i - 1].shape[-2:]) for i in range(self.num_encoder_levels)]

    def shape_constants(self, shapes, device):
        """Per tuple of level shapes, cached on the device as `SemanticFPNWrapper.positional_map` does: the sine encoding of the
        all-valid masks [Q, C] (levels concatenated) and the reference points [Q, L, 2] of :198-202, 230-231."""
        key = (tuple(shapes), str(device))
        hit = self._shape_cache.get(key)
        if hit is None:
            pos, ref = [], []
            for i, (h, w) in enumerate(shapes):
                stride = self.strides[self.num_input_levels - i - 1]
                pos.append(self.postional_encoding(torch.zeros((1, h, w), dtype=torch.bool, device=device))[0].flatten(1).t())
                xs = (torch.arange(w, dtype=torch.float32, device=device) + 0.5) * stride          # MlvlPointGenerator, offset 0.5
                ys = (torch.arange(h, dtype=torch.float32, device=device) + 0.5) * stride
                pts = torch.stack([xs.repeat(h), ys.repeat_interleave(w)], -1)
                ref.append(pts / torch.tensor([[w, h]], dtype=torch.float32, device=device).mul(stride))
            ref = torch.cat(ref, 0)[:, None].repeat(1, self.num_encoder_levels, 1)
            hit = self._shape_cache[key] = (torch.cat(pos, 0).contiguous(), ref.contiguous())
        return hit

    def _level_pos(self, shapes, device):
        """level_positional_encodings of :194-196: the level's embedding row + the sine encoding, [Q, C] fp32"""
        pos, ref = self.shape_constants(shapes, device)
        lvl = torch.cat([self.level_encoding.weight[i].float().expand(h * w, -1) for i, (h, w) in enumerate(shapes)], 0)
        return lvl + pos, ref

    def _tail(self, feats, outs):
        """:259-275 — the FPN over the inputs that did not pass the encoder, `mask_feature`, the output order"""
        for i in range(self.num_input_levels - self.num_encoder_levels - 1, -1, -1):
            cur = self.lateral_convs[i](feats[i])
            y = cur + F.interpolate(outs[-1], size=cur.shape[-2:], mode='bilinear', align_corners=False)
            outs.append(self.output_convs[i](y))
        multi_scale_features = outs[:self.num_outs]
        multi_scale_features.append(self.mask_feature(outs[-1]))
        multi_scale_features.reverse()
        return tuple(multi_scale_features)

    def _split(self, memory, shapes, B):
        """memory [B, C, Q] -> the levels' maps [B, C, H_l, W_l], low to high resolution"""
        outs = torch.split(memory, [h * w for h, w in shapes], dim=-1)
        return [x.reshape(B, -1, h, w) for x, (h, w) in zip(outs, shapes)]

    def forward_torch(self, feats):
        """The reference forward (:165-275) as the torch composition of this module's layers (differentiable)."""
        B = feats[0].shape[0]
        shapes = self._level_shapes(feats)
        proj = [self.input_convs[i](feats[self.num_input_levels - i - 1]).flatten(2).permute(2, 0, 1) for i in range(self.num_encoder_levels)]
        query = torch.cat(proj, 0)                                                                   # [Q, B, C]
        pos, ref = self._level_pos(shapes, query.device)
        pos, ref = pos.to(query.dtype), ref.to(query.dtype)
        memory = self.encoder(query, pos[:, None].expand(-1, B, -1), ref, shapes)
        return self._tail(feats, self._split(memory.permute(1, 2, 0), shapes, B))

    # ------------------------------------------------------------------------------------------------------------------
    def fused_ok(self, feats):
        """The fused path's terms: CUDA fp32 inputs and parameters, the sampling core's envelope, LayerNorm rows of <= 256 channels"""
        attn = self.encoder.layers[0].attentions[0]
        C = self.feat_channels
        if not (ops.msda_fits(attn.num_heads, C // attn.num_heads, attn.num_levels, attn.num_points) and C % 32 == 0
                and self.encoder.layers[0].ffns[0].feedforward_channels % 32 == 0):
            return False
        if not all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in feats):
            return False
        if not all(p.is_cuda and p.dtype == torch.float32 for p in self.parameters()):
            return False
        B, Q = feats[0].shape[0], sum(h * w for h, w in self._level_shapes(feats))
        widest = max(C, 3 * attn.num_heads * attn.num_levels * attn.num_points, self.encoder.layers[0].ffns[0].feedforward_channels)
        return B * Q * widest * 4 < 2 ** 31

    def _needs_grad(self, feats):
        return torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                            or any(torch.is_tensor(x) and x.requires_grad for x in feats))

    def prepared(self):
        """Per layer the split weight images and biases of the five GEMMs (offsets and logits as ONE [3 M L P][C] matrix), rebuilt
        when any encoder weight changed (tensor version counters) or moved: `SemanticFPNWrapper.prepared`'s rule."""
        params = [p for layer in self.encoder.layers for p in layer.parameters()]
        key = tuple((p.data_ptr(), p._version) for p in params)
        if self._prep is not None and self._prep[0] == key:
            return self._prep[1]
        prep = []
        with torch.no_grad():
            for layer in self.encoder.layers:
                a, f = layer.attentions[0], layer.ffns[0]
                mats = dict(qk=(torch.cat([a.sampling_offsets.weight, a.attention_weights.weight], 0).contiguous(),
                                torch.cat([a.sampling_offsets.bias, a.attention_weights.bias]).contiguous()),
                            value=(a.value_proj.weight.detach(), a.value_proj.bias.detach()),
                            out=(a.output_proj.weight.detach(), a.output_proj.bias.detach()),
                            fc1=(f.layers[0][0].weight.detach(), f.layers[0][0].bias.detach()),
                            fc2=(f.layers[1].weight.detach(), f.layers[1].bias.detach()))
                prep.append({k: (w, b, ops.split_weight(w)) for k, (w, b) in mats.items()})
        self._prep = (key, prep)
        return prep

    def forward_fused(self, feats):
        """The encoder on the library's kernels (no gradient); the convs around it are the module's torch layers."""
        B = feats[0].shape[0]
        shapes = self._level_shapes(feats)
        C = self.feat_channels
        proj = [self.input_convs[i](feats[self.num_input_levels - i - 1]).flatten(2) for i in range(self.num_encoder_levels)]
        x = torch.cat(proj, 2).transpose(1, 2).contiguous()                                          # [B, Q, C]: batch-first rows
        Q = x.shape[1]
        pos, ref = self._level_pos(shapes, x.device)
        x = x.view(B * Q, C)
        for layer, w in zip(self.encoder.layers, self.prepared()):
            a = layer.attentions[0]
            n_off = 2 * a.num_heads * a.num_levels * a.num_points
            q = (x.view(B, Q, C) + pos).view(B * Q, C)
            ol = ops.linear(q, w['qk'][0], w['qk'][1], w_split=w['qk'][2])                           # [B Q, 3 M L P]: offsets | logits
            value = ops.linear(x, w['value'][0], w['value'][1], w_split=w['value'][2])
            core = ops.msda_sample(value.view(B, Q, C), shapes, ol[:, :n_off], ol[:, n_off:], ref, a.num_heads, a.num_points)
            y = ops.linear(core.view(B * Q, C), w['out'][0], w['out'][1], w_split=w['out'][2])
            x = ops.layernorm_act(y, layer.norms[0].weight, layer.norms[0].bias, resid=x, eps=layer.norms[0].eps)
            h = ops.linear(x, w['fc1'][0], w['fc1'][1], w_split=w['fc1'][2], act=1)
            y = ops.linear(h, w['fc2'][0], w['fc2'][1], w_split=w['fc2'][2])
            x = ops.layernorm_act(y, layer.norms[1].weight, layer.norms[1].bias, resid=x, eps=layer.norms[1].eps)
        return self._tail(feats, self._split(x.view(B, Q, C).transpose(1, 2), shapes, B))

    def forward(self, feats):
        if self.fused and not self._needs_grad(feats) and self.fused_ok(feats):
            with torch.no_grad():
                return self.forward_fused(feats)
        return self.forward_torch(feats)


NECKS.register_module(force=True)(MSDeformAttnPixelDecoder)
