"""`SemanticFPNWrapper` — drop-in for the reference's localization FPN (knet/det/semantic_fpn_wrapper.py:16-237): same ctor kwargs,
module tree, state-dict keys (mmcv `ConvModule` names `conv` / `gn`) and returns.  Every shipped config gives its `rpn_head` the same
one (GN(32) + ReLU, positional encoding at level 3, upsample_times 2, one aux conv).

Inference (no gradient needed) is ONE C-ABI call (`vkn_localization_fpn_f32`: implicit-GEMM 3x3 convs on MFMA, GroupNorm + ReLU
applied on load by each consumer); with a gradient the module runs the plain torch composition of its own layers, so training works
on the same parameters.  With `fused_backward=True` (an extra keyword, off by default) that training forward runs every
ConvModule inside the kernels' envelope through `autograd.ConvGNReLUFn`: conv + GroupNorm + ReLU forward and backward in HIP
(include/vkn_fpn_train.h), the bilinear x2, the level sum and the positional add staying torch autograd ops.
"""
import math

import torch
import torch.nn as nn

from . import autograd, ops
from .registry import HAVE_MM, HEADS


class SinePositionalEncoding(nn.Module):
    """mmdet 2.x `SinePositionalEncoding` (mmdet/models/utils/positional_encoding.py) for an all-valid mask: the only one this
    package's FPN asks for.  Output [B, 2 num_feats, H, W] in fp32: cat(pos_y, pos_x), sin on even / cos on odd features."""

    def __init__(self, num_feats, temperature=10000, normalize=False, scale=2 * math.pi, eps=1e-6, offset=0.0, init_cfg=None):
        super().__init__()
        if normalize and not isinstance(scale, (float, int)):
            raise TypeError('scale should be a float or int when normalize is True')
        self.num_feats, self.temperature, self.normalize = num_feats, temperature, normalize
        self.scale, self.eps, self.offset = scale, eps, offset

    def forward(self, mask):
        not_mask = (~mask).to(torch.float32)
        y_embed = not_mask.cumsum(1, dtype=torch.float32)
        x_embed = not_mask.cumsum(2, dtype=torch.float32)
        if self.normalize:
            y_embed = (y_embed + self.offset) / (y_embed[:, -1:, :] + self.eps) * self.scale
            x_embed = (x_embed + self.offset) / (x_embed[:, :, -1:] + self.eps) * self.scale
        dim_t = torch.arange(self.num_feats, dtype=torch.float32, device=mask.device)
        dim_t = self.temperature ** (2 * (dim_t // 2) / self.num_feats)
        pos_x = x_embed[:, :, :, None] / dim_t
        pos_y = y_embed[:, :, :, None] / dim_t
        B, H, W = mask.shape
        pos_x = torch.stack((pos_x[:, :, :, 0::2].sin(), pos_x[:, :, :, 1::2].cos()), dim=4).view(B, H, W, -1)
        pos_y = torch.stack((pos_y[:, :, :, 0::2].sin(), pos_y[:, :, :, 1::2].cos()), dim=4).view(B, H, W, -1)
        return torch.cat((pos_y, pos_x), dim=3).permute(0, 3, 1, 2)


class _ConvModule(nn.Module):
    """mmcv `ConvModule(cin, cout, k, stride, padding, norm_cfg=GN, act_cfg=ReLU)`: conv (no bias: a norm follows) -> GN -> ReLU,
    with mmcv's attribute names so that the state-dict keys are the reference's."""

    def __init__(self, cin, cout, k, stride, padding, num_groups):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride=stride, padding=padding, bias=False)
        self.gn = nn.GroupNorm(num_groups, cout)
        self.activate = nn.ReLU()

    def forward(self, x):
        return self.activate(self.gn(self.conv(x)))


def _unsupported(what):
    raise NotImplementedError(f'SemanticFPNWrapper {what} is not built (no shipped config uses it)')


class SemanticFPNWrapper(nn.Module):
    """knet/det/semantic_fpn_wrapper.py:16-237."""

    def __init__(self, in_channels, feat_channels, out_channels, start_level, end_level, cat_coors=False, positional_encoding=None,
                 cat_coors_level=3, fuse_by_cat=False, return_list=False, upsample_times=3, with_pred=True, num_aux_convs=0,
                 act_cfg=dict(type='ReLU', inplace=True), out_act_cfg=dict(type='ReLU'), conv_cfg=None, norm_cfg=None,
                 fused_backward=False):
        super().__init__()
        self.fused_backward = bool(fused_backward)      # not the reference's: the training forward on the HIP block (forward_train_fused)
        assert start_level >= 0 and end_level >= start_level
        if cat_coors:
            _unsupported('cat_coors=True')
        if fuse_by_cat:
            _unsupported('fuse_by_cat=True')
        if conv_cfg is not None:
            _unsupported(f'conv_cfg={conv_cfg!r}')
        if norm_cfg is None or norm_cfg.get('type') != 'GN':
            _unsupported(f'norm_cfg={norm_cfg!r} (GN only)')
        for cfg in (act_cfg, out_act_cfg):
            if cfg is None or cfg.get('type') != 'ReLU':
                _unsupported(f'activation {cfg!r} (ReLU only)')
        if positional_encoding is not None and positional_encoding.get('type', 'SinePositionalEncoding') != 'SinePositionalEncoding':
            _unsupported(f'positional_encoding type {positional_encoding.get("type")!r}')
        self.in_channels, self.feat_channels, self.out_channels = in_channels, feat_channels, out_channels
        self.start_level, self.end_level = start_level, end_level
        self.conv_cfg, self.norm_cfg, self.act_cfg = conv_cfg, norm_cfg, act_cfg
        self.cat_coors, self.cat_coors_level, self.fuse_by_cat = cat_coors, cat_coors_level, fuse_by_cat
        self.return_list, self.upsample_times, self.with_pred = return_list, upsample_times, with_pred
        self.num_groups = norm_cfg.get('num_groups', 32)
        if positional_encoding is not None:
            pe = {k: v for k, v in positional_encoding.items() if k != 'type'}
            self.positional_encoding = SinePositionalEncoding(**pe)
        else:
            self.positional_encoding = None
        g = self.num_groups
        # module tree of :73-146
        self.convs_all_levels = nn.ModuleList()
        for i in range(start_level, end_level + 1):
            level = nn.Sequential()
            if i == 0:
                if upsample_times == end_level - i:
                    level.add_module('conv0', _ConvModule(in_channels, feat_channels, 3, 1, 1, g))
                else:
                    for j in range(end_level - upsample_times):
                        level.add_module('conv' + str(j), _ConvModule(in_channels, feat_channels, 3, 2, 1, g))
                self.convs_all_levels.append(level)
                continue
            for j in range(i):
                level.add_module('conv' + str(j), _ConvModule(in_channels if j == 0 else feat_channels, feat_channels, 3, 1, 1, g))
                if j < upsample_times - (end_level - i):
                    level.add_module('upsample' + str(j), nn.Upsample(scale_factor=2, mode='bilinear', align_corners=False))
            self.convs_all_levels.append(level)
        if with_pred:
            self.conv_pred = _ConvModule(feat_channels, out_channels, 1, 1, 0, g)
        self.num_aux_convs = num_aux_convs
        self.aux_convs = nn.ModuleList([_ConvModule(feat_channels, out_channels, 1, 1, 0, g) for _ in range(num_aux_convs)])
        self._pos_cache = {}
        self._prep = None

    def init_weights(self):
        """:178-183: normal_init(std=0.01), bias 0, on every Conv2d."""
        for m in self.modules():
            if isinstance(m, nn.Conv2d):
                nn.init.normal_(m.weight, 0, 0.01)
                if m.bias is not None:
                    nn.init.constant_(m.bias, 0)

    # ------------------------------------------------------------------------------------------------------------------
    def positional_map(self, B, H, W, device):
        """The encoding of an all-valid [B, H, W] mask: a constant per shape, cached on the device by (H, W, device)."""
        key = (int(H), int(W), str(device))
        pos = self._pos_cache.get(key)
        if pos is None:
            pos = self.positional_encoding(torch.zeros((1, H, W), dtype=torch.bool, device=device)).contiguous()
            self._pos_cache[key] = pos
        return pos.expand(B, -1, -1, -1)

    def forward_torch(self, inputs):
        """The reference forward (:197-237) as the torch composition of this module's layers (differentiable)."""
        mlvl = []
        for i in range(self.start_level, self.end_level + 1):
            x = inputs[i]
            if i == self.cat_coors_level and self.positional_encoding is not None:
                x = x + self.positional_map(x.shape[0], x.shape[-2], x.shape[-1], x.device).to(x.dtype)
            mlvl.append(self.convs_all_levels[i](x))
        feat = sum(mlvl)
        out = self.conv_pred(feat) if self.with_pred else feat
        if self.num_aux_convs > 0:
            return [out] + [conv(feat) for conv in self.aux_convs]
        return [out] if self.return_list else out

    def _conv_modules(self):
        return [m for m in self.modules() if isinstance(m, _ConvModule)]

    def train_fused_ok(self, inputs):
        """Every ConvModule inside the envelope of include/vkn_fpn_train.h, every input an fp32 tensor on the GPU"""
        return (all(ops.conv_gn_relu_fits(m.conv.in_channels, m.conv.out_channels, m.conv.kernel_size[0], m.conv.stride[0], m.gn.num_groups)
                    and m.conv.weight.is_cuda and m.conv.weight.dtype == torch.float32 for m in self._conv_modules())
                and all(torch.is_tensor(x) and x.is_cuda and x.dtype == torch.float32 for x in inputs[self.start_level:self.end_level + 1]))

    @staticmethod
    def _block(m, x):
        return autograd.conv_gn_relu(x, m.conv.weight, m.gn.weight, m.gn.bias, m.gn.num_groups, m.conv.stride[0])

    def forward_train_fused(self, inputs):
        """`forward_torch` with every ConvModule as one `autograd.ConvGNReLUFn` (HIP forward and backward); `nn.Upsample`, the level
        sum and the positional add are the same torch ops."""
        mlvl = []
        for i in range(self.start_level, self.end_level + 1):
            x = inputs[i]
            if i == self.cat_coors_level and self.positional_encoding is not None:
                x = x + self.positional_map(x.shape[0], x.shape[-2], x.shape[-1], x.device).to(x.dtype)
            for layer in self.convs_all_levels[i]:
                x = self._block(layer, x) if isinstance(layer, _ConvModule) else layer(x)
            mlvl.append(x)
        feat = sum(mlvl)
        out = self._block(self.conv_pred, feat) if self.with_pred else feat
        if self.num_aux_convs > 0:
            return [out] + [self._block(conv, feat) for conv in self.aux_convs]
        return [out] if self.return_list else out

    def fused_ok(self):
        """The structure `vkn_localization_fpn_f32` implements: every shipped config's."""
        return (self.start_level == 0 and self.end_level == 3 and self.upsample_times == 2 and self.with_pred and self.num_aux_convs == 1
                and self.cat_coors_level == 3 and self.in_channels == self.feat_channels == self.out_channels
                and self.out_channels % 32 == 0 and self.out_channels <= 256)

    def _needs_grad(self, inputs):
        return torch.is_grad_enabled() and (any(p.requires_grad for p in self.parameters())
                                            or any(torch.is_tensor(x) and x.requires_grad for x in inputs))

    def _layers(self):
        lv = self.convs_all_levels
        return [lv[0].conv0, lv[1].conv0, lv[2].conv0, lv[2].conv1, lv[3].conv0, lv[3].conv1, lv[3].conv2]

    def prepared(self, extra=()):
        """Prepared weight images + GN affines in the order of include/vkn.h (`extra`: the head's loc / seg ConvModules), rebuilt when
        any weight changed (tensor version counters) or moved."""
        mods = self._layers()
        key = tuple((m.conv.weight.data_ptr(), m.conv.weight._version) for m in mods + [self.conv_pred, self.aux_convs[0]] + list(extra))
        key += tuple((m.gn.weight.data_ptr(), m.gn.weight._version, m.gn.bias._version) for m in [self.conv_pred, self.aux_convs[0]])
        if self._prep is not None and self._prep[0] == key:
            return self._prep[1]
        with torch.no_grad():
            imgs = [ops.conv_prepare(m.conv.weight) for m in mods]
            imgs.append(ops.conv_prepare(torch.cat([self.conv_pred.conv.weight, self.aux_convs[0].conv.weight], 0)))
            imgs += [ops.conv_prepare(m.conv.weight) for m in extra]
            gam = [m.gn.weight.detach() for m in mods] + [torch.cat([self.conv_pred.gn.weight, self.aux_convs[0].gn.weight]).detach()]
            bet = [m.gn.bias.detach() for m in mods] + [torch.cat([self.conv_pred.gn.bias, self.aux_convs[0].gn.bias]).detach()]
            gam += [m.gn.weight.detach() for m in extra]
            bet += [m.gn.bias.detach() for m in extra]
        prep = (imgs, gam, bet)
        self._prep = (key, prep)
        return prep

    def forward_fused(self, inputs, loc_convs=None, seg_convs=None):
        """One C-ABI call from P2..P5: [out, aux], or — with the head's single loc / seg ConvModules — their outputs (loc, sem)."""
        p2, p3, p4, p5 = inputs[:4]
        pos = None
        if self.positional_encoding is not None:
            pos = self.positional_map(1, p5.shape[-2], p5.shape[-1], p5.device)[0]
        extra = [loc_convs, seg_convs] if loc_convs is not None else []
        imgs, gam, bet = self.prepared(extra)
        loc, sem = ops.localization_fpn(p2, p3, p4, p5, pos, imgs, gam, bet, self.num_groups)
        return [loc, sem]

    def forward(self, inputs):
        if self._needs_grad(inputs):
            if self.fused_backward and self.train_fused_ok(inputs):
                return self.forward_train_fused(inputs)
            return self.forward_torch(inputs)
        if not self.fused_ok():
            raise NotImplementedError('SemanticFPNWrapper inference is built for the shipped structure (levels 0-3, upsample_times=2, '
                                      'with_pred, one aux conv, equal channel counts <= 256): this one runs only with gradients')
        return self.forward_fused(inputs)


def _register():
    """Bundled registry: ours.  Under real mmdet: registered in NECKS only where the name is absent (the reference's own class
    stays, registry.py's FocalLoss / DiceLoss rule)."""
    if HAVE_MM:
        from mmdet.models.builder import NECKS  # type: ignore
        if NECKS.get('SemanticFPNWrapper') is None:
            NECKS.register_module()(SemanticFPNWrapper)
        return
    HEADS.register_module(force=True)(SemanticFPNWrapper)


_register()
