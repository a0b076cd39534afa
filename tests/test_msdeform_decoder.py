"""CPU: `MSDeformAttnPixelDecoder` (video-k-net_amd/msdeform_decoder.py) as a drop-in for knet/det/msdeformattn_decoder.py — it builds
through `NECKS` from the reference's own neck dicts (tests/golden/msda_neck_cfgs.json: settings only), has the reference's state-dict
keys, its `forward_torch` matches the float64 restatement of tests/msda_ref.py, its outputs come in the reference's order, and
whatever no shipped config uses raises at construction."""
import copy
import json
import math
import os

import pytest
import torch

import msda_ref as R
from helpers import GOLDEN

with open(os.path.join(GOLDEN, 'msda_neck_cfgs.json')) as _f:
    NECK_CFGS = {k: v for k, v in json.load(_f).items() if not k.startswith('_')}
BASE = next(iter(NECK_CFGS.values()))


@pytest.mark.parametrize('name', list(NECK_CFGS))
def test_builds_through_necks_with_the_reference_keys(vkn, name):
    assert len(NECK_CFGS) == 2
    neck = vkn.build_neck(copy.deepcopy(NECK_CFGS[name]))
    assert type(neck) is vkn.MSDeformAttnPixelDecoder is vkn.NECKS.get('MSDeformAttnPixelDecoder')
    assert sorted(neck.state_dict()) == R.expected_keys(num_layers=6) and len(R.expected_keys(6)) == 117
    assert not any('post_norm' in k for k in neck.state_dict())
    sd = neck.state_dict()
    assert sd['encoder.layers.5.attentions.0.sampling_offsets.weight'].shape == (8 * 3 * 4 * 2, 256)
    assert sd['encoder.layers.0.attentions.0.attention_weights.weight'].shape == (8 * 3 * 4, 256)
    assert sd['encoder.layers.0.ffns.0.layers.0.0.weight'].shape == (1024, 256) and sd['encoder.layers.0.ffns.0.layers.1.weight'].shape == (256, 1024)
    assert sd['input_convs.0.conv.weight'].shape == (256, 2048, 1, 1) and sd['input_convs.2.conv.weight'].shape == (256, 512, 1, 1)
    assert sd['lateral_convs.0.conv.weight'].shape == (256, 256, 1, 1) and sd['output_convs.0.conv.weight'].shape == (256, 256, 3, 3)
    assert sd['level_encoding.weight'].shape == (3, 256) and sd['mask_feature.weight'].shape == (256, 256, 1, 1)
    assert (neck.num_encoder_levels, neck.num_input_levels, neck.num_outs, neck.strides) == (3, 4, 3, [4, 8, 16, 32])


def test_defaults_are_the_references(vkn):
    neck = vkn.MSDeformAttnPixelDecoder()                                          # :42-75, the deprecated layer-level FFN arguments
    assert sorted(neck.state_dict()) == R.expected_keys(num_layers=6)
    assert neck.in_channels == [256, 512, 1024, 2048] and neck.return_one_list is True
    assert neck.encoder.layers[0].ffns[0].feedforward_channels == 1024 and neck.postional_encoding.normalize is True
    # the kernel head builds it where a config names it as its neck
    assert type(vkn.ConvKernelHead._build_neck(copy.deepcopy(BASE))) is vkn.MSDeformAttnPixelDecoder


@torch.no_grad()
def test_init_weights_follows_the_reference(vkn):
    torch.manual_seed(3)
    neck = vkn.build_neck(R.module_cfg(R.MODULE_CASES['narrow'], BASE))
    neck.init_weights()
    for layer in neck.encoder.layers:
        a = layer.attentions[0]
        assert float(a.sampling_offsets.weight.abs().max()) == 0 and float(a.attention_weights.weight.abs().max()) == 0
        assert float(a.attention_weights.bias.abs().max()) == 0 and float(a.value_proj.bias.abs().max()) == 0
        grid = a.sampling_offsets.bias.view(a.num_heads, a.num_levels, a.num_points, 2)
        for m in range(a.num_heads):
            th = m * 2 * math.pi / a.num_heads
            d = torch.tensor([math.cos(th), math.sin(th)])
            d = d / d.abs().max()
            for p in range(a.num_points):
                assert torch.allclose(grid[m, :, p], (d * (p + 1)).expand(a.num_levels, 2), atol=1e-6)
        lim = math.sqrt(6 / (2 * a.embed_dims))
        assert 0.9 * lim < float(a.value_proj.weight.abs().max()) <= lim and 0.9 * lim < float(a.output_proj.weight.abs().max()) <= lim
        assert float(layer.ffns[0].layers[0][0].weight.std()) == pytest.approx(math.sqrt(2 / (64 + 1024)), rel=0.05)
    assert float(neck.input_convs[0].conv.bias.abs().max()) == 0 and float(neck.mask_feature.bias.abs().max()) == 0
    assert float(neck.level_encoding.weight.std()) == pytest.approx(1.0, rel=0.2)
    lim = math.sqrt(6 / (128 + 64))
    assert 0.9 * lim < float(neck.input_convs[0].conv.weight.abs().max()) <= lim                     # xavier uniform, fan 128 -> 64
    lim = math.sqrt(3 / 32)
    assert 0.9 * lim < float(neck.lateral_convs[0].conv.weight.abs().max()) <= lim                   # caffe2 xavier: kaiming uniform, a = 1, fan_in 32


@pytest.mark.parametrize('name', list(R.MODULE_CASES))
def test_forward_torch_matches_the_float64_restatement(vkn, name):
    case = R.MODULE_CASES[name]
    torch.manual_seed(11)
    neck = vkn.build_neck(R.module_cfg(case, BASE))
    neck.init_weights()
    R.randomise(neck, 12)
    neck.eval()
    feats = R.module_inputs(case, 13)
    want = R.decoder_f64(neck.state_dict(), feats, num_heads=case['num_heads'])
    with torch.no_grad():
        got = neck(feats)                                                          # CPU tensors: forward_torch
        again = neck.forward_torch(feats)
    assert isinstance(got, tuple) and len(got) == len(want) == 4
    # :270-275 — mask_feature first, then the multi-scale features from the highest encoder level down
    B, C = case['B'], case['feat_channels']
    assert [tuple(g.shape) for g in got] == [(B, C) + tuple(s) for s in case['sizes']] == [tuple(w.shape) for w in want]
    # fp32 against float64: each of the about 60 GEMM / normalisation stages of six layers adds at most sqrt(K) 2^-24 = 2.7e-6 of the
    # O(1) magnitudes that LayerNorm keeps (K <= 2048), stacked linearly: 1.6e-4 — a wrong term is O(1e-2) and more (below)
    for g, a, w in zip(got, again, want):
        assert torch.equal(g, a)
        assert float((g.double() - w).abs().max()) <= 2e-4 * max(1.0, float(w.abs().max())), name
    # the offsets really move the samples: the reference points alone give another result
    flat = {k: (torch.zeros_like(v) if 'sampling_offsets' in k else v) for k, v in neck.state_dict().items()}
    moved = R.decoder_f64(flat, feats, num_heads=case['num_heads'])
    assert float((moved[1] - want[1]).abs().max()) > 1e-2
    # with a gradient the same path runs, and reaches every parameter and input
    neck.train()
    ins = [f.clone().requires_grad_(True) for f in feats]
    sum(o.square().mean() for o in neck(ins)).backward()
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in neck.parameters())
    assert all(x.grad is not None and float(x.grad.abs().max()) > 0 for x in ins)


def test_unshipped_options_raise(vkn):
    def build(**edit):
        cfg = copy.deepcopy(BASE)
        for path, v in edit.items():
            node, keys = cfg, path.split('__')
            for k in keys[:-1]:
                node = node[k]
            node[keys[-1]] = v
        return vkn.build_neck(cfg)
    build()
    layer, attn, ffn = 'encoder__transformerlayers__', 'encoder__transformerlayers__attn_cfgs__', 'encoder__transformerlayers__ffn_cfgs__'
    for edit in ({attn + 'dropout': 0.1}, {attn + 'batch_first': True}, {layer + 'batch_first': True}, {attn + 'norm_cfg': dict(type='LN')},
                 {layer + 'norm_cfg': dict(type='BN')}, {ffn + 'act_cfg': dict(type='GELU')}, {ffn + 'num_fcs': 3}, {ffn + 'ffn_drop': 0.1},
                 {ffn + 'type': 'MoEFFN'}, {ffn + 'add_identity': False},
                 {layer + 'operation_order': ['norm', 'self_attn', 'norm', 'ffn']}, {layer + 'operation_order': ['self_attn', 'norm', 'cross_attn', 'norm', 'ffn', 'norm']},
                 {'encoder__type': 'DeformableDetrTransformerEncoder'}, {layer + 'type': 'DetrTransformerDecoderLayer'},
                 {attn + 'type': 'MultiheadAttention'}, {'norm_cfg': None}, {'norm_cfg': dict(type='BN')}, {'act_cfg': dict(type='GELU')},
                 {'positional_encoding__type': 'LearnedPositionalEncoding'}, {layer + 'ffn_dropout': 0.1}):
        with pytest.raises(NotImplementedError):
            build(**edit)
    cfg = copy.deepcopy(BASE)
    del cfg['encoder']['transformerlayers']['attn_cfgs']['dropout']                # mmcv's own default is dropout = 0.1
    with pytest.raises(NotImplementedError):
        vkn.build_neck(cfg)
    with pytest.raises(KeyError):
        vkn.build_neck(dict(type='NoSuchNeck'))
