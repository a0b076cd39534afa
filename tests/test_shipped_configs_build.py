"""Every config the reference ships, with its `rpn_head`, `roi_head` and `tracker` dicts built through THIS package's registries exactly
as the reference's detectors hand them over (`train_cfg` / `test_cfg` of the model folded in: knet/det/knet.py:40-52,
knet/video/knet.py): the constructor surface a user who switches frameworks relies on.  The configs' model dicts, their `_base_`
inheritance resolved, are stored data (tests/golden/shipped_configs.json, written by oracle/gen_golden_api.py from the reference)."""
import copy
import json
import os

import pytest
import torch.nn as nn

FIXTURE = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden', 'shipped_configs.json')

# parts of a model dict that are outside SURVEY.md §8: the backbone-side FPN wrapper (dense convolutions, §2 row 9) is replaced by a
# placeholder module below.  The quasi-dense EMBEDDING head (`track_head`) builds since round 4 (video-k-net_amd/track_heads.py).
OUT_OF_SCOPE = set()


def _decode(v):
    if isinstance(v, dict):
        return tuple(_decode(a) for a in v['__tuple__']) if set(v) == {'__tuple__'} else {k: _decode(a) for k, a in v.items()}
    if isinstance(v, list):
        return [_decode(a) for a in v]
    return v


with open(FIXTURE) as _f:
    CONFIGS = json.load(_f)


class _Neck(nn.Module):
    """Stands where a config names the backbone-side `localization_fpn`."""


def _strip_necks(d):
    return {k: (_Neck() if k == 'localization_fpn' and isinstance(v, dict) else v) for k, v in d.items()}


@pytest.mark.parametrize('path', sorted(CONFIGS), ids=str)
def test_every_shipped_config_builds_through_the_registries(vkn, path):
    entry = CONFIGS[path]
    if 'skip' in entry:                       # two shipped configs name `_base_` files the reference tree does not contain
        pytest.skip(entry['skip'])
    model = _decode(entry['model'])
    train_cfg, test_cfg = model.get('train_cfg') or {}, model.get('test_cfg') or {}
    built = []
    for part, key in (('rpn_head', 'rpn'), ('roi_head', 'rcnn')):
        if model.get(part):
            hd = _strip_necks(copy.deepcopy(model[part]))
            hd.update(train_cfg=train_cfg.get(key), test_cfg=test_cfg.get(key))
            built.append(vkn.build_head(hd))
    trk = model.get('tracker')
    if trk:
        if 'Tracker' in trk['type']:
            built.append(vkn.build_tracker(copy.deepcopy(trk)))
        else:                                   # the VIS models: `tracker` is the clip-level iteration head
            hd = copy.deepcopy(trk)
            hd.update(train_cfg=train_cfg.get('tracker'), test_cfg=test_cfg.get('tracker'))
            built.append(vkn.build_head(hd))
    th = model.get('track_head')
    if th:
        assert th['type'] not in OUT_OF_SCOPE, th['type']
        built.append(vkn.build_head(copy.deepcopy(th)))
    assert built, 'a model config without any part of the path'
    for m in built:
        if isinstance(m, nn.Module):
            assert sum(p.numel() for p in m.parameters()) > 0
