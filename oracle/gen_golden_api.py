#!/usr/bin/env python3
"""Generate the two JSON fixtures of the API tests from the REFERENCE ITSELF (build container only: needs the reference checkout).

    VKN_REFERENCE=<reference checkout> python oracle/gen_golden_api.py     # rewrites the two files below

tests/golden/shipped_configs.json (tests/test_shipped_configs_build.py)
    every model config the reference ships (configs/**.py outside `_base_/` and `common/`), its `_base_` inheritance resolved the
    way mmcv's `Config.fromfile` does for plain dict configs; stored per config path: the parts of its `model` dict the test builds
    (`rpn_head`, `roi_head`, `tracker`, `track_head`, `train_cfg`, `test_cfg`), or why it cannot be built.  Tuples are stored as
    {"__tuple__": [...]}.
tests/golden/reference_api_surface.json (tests/test_reference_api_surface.py)
    for every reference class this package mirrors: the methods the class defines itself and their parameters
    ([name, has default, kind]).  The classes are imported UNMODIFIED through the plumbing stand-ins of oracle/standins, as
    oracle/gen_golden.py does; a class the stand-ins cannot carry is stored as {"__error__": message}.
"""
import copy
import importlib
import inspect
import json
import os
import sys

sys.dont_write_bytecode = True
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('VKN_REFERENCE')
OUT = os.environ.get('VKN_GOLDEN_OUT', os.path.join(ROOT, 'tests', 'golden'))

MODEL_PARTS = ('rpn_head', 'roi_head', 'tracker', 'track_head', 'train_cfg', 'test_cfg')

# reference class -> class here (tests/test_reference_api_surface.py checks this package against the stored surface of each)
PAIRS = {
    'knet.kernel_updator:KernelUpdator': 'KernelUpdator',
    'knet.det.kernel_update_head:KernelUpdateHead': 'KernelUpdateHead',
    'knet.det.kernel_iter_head:KernelIterHead': 'KernelIterHead',
    'knet.video.kernel_update_head:VideoKernelUpdateHead': 'VideoKernelUpdateHead',
    'knet.video.kernel_iter_head:VideoKernelIterHead': 'VideoKernelIterHead',
    'knet.det.kernel_head:ConvKernelHead': 'ConvKernelHead',
    'knet.det.mask_hungarian_assigner:MaskHungarianAssigner': 'MaskHungarianAssigner',
    'knet.det.mask_pseudo_sampler:MaskPseudoSampler': 'MaskPseudoSampler',
    'knet_vis.tracker.kernel_head:ConvKernelHeadVideo': 'ConvKernelHeadVideo',
    'knet_vis.tracker.kernel_update_head:KernelUpdateHeadVideo': 'KernelUpdateHeadVideo',
    'knet_vis.tracker.kernel_iter_head:KernelIterHeadVideo': 'KernelIterHeadVideo',
    'knet_vis.tracker.kernel_frame_iter_head:KernelFrameIterHeadVideo': 'KernelFrameIterHeadVideo',
    'knet_vis.tracker.mask_hungarian_assigner:MaskHungarianAssignerVideo': 'MaskHungarianAssignerVideo',
    'knet.video.qdtrack.trackers.quasi_dense_embed_tracker:QuasiDenseEmbedTracker': 'QuasiDenseEmbedTracker',
    'knet.cross_entropy_loss:CrossEntropyLoss': 'losses.CrossEntropyLoss',
    'knet.video.track_heads:QuasiDenseMaskEmbedHeadGTMask': 'QuasiDenseMaskEmbedHeadGTMask',
}


# ---- shipped configs: a 25-line reader of the `_base_` inheritance (what mmcv's Config.fromfile does for plain dict configs)
def _merge(base, new):
    out = copy.deepcopy(base)
    for k, v in new.items():
        if isinstance(v, dict) and isinstance(out.get(k), dict) and not v.get('_delete_', False):
            out[k] = _merge(out[k], v)
        else:
            out[k] = {a: b for a, b in v.items() if a != '_delete_'} if isinstance(v, dict) else copy.deepcopy(v)
    return out


def _load(path):
    ns = {}
    exec(compile(open(path).read(), path, 'exec'), ns)
    cfg = {k: v for k, v in ns.items() if not k.startswith('__') and isinstance(v, (dict, list, tuple, str, int, float, bool, type(None)))}
    bases = cfg.pop('_base_', [])
    out = {}
    for b in ([bases] if isinstance(bases, str) else bases):
        out = _merge(out, _load(os.path.normpath(os.path.join(os.path.dirname(path), b))))
    return _merge(out, cfg)


def _encode(v):
    if isinstance(v, tuple):
        return {'__tuple__': [_encode(a) for a in v]}
    if isinstance(v, list):
        return [_encode(a) for a in v]
    if isinstance(v, dict):
        return {k: _encode(a) for k, a in v.items()}
    assert v is None or isinstance(v, (str, int, float, bool)), type(v)
    return v


def shipped_configs():
    root = os.path.join(REF, 'configs')
    out = {}
    for d, _, fs in os.walk(root):
        if '_base_' in d or d.endswith('/common'):
            continue
        for f in sorted(fs):
            if not f.endswith('.py'):
                continue
            path = os.path.join(d, f)
            try:
                model = _load(path).get('model')
            except FileNotFoundError as e:        # two shipped configs name `_base_` files the reference tree does not contain
                out[os.path.relpath(path, root)] = {'skip': 'broken in the reference itself: missing ' + os.path.relpath(e.filename, REF)}
                continue
            out[os.path.relpath(path, root)] = ({'model': _encode({k: model[k] for k in MODEL_PARTS if k in model})} if model
                                                else {'skip': 'not a model config'})
    return dict(sorted(out.items()))


# ---- the reference's method signatures
def api_surface():
    sys.path.insert(0, os.path.join(HERE, 'standins'))
    sys.path.insert(1, REF)
    out = {}
    # QuasiDenseEmbedTracker last: its loader replaces the `knet` package entries in sys.modules
    for key in sorted(PAIRS, key=lambda k: ('QuasiDenseEmbedTracker' in k) + 2 * ('QuasiDenseMaskEmbedHeadGTMask' in k)):
        mod, cls = key.split(':')
        try:
            if cls == 'QuasiDenseEmbedTracker':      # its package __init__ needs cv2: loaded by path, as the golden generator does
                sys.path.insert(0, ROOT)
                from oracle.gen_golden_tracker import load_reference_tracker
                c = load_reference_tracker()
            elif cls == 'QuasiDenseMaskEmbedHeadGTMask':   # knet/video/track_heads.py also holds RoI-based heads: loaded by path with name shims
                sys.path.insert(0, ROOT)
                from oracle.gen_golden_tracker import load_reference_embed_head
                c = load_reference_embed_head()
            else:
                c = getattr(importlib.import_module(mod), cls)
        except Exception as e:            # a module the stand-ins cannot carry
            out[key] = {'__error__': type(e).__name__ + ': ' + str(e)[:200]}
            continue
        ms = {}
        for name, fn in vars(c).items():
            if callable(fn) and (not name.startswith('_') or name in ('__init__', '_get_target_single', '_decode_init_proposals',
                                                                     '_mask_forward', '_mask_forward_train')):
                try:
                    ps = inspect.signature(fn).parameters.values()
                except (TypeError, ValueError):
                    continue
                ms[name] = [[p.name, p.default is not inspect._empty, p.kind.name] for p in ps]
        out[key] = dict(sorted(ms.items()))
    return dict(sorted(out.items()))


def _write(name, obj):
    with open(os.path.join(OUT, name), 'w') as f:
        json.dump(obj, f, indent=1)
        f.write('\n')


if __name__ == '__main__':
    if not REF or not os.path.isdir(os.path.join(REF, 'knet')):
        raise SystemExit('set VKN_REFERENCE to the reference checkout')
    os.makedirs(OUT, exist_ok=True)
    _write('shipped_configs.json', shipped_configs())
    _write('reference_api_surface.json', api_surface())
