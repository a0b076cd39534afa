#!/usr/bin/env python
"""Generate tests/golden/gt_prep_*.npz from the REFERENCE ITSELF (needs the reference checkout; CPU only; never imported by a test).

    VKN_REFERENCE=<reference checkout> python tools/gen_golden_gt_prep.py

The reference's files are loaded UNMODIFIED by path through the plumbing stand-ins of oracle/standins (names only, no arithmetic):
  knet/det/utils.py                                          sem2ins_masks, sem2ins_masks_cityscapes, sem2ins_masks_kitti_step
  knet/video/knet_quansi_dense_embed_fc_joint_train.py       the unbound `preprocess_gt_masks` on a minimal stand-in `self` and a
                                                             bitmap-mask stand-in (.masks, .height, .width + `to_tensor`), and the
                                                             `gt_pids` lines of `forward_train`, executed from the file as they stand
The fixtures hold inputs and outputs only:
  gt_prep_<case>.npz   pad, stride, dataset + class counts, per image: masks{b} uint8, img_shape{b}; sem (the map BEFORE the call);
                       out_masks{b}, out_sem_cls{b}, out_sem_seg{b}: what the reference returned
  gt_prep_tables.npz   per variant the labels the three functions give a map that holds every value 0..255 (-1: not listed)
  gt_prep_match.npz    key / reference id lists and the gt_pids of each
The maps of the cases hold classes of their dataset only: on a uint8 map the reference adds the label shift in uint8, so a class
>= 256 - shift (none exists in a shipped dataset) would come back wrapped; the tables are taken from an int64 map.
"""
import importlib.util
import os
import sys
import textwrap
import types

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
REF = os.environ.get('VKN_REFERENCE')
if not REF:
    raise SystemExit('set VKN_REFERENCE to the reference checkout')
sys.path.insert(0, os.path.join(ROOT, 'oracle', 'standins'))
sys.path.insert(1, REF)

import numpy as np  # noqa: E402
import torch  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden')
DETECTOR = 'knet/video/knet_quansi_dense_embed_fc_joint_train.py'


def _by_path(name, rel):
    spec = importlib.util.spec_from_file_location(name, os.path.join(REF, rel))
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


def load_reference():
    """(utils module, detector class).  Whatever the detector's import lines name beyond the stand-ins becomes an empty placeholder: the
    method under test touches none of it."""
    for pkg in ('knet', 'knet.det', 'knet.video', 'knet.video.qdtrack'):
        m = types.ModuleType(pkg)
        m.__path__ = []
        sys.modules.setdefault(pkg, m)
    utils = _by_path('knet.det.utils', 'knet/det/utils.py')

    class _Registry:
        def register_module(self, *a, **k):
            return lambda cls: cls

    def shim(module, **names):
        if module not in sys.modules:
            try:
                importlib.import_module(module)
            except ImportError:
                sys.modules[module] = types.ModuleType(module)
        for k, v in names.items():
            if not hasattr(sys.modules[module], k):
                setattr(sys.modules[module], k, v)
    nothing = lambda *a, **k: None                                           # noqa: E731
    shim('mmcv.cnn', ConvModule=object, bias_init_with_prob=nothing, build_activation_layer=nothing, build_norm_layer=nothing)
    shim('mmdet.models.builder', DETECTORS=_Registry(), build_head=nothing, build_neck=nothing, build_backbone=nothing,
         build_roi_extractor=nothing)
    shim('mmdet.models.detectors', BaseDetector=torch.nn.Module)
    shim('mmdet.core', build_assigner=nothing, build_sampler=nothing)
    shim('knet.video.qdtrack.builder', build_tracker=nothing)
    shim('unitrack.mask', tensor_mask2box=nothing)
    det = _by_path('knet.video._gt_prep_detector', DETECTOR)
    return utils, det.VideoKNetQuansiEmbedFCJointTrain


class Bitmap:
    """the three attributes `preprocess_gt_masks` reads of mmdet's BitmapMasks, and its `to_tensor`"""

    def __init__(self, masks):
        self.masks, self.height, self.width = masks, int(masks.shape[1]), int(masks.shape[2])

    def to_tensor(self, dtype, device):
        return torch.tensor(self.masks, dtype=dtype, device=device)


def blobs(rng, G, H, W, value=1):
    m = np.zeros((G, H, W), np.uint8)
    for g in range(G):
        y0, x0 = rng.integers(0, max(H - 3, 1)), rng.integers(0, max(W - 3, 1))
        m[g, y0:y0 + rng.integers(2, H), x0:x0 + rng.integers(2, W)] = value
    m[:, -1, :] |= (rng.random((G, W)) > 0.5).astype(np.uint8) * value      # the last row and column are busy: the pad edge cuts here
    m[:, :, -1] |= (rng.random((G, H)) > 0.5).astype(np.uint8) * value
    return m


def sem_map(rng, B, H, W, classes, block=5):
    """piecewise-constant maps over `classes`, with single pixels of other classes sprinkled in"""
    classes = np.asarray(classes)
    coarse = classes[rng.integers(0, len(classes), (B, (H + block - 1) // block, (W + block - 1) // block))]
    sem = np.repeat(np.repeat(coarse, block, 1), block, 2)[:, :H, :W].copy()
    noise = rng.random((B, H, W)) > 0.93
    sem[noise] = classes[rng.integers(0, len(classes), int(noise.sum()))]
    return sem


def cases():
    rng = np.random.default_rng(20240607)
    out = {}
    # Cityscapes form: stride 4, pad 32 x 72 (aW = 18), masks smaller than the pad, img_shape cutting a 2 x 2 centre
    sem = sem_map(rng, 2, 32, 72, list(range(19)) + [255]).astype(np.uint8)
    out['city_s4'] = dict(dataset='cityscapes', stride=4, pad=(32, 72), T=8, S=11, things=-1,
                          masks=[blobs(rng, 3, 30, 61), blobs(rng, 2, 32, 72)], img_shape=[(29, 59), (32, 72)], sem=sem)
    # VIP-Seg shares the Cityscapes function: 58 things behind 66 stuff classes
    sem = sem_map(rng, 1, 32, 72, [0, 3, 65, 66, 70, 123, 255]).astype(np.uint8)
    out['vipseg_s4'] = dict(dataset='vipseg', stride=4, pad=(32, 72), T=58, S=66, things=-1,
                            masks=[blobs(rng, 4, 32, 72)], img_shape=[(32, 70)], sem=sem)
    # KITTI-STEP form: stride 2, pad 34 x 70 (odd aH, aW), int64 map, three mask sizes, an image without things, one all ignore
    sem = sem_map(rng, 3, 34, 70, [0, 1, 5, 10, 11, 12, 13, 14, 18, 255]).astype(np.int64)
    sem[2] = 255
    out['kitti_s2'] = dict(dataset='kitti_step', stride=2, pad=(34, 70), T=2, S=17, things=-1,
                           masks=[blobs(rng, 2, 33, 69), np.zeros((0, 34, 70), np.uint8), blobs(rng, 3, 20, 41)],
                           img_shape=[(33, 69), (34, 70), (20, 41)], sem=sem)
    # generic (COCO) form: stride 8, pad 48 x 80, byte masks holding 255, class 0 is the special thing label
    sem = sem_map(rng, 2, 48, 80, [0, 1, 2, 40, 53, 255]).astype(np.uint8)
    out['generic_s8'] = dict(dataset='generic', stride=8, pad=(48, 80), T=80, S=53, things=0,
                             masks=[blobs(rng, 3, 48, 80, value=255), blobs(rng, 1, 41, 77)], img_shape=[(48, 80), (41, 77)], sem=sem)
    # the identity: stride 1, pad 9 x 13; the special thing label is 3 here, so class 0 is listed
    sem = sem_map(rng, 1, 9, 13, [0, 3, 7, 255], block=3).astype(np.uint8)
    out['generic_s1'] = dict(dataset='generic', stride=1, pad=(9, 13), T=4, S=9, things=3,
                             masks=[blobs(rng, 2, 8, 11)], img_shape=[(8, 11)], sem=sem)
    # no semantic map at all
    out['nosem_s2'] = dict(dataset='generic', stride=2, pad=(34, 70), T=80, S=53, things=0,
                           masks=[blobs(rng, 2, 34, 70), blobs(rng, 1, 30, 66)], img_shape=[(34, 70), (30, 66)], sem=None)
    return out


def stand_in_self(c):
    return types.SimpleNamespace(mask_assign_stride=c['stride'], ignore_label=255, num_thing_classes=c['T'], num_stuff_classes=c['S'],
                                 cityscapes=c['dataset'] == 'cityscapes', vipseg=c['dataset'] == 'vipseg',
                                 kitti_step=c['dataset'] == 'kitti_step', thing_label_in_seg=c['things'])


def gt_pids_lines():
    """the `gt_match_indices` loop of `forward_train`, cut out of the reference's file at run time"""
    with open(os.path.join(REF, DETECTOR)) as f:
        lines = f.read().split('\n')
    a = next(i for i, l in enumerate(lines) if l.strip() == 'gt_pids_list = []')
    b = next(i for i in range(a, len(lines)) if lines[i].strip() == 'gt_match_indices = gt_pids_list')
    return textwrap.dedent('\n'.join(lines[a:b + 1]))


def main():
    utils, Detector = load_reference()
    os.makedirs(GOLDEN, exist_ok=True)
    for name, c in cases().items():
        B = len(c['masks'])
        metas = [dict(batch_input_shape=c['pad'], img_shape=c['img_shape'][b] + (3,)) for b in range(B)]
        sem = None if c['sem'] is None else torch.from_numpy(c['sem'].copy())[:, None]
        labels = [torch.zeros(m.shape[0], dtype=torch.int64) for m in c['masks']]
        masks, sem_cls, sem_seg = Detector.preprocess_gt_masks(stand_in_self(c), metas, [Bitmap(m) for m in c['masks']], labels, sem)
        out = dict(dataset=np.array(c['dataset']), stride=np.int64(c['stride']), pad=np.array(c['pad']), T=np.int64(c['T']),
                   S=np.int64(c['S']), things=np.int64(c['things']), B=np.int64(B))
        if c['sem'] is not None:
            out['sem'] = c['sem']
        for b in range(B):
            out[f'masks{b}'], out[f'img_shape{b}'] = c['masks'][b], np.array(c['img_shape'][b])
            out[f'out_masks{b}'] = masks[b].numpy()
            if sem_cls is not None:
                out[f'out_sem_cls{b}'], out[f'out_sem_seg{b}'] = sem_cls[b].numpy(), sem_seg[b].numpy()
        np.savez_compressed(os.path.join(GOLDEN, f'gt_prep_{name}.npz'), **out)
        print(name, [tuple(m.shape) for m in masks], None if sem_cls is None else [s.tolist() for s in sem_cls])

    every = torch.arange(256, dtype=torch.int64).reshape(1, 16, 16)
    tables = {}
    for key, fn, kw in (('generic_t80_thing0', utils.sem2ins_masks, dict(label_shift=80, thing_label_in_seg=0)),
                        ('generic_t4_thing3', utils.sem2ins_masks, dict(label_shift=4, thing_label_in_seg=3)),
                        ('cityscapes_t8_s11', utils.sem2ins_masks_cityscapes, dict(label_shift=8, thing_label_in_seg=list(range(11, 19)))),
                        ('vipseg_t58_s66', utils.sem2ins_masks_cityscapes, dict(label_shift=58, thing_label_in_seg=list(range(66, 124)))),
                        ('kitti_step', utils.sem2ins_masks_kitti_step, dict(label_shift=2, thing_label_in_seg=(11, 13)))):
        labels, ins = fn(every.clone(), ignore_label=255, **kw)
        listed = [int(every.reshape(-1)[m.reshape(-1) > 0][0]) for m in ins]          # the class each returned mask selects
        table = np.full(256, -1, np.int64)
        table[listed] = labels.numpy()
        assert listed == sorted(listed)
        tables[key] = table
    np.savez_compressed(os.path.join(GOLDEN, 'gt_prep_tables.npz'), **tables)

    rng = np.random.default_rng(7)
    src = gt_pids_lines()
    assert 'gt_pids' in src and 'ref_ids.index' in src
    match = {}
    lists = [([5, 7, 9, 5], [9, 5, 5]), ([], [1, 2]), ([3, 4], []), ([11, 12, 13], [13, 12, 11, 12]),
             (rng.permutation(2000)[:1024].tolist(), rng.permutation(2000)[:1024].tolist())]
    ns = dict(torch=torch, img=torch.zeros(1), gt_instance_ids=[torch.tensor(k, dtype=torch.int64) for k, _ in lists],
              ref_gt_instance_id_list=[torch.tensor(r, dtype=torch.int64) for _, r in lists])
    exec(compile(src, DETECTOR, 'exec'), ns)
    for i, ((k, r), got) in enumerate(zip(lists, ns['gt_match_indices'])):
        match[f'key{i}'], match[f'ref{i}'] = np.array(k, np.int64), np.array(r, np.int64)
        match[f'pids{i}'] = got.numpy().astype(np.int64).reshape(-1)
    match['n'] = np.int64(len(lists))
    np.savez_compressed(os.path.join(GOLDEN, 'gt_prep_match.npz'), **match)
    print('match', [match[f'pids{i}'][:6].tolist() for i in range(len(lists))])


if __name__ == '__main__':
    main()
