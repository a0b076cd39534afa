"""Shared test helpers: golden loading, formula weights/inputs, oracle runs.  Imports oracle/ (allowed in tests/)."""
import os

import numpy as np
import torch

from oracle import synth
from oracle.knet_oracle import HeadCfg, head_param_shapes, iter_head_mask_preds

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASE_FIELDS = ('C', 'heads', 'ffn', 'ncls', 'n_thing', 'n_stuff', 'S', 'up', 'nprop', 'N', 'H', 'W', 'B', 'seed', 'video')


def load_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))
    case = dict(zip(CASE_FIELDS, (int(v) for v in g['case'])))
    if 'plink' in g:   # the "update" video heads (previous_link / previous_type of the swin configs)
        case['plink'], case['ptype'] = (str(g['plink']) or None), str(g['ptype'])   # ('' = no previous_link, a non-'ffn' tracking link)
    return g, case


def cfg_of(case) -> HeadCfg:
    return HeadCfg(num_stages=case['S'], in_channels=case['C'], num_heads=case['heads'], num_classes=case['ncls'],
                   mask_upsample_stride=case['up'], feat_channels=case['C'],
                   previous_type=case.get('ptype', 'ffn') if case['video'] else '', previous_link=case.get('plink') or '',
                   extra=dict(feedforward_channels=case['ffn']))


def make_case(case, dtype=torch.float32):
    """(cfg, state_dict, x, proposal_feats, mask_preds, previous_obj_feats|None) regenerated from the hash formulas."""
    cfg = cfg_of(case)
    shapes = head_param_shapes(cfg)
    sd = {k: torch.from_numpy(v).to(dtype) for k, v in synth.state_dict_like(shapes, case['seed']).items()}
    x, pf, mp = (torch.from_numpy(a).to(dtype) for a in
                 synth.head_inputs(case['B'], case['N'], case['C'], case['H'], case['W'], case['seed']))
    prev = None
    if case['video']:
        prev = torch.from_numpy(synth.normalish((case['B'], case['N'], case['C'], 1, 1), 99 + case['seed'], 1.0)).to(dtype)
    return cfg, sd, x, pf, mp, prev


def run_oracle(case, dtype=torch.float32, traces=None):
    cfg, sd, x, pf, mp, prev = make_case(case, dtype)
    with torch.no_grad():
        return iter_head_mask_preds(sd, x, pf, mp, cfg, previous_obj_feats=prev, traces=traces)


def maxabs(a, b):
    a = a.detach().cpu().double().numpy() if torch.is_tensor(a) else np.asarray(a, dtype=np.float64)
    b = b.detach().cpu().double().numpy() if torch.is_tensor(b) else np.asarray(b, dtype=np.float64)
    return float(np.max(np.abs(a - b))) if a.size else 0.0


INIT_FIELDS = ('C', 'nprop', 'ncls', 'n_thing', 'H', 'W', 'B', 'seed', 'sem', 'cat')


def load_init_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))
    return g, dict(zip(INIT_FIELDS, (int(v) for v in g['case'])))


def make_init_case(case):
    """(loc, sem|None, init_w, seg_w|None, seg_b|None) of a kernel-initialisation golden, from the hash formulas
    (same recipe as oracle/gen_golden.py:init_inputs)."""
    B, C, H, W, seed = case['B'], case['C'], case['H'], case['W'], case['seed']
    loc = torch.from_numpy(synth.normalish((B, C, H, W), 31 + 7 * seed, 1.0))
    sem = torch.from_numpy(synth.normalish((B, C, H, W), 32 + 7 * seed, 1.0)) if case['sem'] else None
    shapes = {'init_kernels.weight': (case['nprop'], C, 1, 1)}
    if case['sem']:
        shapes['conv_seg.weight'] = (case['ncls'], C, 1, 1)
        shapes['conv_seg.bias'] = (case['ncls'],)
    sd = {k: torch.from_numpy(v) for k, v in synth.state_dict_like(shapes, seed).items()}
    return loc, sem, sd['init_kernels.weight'], sd.get('conv_seg.weight'), sd.get('conv_seg.bias')


PAN_FIELDS = ('B', 'N', 'Np', 'T', 'ncls', 'Hm', 'Wm', 'up', 'Hb', 'Wb', 'h', 'w', 'Ho', 'Wo', 'seed')
PAN_CFG = dict(instance_score_thr=0.25, overlap_thr=0.6)   # test_cfg.merge_stuff_thing of the shipped configs


def load_pan_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))
    return g, dict(zip(PAN_FIELDS, (int(v) for v in g['case'])))


def make_pan_case(case):
    cls, logits = synth.panoptic_inputs(case['B'], case['N'], case['Np'], case['ncls'], case['Hm'], case['Wm'], case['seed'])
    meta = dict(img_shape=(case['h'], case['w'], 3), batch_input_shape=(case['Hb'], case['Wb']), ori_shape=(case['Ho'], case['Wo'], 3))
    return torch.from_numpy(cls), torch.from_numpy(logits), meta


def run_pan_oracle(case, b):
    from oracle.knet_oracle import panoptic_joint
    cls, logits, meta = make_pan_case(case)
    with torch.no_grad():
        return panoptic_joint(cls[b], logits[b], case['Np'], case['T'], case['Np'], PAN_CFG['instance_score_thr'],
                              PAN_CFG['overlap_thr'], meta, upsample_stride=case['up'])


def assert_pan_matches_oracle(seg, info, nseg, r, want_seg=None):
    """One frame of the joint panoptic merge (seg [Ho, Wo], info [K, 6], nseg) against an oracle.panoptic_joint result `r`: selection
    (rows / labels / score bits) and segment decisions exact; pixel counts and the map (`want_seg`, default the oracle's own) exact
    except where the arg-max is decided by < 1e-6 (fp32 resampling noise)."""
    assert int(nseg) == len(r['segments_info'])
    assert np.array_equal(info[:, 0], r['rows'].numpy()) and np.array_equal(info[:, 1], r['total_labels'].numpy())
    assert np.array_equal(info[:, 5].view(np.float32), r['total_scores'].numpy())       # score bits
    assert np.array_equal(info[:, 2], r['seg_of'].numpy())                              # accept / reject + ids
    near = (r['margin'].numpy() < 1e-6)
    assert float(near.mean()) < 2e-3
    n_near = int(near.sum())
    assert np.abs(info[:, 3] - r['area'].numpy()).sum() <= 2 * n_near                   # pixels won
    near_half = int(((r['total_masks'] - 0.5).abs() < 1e-6).sum())
    assert np.abs(info[:, 4] - r['orig'].numpy()).sum() <= near_half                    # pixels with prob >= 0.5
    diff = seg != (r['panoptic_seg'].numpy() if want_seg is None else want_seg)
    assert not (diff & ~near).any()
    assert int(diff.sum()) <= n_near


def pan_info_rows(segments_info):
    """segments_info (list of dicts) -> the golden's [id, isthing, category_id, instance_id|-1, score|nan, area|-1] rows."""
    return np.array([[s['id'], int(s['isthing']), s['category_id'], s.get('instance_id', -1), s.get('score', float('nan')),
                      s.get('area', -1)] for s in segments_info], dtype=np.float64).reshape(-1, 6)


MERGE_TF = ('merge_tf_edges', 'merge_tf_thr', 'merge_tf_dupstuff', 'merge_tf_video', 'merge_tf_empty_things', 'merge_tf_empty_stuff',
            'merge_tf_empty_below')


def load_merge_tf(name):
    """A thing-first merge fixture -> (golden, head-level inputs rebuilt from its parameters (numpy), merge thresholds)."""
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))
    thr = dict(instance_score_thr=float(g['instance_score_thr']), iou_thr=float(g['iou_thr']), stuff_max_area=int(g['stuff_max_area']))
    return g, synth.merge_tf_inputs(g), thr


def merge_tf_oracle(a, thr):
    """oracle.thing_first_merge on head-level inputs `a` -> (its ABI-level arguments, its result)."""
    from oracle.knet_oracle import thing_first_merge, thing_first_merge_args
    args = thing_first_merge_args(a['thing_masks'], a['thing_labels'], a['thing_scores'], a['stuff_masks'], a['stuff_labels'],
                                  a['stuff_scores'])
    return args, thing_first_merge(**args, **thr)


ASSIGN_FIELDS = ('N', 'G', 'ncls', 'H', 'W', 'seed')


def load_assign_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, name + '.npz'), allow_pickle=False))
    return g, dict(zip(ASSIGN_FIELDS, (int(v) for v in g['case'])))


def make_assign_case(case):
    return tuple(torch.from_numpy(a) for a in synth.assign_inputs(case['N'], case['G'], case['ncls'], case['H'], case['W'], case['seed']))


# ---- measured parity margins: the free-running tests record WHAT they measured, not only pass / fail; the file is
# rewritten after every record so that a partial run still leaves evidence.  Copied to profiles/r04_parity_margins.json by hand.
_MARGINS = {}


def record_margins(test_id, values):
    import json
    _MARGINS[test_id] = {k: (float(v) if isinstance(v, (int, float, np.floating, np.integer)) else v) for k, v in values.items()}
    path = os.environ.get('VKN_MARGINS_JSON', os.path.join(ROOT, 'gpurun_out', 'parity_margins.json'))
    try:
        os.makedirs(os.path.dirname(path), exist_ok=True)
        old = {}
        if os.path.exists(path):
            with open(path) as f:
                old = json.load(f)
        old.update(_MARGINS)
        with open(path, 'w') as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass
    print(f'[margins] {test_id}: ' + ', '.join(f'{k}={v:.3g}' if isinstance(v, float) else f'{k}={v}' for k, v in _MARGINS[test_id].items()))


def lowres_tail_reference(low, bank, tgt_row, rowk, S, w=(1.0, 4.0, 0.1), g=(1.0, 1.0, 1.0), eps=1e-3):
    """float64 reference of the loss tail on LOW-RES logits, autograd for the gradient (on low's device).  low [B, Ns, h, w]; bank
    [G, S h, S w] target masks; rowk [B Ns] = positive index k of a row or -1; tgt_row [B Ns] = its bank row.  The reference's chain:
    F.interpolate(scale_factor=S, bilinear, align_corners=False) (knet/det/kernel_iter_head.py:122-130), then `loss`
    (knet/det/kernel_update_head.py:313-342) with mmdet's losses restated:
      loss_mask = w[0] mean BCE-with-logits over the K positive rows (CrossEntropyLoss(use_sigmoid=True))
      loss_dice = w[1] mean_k (1 - 2 a / (b + c)),  a = sum p t, b = sum p^2 + eps, c = sum t^2 + eps   (DiceLoss, sigmoid activated)
      loss_rank = w[2] mean over B S h S w of the softmax CE over the Ns rows, target -1 ignored (CrossEntropyLoss(use_sigmoid=False),
                  ignore_index=-1): the target of a pixel is the LAST positive row (in row order) whose mask covers it (:336-340).
    -> dict(rows [K, 4] = per positive row (sum BCE, a, sum p^2, sum t^2), lse / top [B, P], rank_sum (sum of the CE), dice_a / dice_bc
    [K] (what the backward kernels take), losses (3), grad [B, Ns, h, w] = d(sum_i g[i] loss_i) / d low)."""
    import torch.nn.functional as F
    B, Ns = low.shape[:2]
    lo = low.detach().double().requires_grad_(True)
    up = F.interpolate(lo, scale_factor=S, mode='bilinear', align_corners=False)
    P = up.shape[2] * up.shape[3]
    z = up.reshape(B, Ns, P)
    rowk, tgt_row = rowk.long().to(low.device), tgt_row.long().to(low.device)
    pos = torch.nonzero(rowk >= 0).flatten()
    pos = pos[torch.argsort(rowk[pos])]                               # the row of positive k, k = 0 .. K-1
    K = int(pos.numel())
    tbank = bank.reshape(bank.shape[0], P).to(low.device)
    pred = z.reshape(B * Ns, P)[pos]
    tgt = tbank[tgt_row[pos]].double()
    bce = F.binary_cross_entropy_with_logits(pred, tgt, reduction='none').sum(1)
    p = pred.sigmoid()
    a, b, c = (p * tgt).sum(1), (p * p).sum(1), (tgt * tgt).sum(1)
    top = torch.full((B, P), -1, dtype=torch.long, device=low.device)
    for r in sorted(pos.tolist()):                                    # positive rows in order: a later row overwrites an earlier one
        top[r // Ns][tbank[tgt_row[r]] != 0] = r % Ns
    ce = F.cross_entropy(z, top, ignore_index=-1, reduction='none')    # [B, P], 0 where ignored
    losses = (bce.sum() / (K * P), (1 - 2 * a / ((b + eps) + (c + eps))).mean(), ce.sum() / (B * P))
    total = sum(gi * wi * li for gi, wi, li in zip(g, w, losses))
    total.backward()
    return dict(rows=torch.stack([bce, a, b, c], 1).detach(), lse=torch.logsumexp(z, 1).detach(), top=top.int(),
                rank_sum=float(ce.detach().sum()), dice_a=a.detach(), dice_bc=((b + eps) + (c + eps)).detach(),
                losses=tuple(float(v.detach()) for v in losses), grad=lo.grad)


def run_and_kernels(fn):
    """fn()'s result and the names of the device kernels it launched (torch.profiler records the library's launches as well)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    return out, {e.name for e in prof.events()}
