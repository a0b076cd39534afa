"""References of the fused tracking loss (include/vkn_track_train.h), shared by tests/test_track_loss_refs.py (CPU) and
tests/test_gpu_track_loss.py: a float64 restatement of the header's formulas on given fp32 inputs (`reference`), the package's own
fp32 host path on the same inputs (`host_path`), the inputs themselves (the `qd_embed_head` goldens in their compact and full-row
form, hash-formula cases at the decision edges) and the bound the gradients are held to.  No tests in here."""
import functools
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from oracle import synth  # noqa: E402
from oracle.embed_cases import EMBED_CASES, _Sampling, embed_case_inputs  # noqa: E402

GOLDEN = os.path.join(ROOT, 'tests', 'golden', 'qd_embed_head.npz')
GOUTS = ((1.0, 1.0), (0.5, -2.0), (1.0, 0.0), (0.0, 1.0))
ULP = 2.0 ** -23
MIN_GAP = 1e-4            # cost gap at the mining cut below which a kept mask is not compared (fp32 vs float64 selection)


class Case:
    """One input of the loss: key, ref fp32 [B,N,E]; key_gt, ref_gt int64 [B,N]; matches: per image int64 [G]; head: the config of the
    `QuasiDenseMaskEmbedHeadGTMask` whose losses apply."""

    def __init__(self, name, key, ref, key_gt, ref_gt, matches, head):
        self.name, self.key, self.ref, self.key_gt, self.ref_gt, self.matches, self.head = name, key, ref, key_gt, ref_gt, matches, head

    @property
    def shape(self):
        return tuple(self.key.shape)


def loss_cfg(head_cfg):
    """(softmax_temp, has_aux, w_track, w_aux, neg_pos_ub, pos_margin, neg_margin) of a head config, defaults as the classes'."""
    lt = head_cfg.get('loss_track', dict(loss_weight=0.25))
    la = head_cfg.get('loss_track_aux', dict(loss_weight=1.0, hard_mining=True))
    la = dict(la) if la is not None else None
    if la is not None and 'sample_ratio' in la:
        raise ValueError('write neg_pos_ub / pos_margin / neg_margin, as the shipped configs do')
    return dict(softmax_temp=head_cfg.get('softmax_temp', -1), has_aux=la is not None, w_track=lt.get('loss_weight', 1.0),
                w_aux=la.get('loss_weight', 1.0) if la else 0.0, neg_pos_ub=la.get('neg_pos_ub', -1) if la else -1,
                pos_margin=la.get('pos_margin', -1) if la else -1, neg_margin=la.get('neg_margin', -1) if la else -1)


def _positives(gt_row):
    return torch.nonzero(gt_row > 0, as_tuple=False).squeeze(-1)


# ---------------------------------------------------------------------------------------------------- float64 restatement
def reference(case, gout=(1.0, 1.0)):
    """The header's formulas in float64 on the case's fp32 inputs -> dict(losses [2], stats [B,4], kept uint8 [B,N,N],
    d_key, d_ref float64 [B,N,E] for `gout`, targets / weights per image, cut_gap / cut_cost per image (None without mining))."""
    c = loss_cfg(case.head)
    B, N, E = case.shape
    key = case.key.double().requires_grad_(True)
    ref = case.ref.double().requires_grad_(True)
    kept_all = np.zeros((B, N, N), dtype=np.uint8)
    stats = np.zeros((B, 4), dtype=np.int32)
    loss_track, loss_aux = key.new_zeros(()), key.new_zeros(())
    targets, weights, gaps, cuts = [], [], [], []
    for b in range(B):
        kp, rp = _positives(case.key_gt[b]), _positives(case.ref_gt[b])
        k, r = key[b, kp], ref[b, rp]
        t = case.matches[b][case.key_gt[b, kp] - 1].view(-1, 1) == (case.ref_gt[b, rp] - 1).view(1, -1)
        w = t.any(dim=1)
        targets.append(t.int().numpy()); weights.append(w.float().numpy())
        cos = (k / k.norm(dim=1, keepdim=True).clamp_min(1e-12)) @ (r / r.norm(dim=1, keepdim=True).clamp_min(1e-12)).t()
        dists = cos / c['softmax_temp'] if c['softmax_temp'] > 0 else k @ r.t()
        ninf = dists.new_full((), float('-inf'))
        both = torch.logsumexp(torch.where(~t, dists, ninf), dim=1) + torch.logsumexp(torch.where(t, -dists, ninf), dim=1)
        rows = torch.where(torch.isfinite(both), torch.logaddexp(both, torch.zeros_like(both)), torch.zeros_like(both))
        loss_track = loss_track + c['w_track'] * (rows * w.double()).sum() / w.double().sum()
        num_pos = int(t.sum())
        num_neg = t.numel() - num_pos
        kept_neg, gap, cut = 0, None, None
        if c['has_aux']:
            margin = torch.where(t, torch.full_like(cos, max(c['pos_margin'], 0.0)), torch.full_like(cos, max(c['neg_margin'], 0.0)))
            pred = (cos - margin).clamp(0, 1)
            keep = torch.ones_like(t)
            kept_neg = num_neg
            if c['neg_pos_ub'] > 0 and num_neg / (num_pos + 1) > c['neg_pos_ub']:
                kept_neg = num_pos * c['neg_pos_ub']
                cost = (pred.detach() ** 2).reshape(-1).numpy()
                neg = np.flatnonzero(~t.reshape(-1).numpy())
                order = neg[np.lexsort((neg, -cost[neg]))]         # largest cost first, ties to the lowest row-major index
                keep = t.clone().reshape(-1)
                keep[torch.from_numpy(order[:kept_neg])] = True
                keep = keep.reshape(t.shape)
                if 0 < kept_neg < len(order):
                    cut = float(cost[order[kept_neg - 1]])
                    gap = cut - float(cost[order[kept_neg]])
            loss_aux = loss_aux + c['w_aux'] * ((pred - t.double()) ** 2 * keep.double()).sum() / keep.double().sum()
            kept_all[b][np.ix_(kp.numpy(), rp.numpy())] = keep.numpy().astype(np.uint8)
        gaps.append(gap); cuts.append(cut)
        stats[b] = (len(kp), len(rp), num_pos, kept_neg if c['has_aux'] else 0)
    loss_track, loss_aux = loss_track / B, loss_aux / B
    total = gout[0] * loss_track + (gout[1] * loss_aux if c['has_aux'] else 0.0)
    d_key, d_ref = torch.autograd.grad(total, (key, ref), allow_unused=True)
    zero = torch.zeros_like(key)
    return dict(losses=np.array([float(loss_track.detach()), float(loss_aux.detach())]), stats=stats, kept=kept_all,
                d_key=(d_key if d_key is not None else zero).numpy(), d_ref=(d_ref if d_ref is not None else zero).numpy(),
                targets=targets, weights=weights, cut_gap=gaps, cut_cost=cuts)


# ---------------------------------------------------------------------------------------------------- the package's host path
def build_head(vkn, head_cfg):
    return vkn.build_head(dict(head_cfg, type='QuasiDenseMaskEmbedHeadGTMask'))


def sampling(case, device='cpu'):
    """(key rows, ref rows, key / ref sampling stubs, matches) of the case on `device`: what `match` / `get_track_targets` take."""
    kidx, ridx, kres, rres = [], [], [], []
    for b in range(case.shape[0]):
        kp, rp = _positives(case.key_gt[b]), _positives(case.ref_gt[b])
        kidx.append(kp); ridx.append(rp)
        kres.append(_Sampling(len(kp), (case.key_gt[b, kp] - 1).to(device)))
        rres.append(_Sampling(len(rp), (case.ref_gt[b, rp] - 1).to(device)))
    return kidx, ridx, kres, rres, [m.to(device) for m in case.matches]


def host_path(vkn, case, gout=(1.0, 1.0), device='cpu'):
    """`loss(*match(...), *get_track_targets(...))` of the package in fp32 with autograd -> dict(losses [2] (float32 values),
    d_key, d_ref fp32 [B,N,E], kept uint8 [B,N,N]: L2Loss's final `weight > 0`, targets, weights)."""
    head = build_head(vkn, case.head)
    B, N, E = case.shape
    key = case.key.clone().to(device).requires_grad_(True)
    ref = case.ref.clone().to(device).requires_grad_(True)
    kidx, ridx, kres, rres, matches = sampling(case, device)
    ke = torch.cat([key[b, kidx[b].to(device)] for b in range(B)])
    re_ = torch.cat([ref[b, ridx[b].to(device)] for b in range(B)])
    dists, cos = head.match(ke, re_, kres, rres)
    targets, weights = head.get_track_targets(matches, kres, rres)
    kept = np.zeros((B, N, N), dtype=np.uint8)
    if head.loss_track_aux is not None:
        for b in range(B):
            _, wgt, _ = head.loss_track_aux.update_weight(cos[b].detach().clone(), targets[b].clone(), None, None)
            kept[b][np.ix_(kidx[b].numpy(), ridx[b].numpy())] = (wgt > 0).cpu().numpy().astype(np.uint8)
    losses = head.loss(dists, cos, [t.clone() for t in targets], [w.clone() for w in weights])
    lt, la = losses['loss_track'], losses.get('loss_track_aux')
    total = gout[0] * lt + (gout[1] * la if la is not None else 0.0)
    d_key, d_ref = torch.autograd.grad(total, (key, ref), allow_unused=True)
    zero = torch.zeros_like(key)
    return dict(losses=np.array([float(lt.detach()), float(la.detach()) if la is not None else 0.0], dtype=np.float32),
                d_key=(d_key if d_key is not None else zero).detach().cpu().numpy(), d_ref=(d_ref if d_ref is not None else zero).detach().cpu().numpy(),
                kept=kept, targets=[t.cpu().numpy() for t in targets], weights=[w.cpu().numpy() for w in weights])


def rel_err(got, want):
    """max-norm error relative to the reference tensor's largest magnitude; NaN must sit where the reference has it (else inf) and is
    left out of both norms"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    if not np.array_equal(nan, np.isnan(got)):
        return float('inf')
    if nan.all():
        return 0.0
    scale = float(np.abs(want[~nan]).max())
    return float(np.abs(got[~nan] - want[~nan]).max()) / (scale if scale > 0 else 1.0)


@functools.lru_cache(maxsize=None)
def grad_bounds(vkn, name, gout):
    """((bound d_key, bound d_ref), (host error d_key, d_ref), float64 reference) of a case: 8 x the error of the package's fp32 host path
    against the float64 restatement (a different summation order over up to 1024 terms), at least 4 fp32 ulps of the tensor's
    largest magnitude.  Measured on the reference arithmetic, not on the kernel."""
    case = CASES[name]()
    want, host = reference(case, gout), host_path(vkn, case, gout)
    errs = (rel_err(host['d_key'], want['d_key']), rel_err(host['d_ref'], want['d_ref']))
    return tuple(max(8.0 * e, 4.0 * ULP) for e in errs), errs, want


# ---------------------------------------------------------------------------------------------------- inputs
def golden_case(name, full_rows):
    """The `qd_embed_head` golden `name` (two images, the reference's own embeddings): compact rows zero-padded to the longer image, or
    the same rows scattered in ascending order among gt = 0 rows (non-zero embeddings) up to N = 100."""
    g = np.load(GOLDEN)
    cfg, sizes, seed = EMBED_CASES[name]
    _, _, _, kres, rres, matches = embed_case_inputs(cfg, sizes, seed)
    nk, nr = [sizes[0], sizes[1]], [sizes[1], sizes[0]]
    E = cfg['embed_channels']
    ke = torch.split(torch.from_numpy(g[name + '_key_embeds']), nk)
    re_ = torch.split(torch.from_numpy(g[name + '_ref_embeds']), nr)
    N = 100 if full_rows else max(sizes)
    key = torch.from_numpy(synth.normalish((2, N, E), 9000 + seed, 1.0)) if full_rows else torch.zeros(2, N, E)
    ref = torch.from_numpy(synth.normalish((2, N, E), 9100 + seed, 1.0)) if full_rows else torch.zeros(2, N, E)
    key_gt, ref_gt = torch.zeros(2, N, dtype=torch.int64), torch.zeros(2, N, dtype=torch.int64)
    for b in range(2):
        for emb, gt, rows, res, n, salt in ((key, key_gt, ke, kres, nk, 1), (ref, ref_gt, re_, rres, nr, 2)):
            at = torch.arange(n[b])
            if full_rows:
                at = torch.from_numpy(np.sort(np.argsort(synth.uniform((N,), 9200 + 10 * seed + 2 * b + salt))[:n[b]]).copy())
            emb[b, at] = rows[b]
            gt[b, at] = res[b].pos_assigned_gt_inds + 1
    return Case(name + ('_full' if full_rows else '_compact'), key, ref, key_gt, ref_gt, matches, cfg)


EDGE_HEAD = dict(num_convs=0, num_fcs=1, roi_feat_size=1, in_channels=16, fc_out_channels=16, embed_channels=16,
                 loss_track=dict(type='MultiPosCrossEntropyLoss', loss_weight=0.25),
                 loss_track_aux=dict(type='L2Loss', neg_pos_ub=3, pos_margin=0, neg_margin=0.1, hard_mining=True, loss_weight=1.0))


def _aux(**kw):
    return dict(EDGE_HEAD, loss_track_aux=dict(EDGE_HEAD['loss_track_aux'], **kw))


def edge_case(name, images, head=EDGE_HEAD, N=None, E=16, seed=0, scale=1.0):
    """images: per image (key instances, reference instances, match): the instance (0-based) of every positive key / reference row,
    and the partner list.  Rows without ground truth are interleaved when N exceeds the positives."""
    B = len(images)
    N = N or max(max(len(k), len(r)) for k, r, _ in images)
    key = torch.from_numpy(synth.normalish((B, N, E), 7000 + 31 * seed, scale))
    ref = torch.from_numpy(synth.normalish((B, N, E), 7001 + 31 * seed, scale))
    key_gt, ref_gt = torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N, dtype=torch.int64)
    matches = []
    for b, (kinst, rinst, match) in enumerate(images):
        for gt, inst, salt in ((key_gt, kinst, 3), (ref_gt, rinst, 4)):
            at = np.sort(np.argsort(synth.uniform((N,), 7100 + 31 * seed + 2 * b + salt))[:len(inst)]).copy()
            gt[b, torch.from_numpy(at)] = torch.tensor(inst, dtype=torch.int64) + 1
        matches.append(torch.tensor(match, dtype=torch.int64))
    return Case(name, key, ref, key_gt, ref_gt, matches, head)


def _capacity():
    n = 128                                              # every row a positive, every instance once, every second key with a partner
    match = [(3 * g + 1) % n if g % 2 == 0 else -1 for g in range(n)]
    return edge_case('capacity', [(list(range(n)), [(5 * i + 2) % n for i in range(n)], match)], N=n, E=1024, seed=9)


CASES = {
    'emb_cfg_compact': lambda: golden_case('emb_cfg', False), 'emb_cfg_full': lambda: golden_case('emb_cfg', True),
    'emb_one_compact': lambda: golden_case('emb_one', False), 'emb_one_full': lambda: golden_case('emb_one', True),
    'emb_temp_compact': lambda: golden_case('emb_temp', False), 'emb_temp_full': lambda: golden_case('emb_temp', True),
    # 2 x 3 entries, 2 positives: 4 / 3 <= 3, no mining
    'no_mining': lambda: edge_case('no_mining', [([0, 1], [1, 0, 2], [1, 0, -1])], seed=1),
    # neg_pos_ub = 3 and one positive: 6 negatives are exactly the ratio (no mining), 7 are above it (3 of them stay)
    'edge_at': lambda: edge_case('edge_at', [([0], [1, 2, 3, 4, 5, 6, 7], [1])], N=9, seed=2),
    'edge_above': lambda: edge_case('edge_above', [([0, 1], [1, 2, 3, 4], [1, -1])], N=6, seed=3),
    'edge_below': lambda: edge_case('edge_below', [([0, 1, 2], [1, 0, 3], [1, 0, -1])], N=5, seed=4),
    'ub_off': lambda: edge_case('ub_off', [(list(range(8)), [(3 * i + 1) % 9 for i in range(9)], [-1, 1, 4, -1, 7, 1, -1, 4])],
                                head=_aux(neg_pos_ub=-1), N=13, seed=5),
    'pos_margin': lambda: edge_case('pos_margin', [(list(range(7)), list(range(6)), [g if g % 2 == 0 else -1 for g in range(7)])],
                                    head=_aux(pos_margin=0.2), N=10, seed=6),
    # image 1: no key has a partner (num_pos = 0): 0 / 0 in both losses
    'no_partner': lambda: edge_case('no_partner', [([0, 1, 2, 3], [0, 1, 2], [1, 0, -1, 2]), ([0, 1, 2], [0, 1, 2, 3], [-1, -1, -1])], N=7, seed=7),
    # image 1: one reference row; key row 0 has only positives, key rows 1 and 2 have weight 0 and count as L2 negatives
    'degenerate': lambda: edge_case('degenerate', [([0, 1, 2], [1, 0, 3], [1, 0, -1]), ([0, 1, 2], [5], [5, -1, 3])], N=8, seed=8),
    'one_by_one': lambda: edge_case('one_by_one', [([0], [0], [0])], N=1, seed=10),
    'capacity': _capacity,
}
GOLDEN_CASES = [n for n in CASES if n.startswith('emb_')]
EDGE_CASES = [n for n in CASES if not n.startswith('emb_')]
MASK_CASES = [n for n in CASES if n not in ('emb_temp_compact', 'emb_temp_full')]      # cases with an auxiliary loss
