"""A/B of the tracking loss of one training step, forward + backward down to the embeddings: the host path
(`match` -> `get_track_targets` -> `loss` on the gathered positives, autograd's backward) against the fused path
(`match_loss_rows`: csrc/vkn_trackloss.hip).  B = 2 images, N = 100 rows, ~40 positives per side, E = 256, the shipped
`*_joint_train` loss configuration.  Both run in this process one after the other; per call HIP events after a warm-up.

    python tools/track_loss_ab.py [--calls 200] [--warmup 30] [--out profiles/track_loss_ab.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vkn_import  # noqa: E402
from oracle import synth  # noqa: E402
from oracle.embed_cases import EMBED_CFG, _Sampling  # noqa: E402

B, N, E, POS, G = 2, 100, 256, 40, 44


def inputs(dev):
    key = torch.from_numpy(synth.normalish((B, N, E), 501, 1.0)).to(dev)
    ref = torch.from_numpy(synth.normalish((B, N, E), 502, 1.0)).to(dev)
    key_gt, ref_gt = torch.zeros(B, N, dtype=torch.int64), torch.zeros(B, N, dtype=torch.int64)
    matches = []
    for b in range(B):
        for gt, salt in ((key_gt, 1), (ref_gt, 2)):
            rows = np.sort(np.argsort(synth.uniform((N,), 510 + 2 * b + salt))[:POS])
            inst = np.argsort(synth.uniform((G,), 520 + 2 * b + salt))[:POS]
            gt[b, torch.from_numpy(rows.copy())] = torch.from_numpy(inst.copy()) + 1
        m = torch.full((G,), -1, dtype=torch.int64)
        m[::2] = torch.arange(0, G, 2)                     # every second key instance has a partner (itself, if the reference kept it)
        matches.append(m.to(dev))
    return key, ref, key_gt.to(dev), ref_gt.to(dev), matches


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(calls):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return min(ms), statistics.median(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=30)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'track_loss_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('track_loss_ab.py measures on the GPU; there is none here')
    vkn = vkn_import.load()
    dev = 'cuda:0'
    head = vkn.build_head(dict(EMBED_CFG, type='QuasiDenseMaskEmbedHeadGTMask')).to(dev)
    key, ref, key_gt, ref_gt, matches = inputs(dev)
    key.requires_grad_(True); ref.requires_grad_(True)
    kidx = [torch.nonzero(key_gt[b] > 0).squeeze(-1) for b in range(B)]          # the sampler's work: outside the timed region
    ridx = [torch.nonzero(ref_gt[b] > 0).squeeze(-1) for b in range(B)]
    kres = [_Sampling(len(kidx[b]), key_gt[b, kidx[b]] - 1) for b in range(B)]
    rres = [_Sampling(len(ridx[b]), ref_gt[b, ridx[b]] - 1) for b in range(B)]

    def host():
        ke = torch.cat([key[b, kidx[b]] for b in range(B)])
        re_ = torch.cat([ref[b, ridx[b]] for b in range(B)])
        losses = head.loss(*head.match(ke, re_, kres, rres), *head.get_track_targets(matches, kres, rres))
        return losses, torch.autograd.grad(losses['loss_track'] + losses['loss_track_aux'], (key, ref))

    def fused():
        losses = head.match_loss_rows(key, ref, key_gt, ref_gt, matches)
        return losses, torch.autograd.grad(losses['loss_track'] + losses['loss_track_aux'], (key, ref))

    (lh, gh), (lf, gf) = host(), fused()
    for k in lh:
        assert abs(float(lh[k].detach()) - float(lf[k].detach())) < 1e-5 * max(1.0, abs(float(lh[k].detach()))), k
    for a, b in zip(gh, gf):
        assert float((a - b).abs().max()) < 1e-4 * float(a.abs().max())
    h_min, h_med = timed(host, args.calls, args.warmup)
    f_min, f_med = timed(fused, args.calls, args.warmup)
    box = torch.cuda.get_device_name(0)
    stamp = datetime.date.today().isoformat()
    shape = f'B={B} N={N} positives={POS}/{POS} E={E} calls={args.calls}'
    lines = [f'{stamp} {box} {shape} host  fwd+bwd per call: min {h_min * 1e3:.1f} us  median {h_med * 1e3:.1f} us',
             f'{stamp} {box} {shape} fused fwd+bwd per call: min {f_min * 1e3:.1f} us  median {f_med * 1e3:.1f} us  '
             f'(host / fused: min {h_min / f_min:.2f}x median {h_med / f_med:.2f}x)']
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
