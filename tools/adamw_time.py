"""The optimizer step of the shipped schedule (AdamW lr 1e-4, weight_decay 0.05, clip max_norm 1) on the cfg3 training head that
`bench.py --train` builds: dist.FlatAdamW (vkn_adamw_flat_f32, three launches over the flat gradient buckets) against
torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW (fused=True where this torch builds it, foreach otherwise) over the same
parameters with the same seeded gradients.  Device events around `--iters` steps after `--warmup`; prints one JSON line with the
parameter count and the byte floor (the norm reads 4 B, the update reads 16 B and writes 12 B per parameter, at 6.3 TB/s).
The kernel trace is a separate run: `rocprofv3 --kernel-trace --stats -- python tools/adamw_time.py --only flat`.

    python tools/adamw_time.py [--warmup 20] [--iters 200] [--only flat|torch] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vkn_import  # noqa: E402
from bench import CFG2  # noqa: E402

HBM_BYTES_PER_S = 6.3e12
BYTES_PER_PARAM = 4 + 16 + 12


def _head(vkn, device):
    """bench.py train_main's head: the cfg3 video head at x4, seeded construction and init."""
    cfg = vkn.configs.roi_head_cfg(True, C=CFG2['C'], heads=CFG2['heads'], ffn=CFG2['ffn'], ncls=CFG2['ncls'], n_thing=CFG2['n_thing'],
                                   n_stuff=CFG2['n_stuff'], S=CFG2['S'], up=4, nprop=CFG2['nprop'],
                                   train_cfg=vkn.configs.rcnn_train_cfg(CFG2['S']))
    torch.manual_seed(0)
    head = vkn.build_head(cfg)
    torch.manual_seed(0)
    head.init_weights()
    return head.to(device).train()


def _seeded_grads(params, seed=4321):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return [torch.randn(tuple(p.shape), generator=g) * 1e-3 for p in params]


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--iters', type=int, default=200)
    ap.add_argument('--only', choices=['flat', 'torch'], default=None)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    vkn = vkn_import.load()
    from importlib import import_module
    vdist = import_module('video_k_net_amd.dist')
    dev = torch.device('cuda:0')
    head = _head(vkn, dev)
    red = vdist.BucketedGradAllReducer(head)
    params = [p for b in red.buckets for p in b['params']]
    grads = _seeded_grads(params)
    n = sum(p.numel() for p in params)
    res = dict(tool='adamw_time', params=n, tensors=len(params), buckets=len(red.buckets), warmup=args.warmup, iters=args.iters,
               bytes_per_param=BYTES_PER_PARAM, floor_us=round(n * BYTES_PER_PARAM / HBM_BYTES_PER_S * 1e6, 2))
    if args.only in (None, 'torch'):
        clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
        for c, g in zip(clones, grads):
            c.grad = g.to(dev)
        try:
            topt, kind = torch.optim.AdamW(clones, lr=1e-4, weight_decay=0.05, fused=True), 'fused'
        except (RuntimeError, ValueError, TypeError):
            topt, kind = torch.optim.AdamW(clones, lr=1e-4, weight_decay=0.05, foreach=True), 'foreach'

        def torch_step():
            torch.nn.utils.clip_grad_norm_(clones, 1.0)
            topt.step()
        res['torch_kind'] = kind
        res['torch_us'] = round(_time(torch_step, args.warmup, args.iters) * 1e3, 2)
    if args.only in (None, 'flat'):
        red.zero_grad(set_to_none=True)
        for p, g in zip(params, grads):
            p.grad = g.to(dev)
        red.finalize()
        opt = vdist.FlatAdamW(red, lr=1e-4, weight_decay=0.05, max_norm=1.0)
        res['work_items'] = opt._n_items
        res['flat_us'] = round(_time(opt.step, args.warmup, args.iters) * 1e3, 2)
        res['flat_over_floor'] = round(res['flat_us'] / res['floor_us'], 2)
        res['grad_norm'] = float(opt.last_grad_norm)
    if 'flat_us' in res and 'torch_us' in res:
        res['torch_over_flat'] = round(res['torch_us'] / res['flat_us'], 2)
    line = json.dumps(res)
    print(line, flush=True)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
