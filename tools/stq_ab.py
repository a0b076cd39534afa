"""A/B of one STQ `update_state`: the device meter (`STQMeter`, csrc/vkn_stq.hip: one launch, no host read) against the host path on the
same tensors — the device -> host copy of the four int32 maps plus the NumPy restatement tests/stq_ref.py (`np.unique` per table, as the
reference's `STQuality.update_state` does; the reference itself is not needed).

    device   HIP events around each `update_state`, `--iters` timed calls after `--warmup`; the inputs rotate through `--frames` distinct
             batches, so that no cache level serves the maps (16 batches of 1024 x 2048 x 4 maps are 537 MB at B = 1);
    copy     the four `.cpu()` copies alone, wall clock with a synchronisation;
    host     copy + `STQRef.update_state`, wall clock, `--host-iters` calls.
Achieved bytes / s is the algorithmic traffic, 16 bytes per pixel, over the device time.  The tables of the first batch are compared with
the host's before anything is timed.

    python tools/stq_ab.py [--iters 20] [--warmup 5] [--frames 16] [--host-iters 3] [--out profiles/stq_ab.txt]
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import stq_ref  # noqa: E402
import vkn_import  # noqa: E402

HBM = 6.3e12      # bytes / s: the rate the other floors of DESIGN.md use
SHAPES = ((384, 1248), (1024, 2048))
BATCHES = (1, 8)
CFG = stq_ref.KITTI


def batch(gen, B, H, W, dev):
    """gt_sem, gt_ins, pred_sem, pred_ins int32 [B,H,W] on the device: segments of 32 x 32 pixels, 5 % ignore, ids 0 .. 5 on things; the
    prediction is the ground truth moved by (5, 9) pixels with a tenth of its segments redrawn."""
    hb, wb = -(-H // 32), -(-W // 32)
    up = lambda a: a.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W]            # noqa: E731
    sem = torch.randint(0, CFG['num_classes'], (B, hb, wb), generator=gen, device=dev, dtype=torch.int32)
    sem[torch.rand((B, hb, wb), generator=gen, device=dev) < 0.05] = CFG['ignore_label']
    ins = torch.randint(0, 6, (B, hb, wb), generator=gen, device=dev, dtype=torch.int32)
    redraw = torch.rand((B, hb, wb), generator=gen, device=dev) < 0.1
    psem = torch.where(redraw, torch.randint(0, CFG['num_classes'], (B, hb, wb), generator=gen, device=dev, dtype=torch.int32), sem)
    pins = torch.where(redraw, torch.randint(1, 6, (B, hb, wb), generator=gen, device=dev, dtype=torch.int32), ins.clamp(min=1))
    thing = lambda s: (s >= CFG['things_list'][0]) & (s <= CFG['things_list'][-1])           # noqa: E731
    gs, gi, ps, pi = up(sem), up(ins), up(psem).roll((5, 9), (1, 2)), up(pins).roll((5, 9), (1, 2))
    return [t.contiguous() for t in (gs, gi * thing(gs), ps, pi * thing(ps))]


def measure(vkn, H, W, B, args, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * B + H)
    inputs = [batch(gen, B, H, W, dev) for _ in range(args.frames)]
    # the values first
    meter = vkn.STQMeter(**CFG, device=dev)
    meter.update_state(*inputs[0])
    ref = stq_ref.STQRef(**CFG)
    ref.update_state(*(t.cpu().numpy() for t in inputs[0]))
    got, want = meter.tables(0), ref.tables(0)
    assert got['status'] == 0 and all(np.array_equal(got[k], want[k]) for k in stq_ref.TABLE_KEYS), 'device and host tables differ'
    # device
    meter.reset_states()
    for i in range(args.warmup):
        meter.update_state(*inputs[i % args.frames])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
    for i, (a, b) in enumerate(ev):
        a.record()
        meter.update_state(*inputs[(args.warmup + i) % args.frames])
        b.record()
    torch.cuda.synchronize()
    meter.check_status()
    t_dev = [a.elapsed_time(b) * 1e-3 for a, b in ev]
    # the copy alone, then copy + host counting
    t_copy, t_host = [], []
    for i in range(args.host_iters):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        host = [t.cpu() for t in inputs[i % args.frames]]
        torch.cuda.synchronize()
        t1 = time.perf_counter()
        ref.update_state(*(t.numpy() for t in host))
        t2 = time.perf_counter()
        t_copy.append(t1 - t0)
        t_host.append(t2 - t0)
    med = statistics.median
    return dict(H=H, W=W, B=B, dev=med(t_dev) / B, dev_min=min(t_dev) / B, dev_max=max(t_dev) / B, copy=med(t_copy) / B, host=med(t_host) / B,
                rate=16.0 * H * W * B / med(t_dev), pairs=int(want['pair_keys'].size))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'stq_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('stq_ab.py measures on the GPU; there is none here')
    assert args.frames >= 16
    vkn = vkn_import.load()
    dev = torch.device('cuda:0')
    rows = [measure(vkn, H, W, B, args, dev) for (H, W) in SHAPES for B in BATCHES]
    lines = [f'# tools/stq_ab.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} '
             f'frames={args.frames} host_iters={args.host_iters}',
             f'# SPAN_PX={vkn._lib.STQ["VKN_STQ_SPAN_PX"]} LDS_SLOTS={vkn._lib.STQ["VKN_STQ_LDS_SLOTS"]}; per FRAME: median (min .. max) of the timed calls / B',
             '#   shape      B   device us (min .. max)      copy us    copy+host us   host/device   copy/device   GB/s @16 B/px   % of 6.3 TB/s   pairs']
    for r in rows:
        lines.append(f'{r["H"]:5d}x{r["W"]:<5d} {r["B"]:2d}   {r["dev"] * 1e6:8.1f} ({r["dev_min"] * 1e6:.1f} .. {r["dev_max"] * 1e6:.1f})   '
                     f'{r["copy"] * 1e6:10.0f}   {r["host"] * 1e6:12.0f}   {r["host"] / r["dev"]:10.0f}x   {r["copy"] / r["dev"]:9.1f}x   '
                     f'{r["rate"] / 1e9:12.0f}   {100 * r["rate"] / HBM:10.1f}   {r["pairs"]:6d}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
