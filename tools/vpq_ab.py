"""A/B of one VPQ `update_state` with ks = (1, 2, 4, 6): the device meter (`VPQMeter`, csrc/vkn_vpq.hip: per VKN_VPQ_GROUP frames one clear,
one count and one window launch, no host read) beside
    stq      `STQMeter.update_state` on the same maps (csrc/vkn_stq.hip: the same 16 bytes per pixel through the same counting engine,
             csrc/vkn_mapcount.h, one launch);
    copy     the device -> host copy of the four int32 maps alone, wall clock with a synchronisation;
    host     copy + the NumPy restatement tests/vpq_ref.py (one np.unique per table and frame, then dicts per window: already far less
             work than the scripts' three np.unique sorts per window and window length; the reference itself is not needed).

    device   HIP events around each `update_state`, `--iters` timed calls after `--warmup`; the inputs rotate through `--frames` distinct
             batches, so that no cache level serves the maps (16 batches of 1024 x 2048 x 4 maps are 537 MB at B = 1).  The batches are
             fed as consecutive frames of one sequence.
The tables after the first two batches are compared with the host's before anything is timed.

    python tools/vpq_ab.py [--iters 20] [--warmup 5] [--frames 16] [--host-iters 3] [--out profiles/vpq_ab.txt]
    python tools/vpq_ab.py --trace-only        # only VPQ updates at the larger shape, for a kernel trace of its own
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
import vpq_ref  # noqa: E402
import vkn_import  # noqa: E402

SHAPES = ((384, 1248), (1024, 2048))
BATCHES = (1, 8)
KS = (1, 2, 4, 6)
STQ_CFG = dict(num_classes=19, things_list=list(range(11, 19)), ignore_label=255, label_bit_shift=16, offset=2 ** 16 * 256)
VPQ_CFG = dict(num_classes=19, things_list=list(range(11, 19)), ks=KS)
CAPACITY = dict(pair=8192)      # 60 x 60 ids can meet in a window of these maps: more than the default 2048


def batch(gen, B, H, W, dev):
    """gt_sem, gt_ins, pred_sem, pred_ins int32 [B,H,W] on the device: segments of 32 x 32 pixels, 5 % ignore, ids 0 .. 5 on things; the
    prediction is the ground truth moved by (5, 9) pixels with a tenth of its segments redrawn (the inputs of tools/stq_ab.py)."""
    hb, wb = -(-H // 32), -(-W // 32)
    up = lambda a: a.repeat_interleave(32, 1).repeat_interleave(32, 2)[:, :H, :W]            # noqa: E731
    sem = torch.randint(0, 19, (B, hb, wb), generator=gen, device=dev, dtype=torch.int32)
    sem[torch.rand((B, hb, wb), generator=gen, device=dev) < 0.05] = 255
    ins = torch.randint(0, 6, (B, hb, wb), generator=gen, device=dev, dtype=torch.int32)
    redraw = torch.rand((B, hb, wb), generator=gen, device=dev) < 0.1
    psem = torch.where(redraw | (sem == 255), torch.randint(0, 19, (B, hb, wb), generator=gen, device=dev, dtype=torch.int32), sem)
    pins = torch.where(redraw, torch.randint(1, 6, (B, hb, wb), generator=gen, device=dev, dtype=torch.int32), ins.clamp(min=1))
    thing = lambda s: (s >= 11) & (s <= 18)           # noqa: E731
    gs, gi, ps, pi = up(sem), up(ins), up(psem).roll((5, 9), (1, 2)), up(pins).roll((5, 9), (1, 2))
    return [t.contiguous() for t in (gs, gi * thing(gs), ps, pi * thing(ps))]


def timed(fn, inputs, args):
    for i in range(args.warmup):
        fn(*inputs[i % args.frames])
    torch.cuda.synchronize()
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(args.iters)]
    for i, (a, b) in enumerate(ev):
        a.record()
        fn(*inputs[(args.warmup + i) % args.frames])
        b.record()
    torch.cuda.synchronize()
    return [a.elapsed_time(b) * 1e-3 for a, b in ev]


def measure(vkn, H, W, B, args, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(1000 * B + H)
    inputs = [batch(gen, B, H, W, dev) for _ in range(args.frames)]
    # the values first: two calls, so that windows reach back over a call
    meter = vkn.VPQMeter(**VPQ_CFG, capacity=CAPACITY, device=dev)
    ref = vpq_ref.VPQRef(**VPQ_CFG)
    for i in range(2):
        meter.update_state(*inputs[i])
        ref.update_state(*(t.cpu().numpy() for t in inputs[i]))
    got, want = meter.tables(0), ref.tables(0)
    assert got['status'] == 0 and np.array_equal(got['acc'], want['acc']) and np.array_equal(got['log'], want['log']), 'device and host differ'
    meter.reset_states()
    t_vpq = timed(meter.update_state, inputs, args)
    meter.check_status()
    stq = vkn.STQMeter(**STQ_CFG, device=dev)
    t_stq = timed(stq.update_state, inputs, args)
    stq.check_status()
    t_copy, t_host = [], []
    ref = vpq_ref.VPQRef(**VPQ_CFG)
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
    return dict(H=H, W=W, B=B, vpq=med(t_vpq) / B, vpq_min=min(t_vpq) / B, vpq_max=max(t_vpq) / B, stq=med(t_stq) / B, copy=med(t_copy) / B,
                host=med(t_host) / B, rate=16.0 * H * W * B / med(t_vpq), largest=dict(ref.largest))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=20)
    ap.add_argument('--warmup', type=int, default=5)
    ap.add_argument('--frames', type=int, default=16)
    ap.add_argument('--host-iters', type=int, default=3)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vpq_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('vpq_ab.py measures on the GPU; there is none here')
    assert args.frames >= 16
    vkn = vkn_import.load()
    dev = torch.device('cuda:0')
    if args.trace_only:
        for B in BATCHES:
            gen = torch.Generator(device=dev)
            gen.manual_seed(B)
            inputs = [batch(gen, B, *SHAPES[1], dev) for _ in range(args.frames)]
            meter = vkn.VPQMeter(**VPQ_CFG, capacity=CAPACITY, device=dev)
            t = timed(meter.update_state, inputs, args)
            meter.check_status()
            print(f'{SHAPES[1]} B={B}: {statistics.median(t) / B * 1e6:.1f} us per frame')
        return
    rows = [measure(vkn, H, W, B, args, dev) for (H, W) in SHAPES for B in BATCHES]
    C = vkn._lib.VPQ
    lines = [f'# tools/vpq_ab.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} '
             f'frames={args.frames} host_iters={args.host_iters}  ks={KS}',
             f'# SPAN_PX={C["VKN_VPQ_SPAN_PX"]} LDS_SLOTS={C["VKN_VPQ_LDS_SLOTS"]} GROUP={C["VKN_VPQ_GROUP"]}; per FRAME: median (min .. max) of the timed calls / B',
             '#   shape      B   VPQ us (min .. max)        STQ us   VPQ/STQ      copy us    copy+host us   host/VPQ   copy/VPQ   GB/s @16 B/px   keys gt/pred/pair']
    for r in rows:
        lines.append(f'{r["H"]:5d}x{r["W"]:<5d} {r["B"]:2d}   {r["vpq"] * 1e6:8.1f} ({r["vpq_min"] * 1e6:.1f} .. {r["vpq_max"] * 1e6:.1f})   '
                     f'{r["stq"] * 1e6:8.1f}   {r["vpq"] / r["stq"]:6.2f}x   {r["copy"] * 1e6:10.0f}   {r["host"] * 1e6:12.0f}   {r["host"] / r["vpq"]:8.0f}x   '
                     f'{r["copy"] / r["vpq"]:7.1f}x   {r["rate"] / 1e9:12.0f}   {r["largest"]["gt"]}/{r["largest"]["pred"]}/{r["largest"]["pair"]}')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
