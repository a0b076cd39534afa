"""A/B of one image's way into COCO mask AP: the device meter (`MaskAPMeter.update`, csrc/vkn_maskap.hip: two pack launches, one overlap
launch, three small matching launches, nothing read back) beside what a host scorer needs first.

    a_u8     `meter.update(...)` on the K boolean masks, wall clock to a device synchronisation (launches only: there is no copy);
    a_f32    the same on the K fp32 maps the rescale leaves, with `thr` (what follows `get_seg_masks_device` without its `>`);
    dev_u8 / dev_f32   the overlap call alone (`ops.mask_overlap`: two packs + the overlap kernel), HIP events around it.  Its floor is
             ONE read of the inputs, (K * element bytes + G) * H * W bytes: GB/s = those bytes / this time, a LOWER bound of the pack's rate;
    b        the device -> host copy of the K boolean masks ALONE, wall clock with a synchronisation: a floor under any host scorer;
    c        that copy + tests/maskap_ref.py's NumPy overlaps and matching of the image (pycocotools is not installed here: its C code
             would sit between b and c).

The arms alternate inside one process, iteration by iteration, and the inputs rotate through `--frames` distinct images so that no cache
level serves them.  Per-image medians over `--iters` (c: `--host-iters`).  Inputs: thresholded box-filtered noise (instance-like blobs)
on both sides.  The tables of the first detections are compared with maskap_ref before anything is timed.  No time is a pass condition.

    python tools/maskap_ab.py [--iters 15] [--warmup 3] [--frames 3] [--host-iters 1] [--out profiles/maskap_ab.txt]
    python tools/maskap_ab.py --trace-only    # only device updates at the first size, for a kernel trace of its own
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
import maskap_ref  # noqa: E402
import vkn_import  # noqa: E402

SIZES = ((100, 20, 800, 1344), (100, 10, 720, 1280))
NUM_CLASSES = 80
HBM_PEAK = 8.0e12          # bytes / s, MI355X


def blobs(gen, n, H, W, dev, level):
    """fp32 [n,H,W]: box-filtered noise, standardised and shifted: `> 0` leaves instance-like blobs (the higher `level`, the smaller)"""
    x = torch.rand((n, 1, H, W), generator=gen, device=dev)
    for _ in range(3):
        x = torch.nn.functional.avg_pool2d(x, 15, stride=1, padding=7, count_include_pad=False)
    return ((x - x.mean()) / x.std() - level)[:, 0].contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(vkn, K, G, H, W, args, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(H * 7 + K + G)
    logits = [blobs(gen, K, H, W, dev, 1.0) for _ in range(args.frames)]
    masks = [x > 0 for x in logits]
    gts = [blobs(gen, G, H, W, dev, 1.0) > 0 for _ in range(args.frames)]
    scores = torch.rand((K,), generator=gen, device=dev)
    dl, gl = torch.randint(0, NUM_CLASSES, (K,), generator=gen, device=dev), torch.randint(0, NUM_CLASSES, (G,), generator=gen, device=dev)
    gl[:G // 2] = dl[:G // 2]                                           # some pairs share a class, so the matching has work
    crowd = torch.zeros((G,), dtype=torch.uint8, device=dev)
    for x, m, g in zip(logits, masks, gts):                             # the values first
        tu, tf = vkn.ops.mask_overlap(m, g), vkn.ops.mask_overlap(x, g, thr=0.0)
        want = maskap_ref.overlaps(m[:3].cpu().numpy(), g.cpu().numpy())
        assert all(torch.equal(a, b) for a, b in zip(tu, tf)), 'the two arms differ'
        assert np.array_equal(tu[0][:3].cpu().numpy(), want[0]) and np.array_equal(tu[1][:3].cpu().numpy(), want[1]) and np.array_equal(tu[2].cpu().numpy(), want[2]), 'device and host differ'
    meter = vkn.MaskAPMeter(NUM_CLASSES, capacity=K * (args.warmup + args.iters) * 2 + K)

    def dev_only(src, g, thr):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        vkn.ops.mask_overlap(src, g, thr=thr)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) * 1e-3

    def host(m, g):
        dt, gt = m.cpu().numpy(), g.cpu().numpy()
        tables = maskap_ref.overlaps(dt, gt)
        s, d, l = scores.cpu().numpy(), dl.cpu().numpy(), gl.cpu().numpy()
        for c in sorted(set(d.tolist()) | set(l.tolist())):
            for rng in maskap_ref.COCO_AREAS:
                maskap_ref.evaluate_img(tables, s, d, l, [0] * G, None, c, rng, maskap_ref.COCO_THRS, 1000)
    t = dict(a_u8=[], a_f32=[], dev_u8=[], dev_f32=[], b=[], c=[])
    for i in range(args.warmup + args.iters):
        x, m, g = logits[i % args.frames], masks[i % args.frames], gts[i % args.frames]
        row = dict(a_u8=wall(lambda: meter.update(i, m, scores, dl, g, gl, crowd))[0], a_f32=wall(lambda: meter.update(i, x, scores, dl, g, gl, crowd, thr=0.0))[0],
                   dev_u8=dev_only(m, g, None), dev_f32=dev_only(x, g, 0.0), b=wall(lambda: m.cpu())[0])
        if i >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
            if len(t['c']) < args.host_iters:
                t['c'].append(wall(lambda: host(m, g))[0])
    meter.check_status()
    med = {k: statistics.median(v) for k, v in t.items()}
    return dict(K=K, G=G, H=H, W=W, fill=float(torch.stack(masks).float().mean()), **med, lo=min(t['a_u8']), hi=max(t['a_u8']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--host-iters', type=int, default=1)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'maskap_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('maskap_ab.py measures on the GPU; there is none here')
    vkn = vkn_import.load()
    dev = torch.device('cuda:0')
    if args.trace_only:
        K, G, H, W = SIZES[0]
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        x, g = blobs(gen, K, H, W, dev, 1.0), blobs(gen, G, H, W, dev, 1.0) > 0
        m, meter = x > 0, vkn.MaskAPMeter(NUM_CLASSES, capacity=2 * K * (args.warmup + args.iters))
        scores, dl, gl = torch.rand((K,), device=dev), torch.randint(0, NUM_CLASSES, (K,), device=dev), torch.randint(0, NUM_CLASSES, (G,), device=dev)
        for i in range(args.warmup + args.iters):
            meter.update(i, m, scores, dl, g, gl)
            meter.update(i, x, scores, dl, g, gl, thr=0.0)
        torch.cuda.synchronize()
        return
    rows = []
    for size in SIZES:
        rows.append(measure(vkn, *size, args, dev))
        print(f'# measured {size}', flush=True)
    C = vkn._lib.MASKAP
    lines = [f'# tools/maskap_ab.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} '
             f'frames={args.frames} host_iters={args.host_iters}  ROW_RUN={C["VKN_MASKAP_ROW_RUN"]} DT_TILE={C["VKN_MASKAP_DT_TILE"]} '
             f'GT_TILE={C["VKN_MASKAP_GT_TILE"]} GT_CHUNK={C["VKN_MASKAP_GT_CHUNK"]}',
             '# per IMAGE, medians, ms.  a = MaskAPMeter.update to a synchronisation (min .. max of a_u8); dev = the overlap call alone (two packs + overlap);',
             '# b = D2H copy of the K boolean masks alone; c = b + the NumPy restatement (overlaps + matching).  GB/s = (K elem + G) H W bytes / dev:',
             f'# the floor of the overlap call is one read of its inputs; HBM peak {HBM_PEAK / 1e12:.1f} TB/s.',
             '#   K    G     shape    set px |   a_u8 (min .. max)     a_f32 |  dev_u8  dev_f32 |       b         c |  b/a_u8  b/a_f32  c/a_u8 | GB/s u8 (of peak)  GB/s f32 (of peak)']
    for r in rows:
        px = r['H'] * r['W']
        gu, gf = (r['K'] + r['G']) * px / r['dev_u8'], (4 * r['K'] + r['G']) * px / r['dev_f32']
        lines.append(f'{r["K"]:5d} {r["G"]:4d} {r["H"]:5d}x{r["W"]:<5d} {100 * r["fill"]:5.1f} % | {r["a_u8"] * 1e3:7.3f} ({r["lo"] * 1e3:.3f} .. {r["hi"] * 1e3:.3f}) '
                     f'{r["a_f32"] * 1e3:8.3f} | {r["dev_u8"] * 1e3:7.3f} {r["dev_f32"] * 1e3:8.3f} | {r["b"] * 1e3:7.2f} {r["c"] * 1e3:9.1f} | {r["b"] / r["a_u8"]:6.1f}x '
                     f'{r["b"] / r["a_f32"]:7.1f}x {r["c"] / r["a_u8"]:6.0f}x | {gu / 1e9:7.0f} ({100 * gu / HBM_PEAK:4.1f} %) {gf / 1e9:9.0f} ({100 * gf / HBM_PEAK:4.1f} %)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
