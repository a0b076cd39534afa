"""A/B of the instance masks' way to COCO RLE, per image of K masks: the device encoder (`MaskRLE`, csrc/vkn_rle.hip: eight launches, then
the records and the used prefix of the byte pool copied to the host) beside what the reference's test loops do.

    a_u8     `MaskRLE()(masks)` on the K boolean masks, wall clock to the finished list of dicts (launches + both copies);
    a_f32    `MaskRLE()(logits, thr)` on the K fp32 maps the rescale leaves, the same way (what `get_seg_masks_rle` calls);
    dev_u8 / dev_f32   the eight launches alone, HIP events around `ops.rle_encode` (no copy): K H W element bytes over this time is a
             LOWER bound of the rate of the one pass that reads the input (k_rle_pack), whose floor is one read of K H W elements;
    b        the device -> host copy of the K boolean masks ALONE, wall clock with a synchronisation: a floor under any host encoder;
    c        that copy + tests/rle_ref.py's NumPy encoder over the K masks (pycocotools is not installed here: its C encoder would sit
             between b and c).

The arms alternate inside one process, iteration by iteration, and the inputs rotate through `--frames` distinct images so that no cache
level serves them.  Medians over `--iters` (c: `--host-iters`).  Inputs: "blobs" = a thresholded box-filtered noise (instance-like
masks), "noise" = independent pixels at p = 0.5, the encoder's worst case (every second pixel starts a run).  The first three masks of
every input are compared with rle_ref before anything is timed.

    python tools/rle_ab.py [--iters 15] [--warmup 3] [--frames 3] [--host-iters 2] [--out profiles/rle_ab.txt]
    python tools/rle_ab.py --trace-only       # only device encodes at the first size, for a kernel trace of its own
"""
import argparse
import datetime
import os
import statistics
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
import rle_ref  # noqa: E402
import vkn_import  # noqa: E402

SIZES = ((100, 720, 1280), (100, 384, 1248), (20, 1024, 2048))
HBM_PEAK = 8.0e12          # bytes / s, MI355X


def image(gen, kind, K, H, W, dev):
    """fp32 [K,H,W] whose sign is the mask: box-filtered noise (blobs of some tens of pixels) or plain noise"""
    n = torch.rand((K, 1, H, W), generator=gen, device=dev)
    if kind == 'blobs':
        for _ in range(3):
            n = torch.nn.functional.avg_pool2d(n, 15, stride=1, padding=7, count_include_pad=False)
        n = (n - n.mean()) / n.std()
        return n[:, 0].contiguous()
    return (n[:, 0] - 0.5).contiguous()


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def measure(vkn, kind, K, H, W, args, dev):
    gen = torch.Generator(device=dev)
    gen.manual_seed(H * 7 + K)
    logits = [image(gen, kind, K, H, W, dev) for _ in range(args.frames)]
    masks = [x > 0 for x in logits]
    enc = vkn.MaskRLE()
    for x, m in zip(logits, masks):                                     # the values first (and the pools grow to their final size)
        got_f, got_u = enc(x, thr=0.0), enc(m)
        assert got_f == got_u and got_u[:3] == [rle_ref.encode(a) for a in m[:3].cpu().numpy()], 'device and host differ'
    rec = enc.records()
    nruns, nbytes = float(rec[:, 0].mean()), float(rec[:, 2].mean())
    b = enc._buffers(dev)
    head = torch.zeros((K * 9 + 1,), dtype=torch.int32, device=dev)
    need = vkn.ops.rle_workspace_bytes(K, H, W)

    def dev_only(src, thr):
        a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        vkn.ops.rle_encode(src, head[:-1], b['runs'], b['pool'], head[-1:], b['ws'][:need], thr=thr)
        z.record()
        torch.cuda.synchronize()
        return a.elapsed_time(z) * 1e-3
    t = dict(a_u8=[], a_f32=[], dev_u8=[], dev_f32=[], b=[], c=[])
    for i in range(args.warmup + args.iters):
        x, m = logits[i % args.frames], masks[i % args.frames]
        row = dict(a_u8=wall(lambda: enc(m))[0], a_f32=wall(lambda: enc(x, thr=0.0))[0], dev_u8=dev_only(m, None), dev_f32=dev_only(x, 0.0),
                   b=wall(lambda: m.cpu())[0])
        if i >= args.warmup:
            for k, v in row.items():
                t[k].append(v)
            if len(t['c']) < args.host_iters:
                t['c'].append(wall(lambda: [rle_ref.encode(a) for a in m.cpu().numpy()])[0])
    med = {k: statistics.median(v) for k, v in t.items()}
    return dict(kind=kind, K=K, H=H, W=W, nruns=nruns, nbytes=nbytes, **med, lo=min(t['a_u8']), hi=max(t['a_u8']))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=15)
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--frames', type=int, default=3)
    ap.add_argument('--host-iters', type=int, default=2)
    ap.add_argument('--trace-only', action='store_true')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'rle_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('rle_ab.py measures on the GPU; there is none here')
    vkn = vkn_import.load()
    dev = torch.device('cuda:0')
    if args.trace_only:
        K, H, W = SIZES[0]
        gen = torch.Generator(device=dev)
        gen.manual_seed(1)
        x = image(gen, 'blobs', K, H, W, dev)
        m, enc = x > 0, vkn.MaskRLE()
        for _ in range(args.warmup + args.iters):
            enc(m)
            enc(x, thr=0.0)
        return
    rows = []
    for size in SIZES:
        for kind in ('blobs', 'noise'):
            rows.append(measure(vkn, kind, *size, args, dev))
            print(f'# measured {size} {kind}', flush=True)
    lines = [f'# tools/rle_ab.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup} '
             f'frames={args.frames} host_iters={args.host_iters}  STRIP_COLS={vkn._lib.RLE["VKN_RLE_STRIP_COLS"]} launches={vkn._lib.RLE["VKN_RLE_LAUNCHES"]}',
             '# per IMAGE of K masks, medians, ms.  a = device encode + copies of records and bytes (min .. max of a_u8); dev = the launches alone;',
             '# b = D2H copy of the K boolean masks alone; c = b + the NumPy encoder.  GB/s = K H W element bytes / dev: a lower bound of the',
             f'# input pass (k_rle_pack), whose floor is one read of the input; HBM peak {HBM_PEAK / 1e12:.1f} TB/s.',
             '#   K     shape     input  runs/mask  bytes/mask |   a_u8 (min .. max)     a_f32 |  dev_u8  dev_f32 |       b         c |  b/a_u8  b/a_f32  c/a_u8 | GB/s u8 (of peak)  GB/s f32 (of peak)']
    for r in rows:
        px = r['K'] * r['H'] * r['W']
        gu, gf = px / r['dev_u8'], 4 * px / r['dev_f32']
        lines.append(f'{r["K"]:5d} {r["H"]:5d}x{r["W"]:<5d} {r["kind"]:>6s} {r["nruns"]:10.0f} {r["nbytes"]:11.0f} | {r["a_u8"] * 1e3:7.3f} ({r["lo"] * 1e3:.3f} .. {r["hi"] * 1e3:.3f}) '
                     f'{r["a_f32"] * 1e3:8.3f} | {r["dev_u8"] * 1e3:7.3f} {r["dev_f32"] * 1e3:8.3f} | {r["b"] * 1e3:7.2f} {r["c"] * 1e3:9.1f} | {r["b"] / r["a_u8"]:6.1f}x '
                     f'{r["b"] / r["a_f32"]:7.1f}x {r["c"] / r["a_u8"]:6.0f}x | {gu / 1e9:7.0f} ({100 * gu / HBM_PEAK:4.1f} %) {gf / 1e9:9.0f} ({100 * gf / HBM_PEAK:4.1f} %)')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text)


if __name__ == '__main__':
    main()
