"""A/B of the instance masks' way from the head's logits to their two device consumers, per image of K masks.

    arm A   the unfused path: torch's `rescale_masks` chain (sigmoid, two bilinear resizes with a crop between them: K full-resolution fp32
            maps, twice as intermediates and once as the result), then `ops.rle_encode(fp32, thr)` resp. `ops.mask_overlap(fp32, gt, thr)`,
            whose first pass packs the fp32 maps to bits;
    arm B   the fused path with up = 1: `ops.instance_mask_bits` on the same x4-scaled logits (one launch: logits in, bits out), then
            `ops.rle_encode_bits` resp. `ops.mask_overlap_bits`;
    arm C   the fused path from the stride-8 logits (up = 4): the x4 upsample happens inside the tile as well.

Device time only (HIP events around the launches, nothing copied to the host), medians over `--iters`, the arms alternating inside one
process, iteration by iteration.  Every arm's inputs rotate through as many distinct buffers as it takes to exceed 256 MiB, so that the
Infinity Cache serves none of them.  Beside each median its spread (max - min over the iterations); the verdict column says whether B's
median beats A's by more than the larger of the two spreads.  `floor` is the fused kernel's one-read-one-write time at HBM peak from the
ALGORITHMIC bytes (the logits it reads once + the bits it writes); `share` = floor / measured.

Before anything is timed the three arms' mask areas are compared on the first image: they must agree within 1e-3 of the pixels (the
exact comparison, on the pixels that tests/instmask_ref.py calls decided, is the suite's business).

    python tools/instmask_ab.py [--iters 11] [--warmup 2] [--out profiles/instmask_ab.txt] [--kernels profiles/instmask_kernels.txt]
"""
import argparse
import datetime
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vkn_import  # noqa: E402

# name, K, stride-8 logits (Hm, Wm), batch_input_shape, img_shape, ori_shape
SHAPES = (('VIP-Seg 720x1280', 100, (184, 320), (736, 1280), (720, 1280), (720, 1280)),
          ('YouTube-VIS 360x640 -> 720x1280', 100, (96, 160), (384, 640), (360, 640), (720, 1280)),
          ('COCO 800x1344', 100, (200, 336), (800, 1344), (800, 1344), (800, 1344)),
          ('1024x2048', 20, (256, 512), (1024, 2048), (1024, 2048), (1024, 2048)))
UP = 4
HBM_PEAK = 8.0e12          # bytes / s, MI355X
ROTATE_BYTES = 256 << 20
G = 10                     # ground truths of the overlap arms
THR = 0.5


def blobs(gen, N, H, W, dev):
    """stride-8 logits of instance-like masks: box-filtered noise, scaled so that the sigmoid saturates inside the blobs"""
    n = torch.rand((N, 1, H, W), generator=gen, device=dev)
    for _ in range(2):
        n = torch.nn.functional.avg_pool2d(n, 7, stride=1, padding=3, count_include_pad=False)
    n = (n - n.mean()) / n.std()
    return (6.0 * n[:, 0] - 3.0).contiguous()


def timed(fn):
    a, z = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    z.record()
    torch.cuda.synchronize()
    return a.elapsed_time(z) * 1e-3, out


def measure(vkn, name, K, lo, bis, img, ori, args, dev, stages):
    ops = vkn.ops
    meta = dict(batch_input_shape=bis, img_shape=(*img, 3), ori_shape=(*ori, 3))
    H, W = ori
    gen = torch.Generator(device=dev)
    gen.manual_seed(K + H)
    n_lo = ROTATE_BYTES // (K * lo[0] * lo[1] * 4) + 2
    n_hi = ROTATE_BYTES // (K * lo[0] * lo[1] * 4 * UP * UP) + 2
    low = [blobs(gen, K, *lo, dev) for _ in range(n_lo)]
    scaled = [torch.nn.functional.interpolate(x[None], scale_factor=UP, mode='bilinear', align_corners=False)[0].contiguous() for x in low[:n_hi]]
    gt = (ops.rescale_masks_torch(scaled[0][:G].roll(5, 2), meta) > THR).contiguous()
    need_f, need_b = ops.rle_workspace_bytes(K, H, W), ops.rle_bits_workspace_bytes(K, H, W)
    ws = torch.empty((need_f,), dtype=torch.uint8, device=dev)
    head = torch.zeros((K * 9 + 1,), dtype=torch.int32, device=dev)
    runs, pool = torch.empty((1 << 22,), dtype=torch.int32, device=dev), torch.empty((1 << 23,), dtype=torch.uint8, device=dev)

    def rle_f32(p):
        ops.rle_encode(p, head[:-1], runs, pool, head[-1:], ws[:need_f], thr=THR)

    def rle_bits(b):
        ops.rle_encode_bits(b, W, head[:-1], runs, pool, head[-1:], ws[:need_b])
    arms = dict(
        A_rle=lambda i: rle_f32(ops.rescale_masks_torch(scaled[i % n_hi], meta)),
        B_rle=lambda i: rle_bits(ops.instance_mask_bits(scaled[i % n_hi], meta, THR, up=1)),
        C_rle=lambda i: rle_bits(ops.instance_mask_bits(low[i % n_lo], meta, THR, up=UP)),
        A_ap=lambda i: ops.mask_overlap(ops.rescale_masks_torch(scaled[i % n_hi], meta), gt, thr=THR),
        B_ap=lambda i: ops.mask_overlap_bits(ops.instance_mask_bits(scaled[i % n_hi], meta, THR, up=1), W, gt),
        C_ap=lambda i: ops.mask_overlap_bits(ops.instance_mask_bits(low[i % n_lo], meta, THR, up=UP), W, gt),
        A_chain=lambda i: ops.rescale_masks_torch(scaled[i % n_hi], meta),
        B_bits=lambda i: ops.instance_mask_bits(scaled[i % n_hi], meta, THR, up=1),
        C_bits=lambda i: ops.instance_mask_bits(low[i % n_lo], meta, THR, up=UP))
    # the values first: areas of the three arms on image 0
    ta, tb, tc = (arms[k](0) for k in ('A_ap', 'B_ap', 'C_ap'))
    torch.cuda.synchronize()
    px = K * H * W
    for t, arm in ((tb, 'B'), (tc, 'C')):
        d = int((t[1] - ta[1]).abs().sum())
        assert d <= 1e-3 * px, f'{name}: arm {arm} differs from arm A in {d} of {px} pixels'
    t = {k: [] for k in arms}
    for i in range(args.warmup + args.iters):
        for k, fn in arms.items():
            dt, out = timed(lambda: fn(i))
            del out
            if i >= args.warmup:
                t[k].append(dt)
    row = dict(name=name, K=K, H=H, W=W, lo=lo)
    for k, v in t.items():
        row[k] = statistics.median(v)
        row[k + '_sp'] = max(v) - min(v)
    bits_bytes = 8 * K * ((W + 63) // 64) * H
    row['floor_B'] = (K * lo[0] * lo[1] * 4 * UP * UP + bits_bytes) / HBM_PEAK
    row['floor_C'] = (K * lo[0] * lo[1] * 4 + bits_bytes) / HBM_PEAK
    row['chain_bytes'] = px * 4 * 2 + 2 * 2 * K * bis[0] * bis[1] * 4 + K * lo[0] * lo[1] * 16 * 4      # logits read, two intermediates written and read, the result written, then read by the pack
    stages.append(row)
    return row


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--iters', type=int, default=11)
    ap.add_argument('--warmup', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'instmask_ab.txt'))
    ap.add_argument('--kernels', default=os.path.join(ROOT, 'profiles', 'instmask_kernels.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('instmask_ab.py measures on the GPU; there is none here')
    vkn = vkn_import.load()
    dev = torch.device('cuda:0')
    rows, stages = [], []
    for shape in SHAPES:
        rows.append(measure(vkn, *shape, args, dev, stages))
        print(f'# measured {shape[0]}', flush=True)
        torch.cuda.empty_cache()
    C = vkn._lib.INSTMASK
    head = (f'# tools/instmask_ab.py  {datetime.date.today().isoformat()}  {torch.cuda.get_device_name(0)}  iters={args.iters} warmup={args.warmup}  '
            f'tile 64 x {C["VKN_INSTMASK_TILE_ROWS"]}, {C["VKN_INSTMASK_BATCH"]} masks per workgroup; inputs rotate through > 256 MiB')
    ms = lambda r, k: f'{r[k] * 1e3:8.3f} (+-{r[k + "_sp"] * 1e3:6.3f})'          # noqa: E731
    lines = [head, '# per IMAGE of K masks, device time in ms: median (max - min).  A = torch rescale + f32 consumer; B = fused, up = 1; C = fused from the stride-8 logits.',
             '# verdict: B beats A iff median(A) - median(B) > max(spread A, spread B).']
    for cons, label in (('rle', 'run-length encoder'), ('ap', f'mask overlap, {G} ground truths')):
        lines.append(f'# ---- consumer: {label}')
        lines.append('#   K  shape                               |                 A                  B                  C |   A/B    A/C | B beats A by more than the spread')
        for r in rows:
            a, b = r[f'A_{cons}'], r[f'B_{cons}']
            ok = a - b > max(r[f'A_{cons}_sp'], r[f'B_{cons}_sp'])
            lines.append(f'{r["K"]:5d}  {r["name"]:<35s} | {ms(r, "A_" + cons)} {ms(r, "B_" + cons)} {ms(r, "C_" + cons)} | {a / b:5.1f}x {a / r["C_" + cons]:5.1f}x | {"yes" if ok else "NO"}')
    lines.append('# ---- the fused kernel alone against its one-read-one-write floor at HBM peak (algorithmic bytes: the logits once + the bits)')
    lines.append(f'#   K  shape                               |   B kernel   floor  share |   C kernel   floor  share   (HBM peak {HBM_PEAK / 1e12:.1f} TB/s)')
    for r in rows:
        lines.append(f'{r["K"]:5d}  {r["name"]:<35s} | {r["B_bits"] * 1e3:10.3f} {r["floor_B"] * 1e3:7.3f} {100 * r["floor_B"] / r["B_bits"]:5.1f} % | '
                     f'{r["C_bits"] * 1e3:10.3f} {r["floor_C"] * 1e3:7.3f} {100 * r["floor_C"] / r["C_bits"]:5.1f} %')
    text = '\n'.join(lines) + '\n'
    print(text, end='')
    klines = [head, '# the stages of each arm on their own, device time in ms, median (max - min); torch chain: bytes moved by shape / time',
              '#   K  shape                               |  A: torch chain   (GB moved, TB/s) |  B: k_instmask up=1 |  C: k_instmask up=4 | f32 consumers minus chain: rle, overlap | bits consumers minus kernel: rle, overlap']
    for r in stages:
        klines.append(f'{r["K"]:5d}  {r["name"]:<35s} | {ms(r, "A_chain")} ({r["chain_bytes"] / 1e9:5.2f}, {r["chain_bytes"] / r["A_chain"] / 1e12:4.2f}) | {ms(r, "B_bits")} | {ms(r, "C_bits")} | '
                      f'{(r["A_rle"] - r["A_chain"]) * 1e3:7.3f} {(r["A_ap"] - r["A_chain"]) * 1e3:7.3f} | {(r["B_rle"] - r["B_bits"]) * 1e3:7.3f} {(r["B_ap"] - r["B_bits"]) * 1e3:7.3f}')
    ktext = '\n'.join(klines) + '\n'
    print(ktext, end='')
    for path, body in ((args.out, text), (args.kernels, ktext)):
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, 'w') as f:
            f.write(body)


if __name__ == '__main__':
    main()
