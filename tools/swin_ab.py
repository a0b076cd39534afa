"""Swin backbone, A/B in one process: the attention span of a `SwinTransformerBlock` (video-k-net_amd/swin.py) on the fused path
(`attention_fused`: qkv Linear + `vkn_swin_window_attn_f32` + proj) against the torch composition's same span (`attention_torch`: pad,
roll, partition, qkv Linear, bias gather, mask add, softmax, P V, proj, reverse, roll back, crop), from after norm1 to before the residual,
on the same parameters; then the whole eval forward of Swin-B, fused against `fused=False`.

Shapes: the four stage maps of Swin-B (128 ... 1024 channels, 4 ... 32 heads) and Swin-L (192 ... 1536, 6 ... 48) at a KITTI-STEP frame
(384 x 1248) and a COCO frame (800 x 1344), unshifted and shifted blocks, B = 1 and 2.

Per shape: warm-up of both arms, then `--passes` passes of `--repeats` rounds that alternate the arms; every call is timed with its own
pair of HIP events (device time), on inputs that rotate through as many seeded copies as exceed 256 MiB (no arm re-reads what the other
left in the caches).  Reported per arm: the median of all rounds, and the SPREAD = (largest - smallest) / middle of the passes' medians,
the run-to-run variation of this tool on this box.  The kernel alone is timed the same way on rotating qkv rows and set against its floor,
one read of qkv plus one write of out at 8.0 TB/s (the HBM3E specification).

The verdict line says whether the fused span is faster at EVERY shape by more than the larger spread of the two arms: that decides
`swin.FUSED_DEFAULT`.  Writes profiles/swin_ab.txt (or --out).

    python tools/swin_ab.py [--warmup 3] [--repeats 7] [--passes 3] [--quick] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vkn_import  # noqa: E402

FRAMES = {'kitti_384x1248': (384, 1248), 'coco_800x1344': (800, 1344)}
MODELS = {'swin_b': (128, (2, 2, 18, 2), (4, 8, 16, 32)), 'swin_l': (192, (2, 2, 18, 2), (6, 12, 24, 48))}
WINDOW, ROTATE_BYTES, HBM_BYTES_PER_S = 7, 256 << 20, 8.0e12


def stage_maps(h, w):
    h, w = (h + 3) // 4, (w + 3) // 4
    out = []
    for _ in range(4):
        out.append((h, w))
        h, w = (h + 1) // 2, (w + 1) // 2
    return out


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def _ab(arms, sets, warmup, repeats, passes):
    """arms ((name, fn(set)), ...) -> {name: (median ms of all rounds, spread of the passes' medians)}"""
    for i in range(warmup):
        for _, fn in arms:
            fn(sets[i % len(sets)])
    torch.cuda.synchronize()
    result, n = {name: [] for name, _ in arms}, 0
    for _ in range(passes):
        times = {name: [] for name, _ in arms}
        for i in range(repeats):
            for name, fn in (arms if i % 2 == 0 else arms[::-1]):
                s = sets[n % len(sets)]
                n += 1
                times[name].append(_time(lambda: fn(s)))
        for name in times:
            result[name].append(times[name])
    out = {}
    for name, per_pass in result.items():
        meds = sorted(statistics.median(p) for p in per_pass)
        out[name] = (statistics.median([t for p in per_pass for t in p]), (meds[-1] - meds[0]) / statistics.median(meds))
    return out


def _copies(nbytes):
    return max(2, ROTATE_BYTES // max(1, nbytes) + 2)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='one frame, one model, B = 1: a rehearsal')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swin_ab.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'swin_ab.py measures on the MI355X: there is no CPU arm'
    vkn = vkn_import.load()
    from video_k_net_amd import swin
    dev = torch.device('cuda:0')
    lines = [f'swin_ab: {torch.cuda.get_device_name(0)}; warmup {args.warmup}, {args.passes} passes x {args.repeats} alternating rounds, device events, ms',
             'span = qkv Linear + window attention + proj, after norm1, before the residual; floor = (qkv + out bytes) / 8.0 TB/s', '']
    frames = dict(list(FRAMES.items())[:1]) if args.quick else FRAMES
    models = dict(list(MODELS.items())[:1]) if args.quick else MODELS
    worst, all_faster = None, True
    torch.manual_seed(0)
    with torch.no_grad():
        for fname, (fh, fw) in frames.items():
            for mname, (embed, _, heads) in models.items():
                for stage, (H, W) in enumerate(stage_maps(fh, fw)):
                    dim, nh = embed * 2 ** stage, heads[stage]
                    for shift in (0, WINDOW // 2):
                        blk = swin.SwinTransformerBlock(dim=dim, num_heads=nh, window_size=WINDOW, shift_size=shift, fused=True).to(dev).eval()
                        torch.nn.init.normal_(blk.attn.relative_position_bias_table, std=0.5)
                        blk.H, blk.W = H, W
                        mask = swin.shift_attention_mask(H, W, WINDOW, WINDOW // 2, dev)
                        for B in ((1,) if args.quick else (1, 2)):
                            assert blk.fused_path(torch.empty((B, H * W, dim), device=dev))
                            xs = [torch.randn((B, H * W, dim), device=dev) for _ in range(_copies(B * H * W * dim * 4))]
                            r = _ab((('fused', blk.attention_fused), ('torch', lambda x: blk.attention_torch(x, mask))), xs, args.warmup, args.repeats, args.passes)
                            err = (blk.attention_fused(xs[0]) - blk.attention_torch(xs[0], mask)).abs().max().item()
                            del xs
                            qs = [torch.randn((B, H * W, 3 * dim), device=dev) for _ in range(_copies(B * H * W * 3 * dim * 4))]
                            a = blk.attn
                            k = _ab((('kernel', lambda q: vkn.ops.swin_window_attention(q, a.qkv.bias, a.relative_position_bias_table, H, W, nh, WINDOW, shift, a.scale)),),
                                    qs, args.warmup, args.repeats, args.passes)['kernel']
                            del qs
                            floor_ms = B * H * W * 4 * dim * 4 / HBM_BYTES_PER_S * 1e3
                            (tf, sf), (tt, st) = r['fused'], r['torch']
                            spread = max(sf, st)
                            faster = tf * (1 + spread) < tt
                            all_faster &= faster
                            if worst is None or tt / tf < worst[0]:
                                worst = (tt / tf, f'{fname} {mname} stage {stage} shift {shift} B {B}')
                            lines.append(f'{fname} {mname} stage {stage} {H:>3}x{W:<3} C {dim:<4} heads {nh:<2} shift {shift} B {B}: fused {tf:8.3f} (spread {sf:5.1%})  '
                                         f'torch {tt:8.3f} (spread {st:5.1%})  torch/fused {tt / tf:5.2f}  {"faster" if faster else "NOT faster"}  |  kernel {k[0]:7.3f} '
                                         f'floor {floor_ms:6.3f} share {floor_ms / k[0]:5.1%}  |  max |fused - torch| {err:.1e}')
                            print(lines[-1], flush=True)
        lines += ['', f'fused span faster than the torch span by more than the spread at every shape: {"YES" if all_faster else "NO"}; the smallest torch/fused is '
                  f'{worst[0]:.2f} ({worst[1]})', '']
        print(lines[-2], flush=True)
        # the whole eval forward of Swin-B
        embed, depths, heads = MODELS['swin_b']
        nets = {}
        for fused in (True, False):
            torch.manual_seed(1)
            nets[fused] = swin.SwinTransformerDIY(embed_dims=embed, depths=list(depths), num_heads=list(heads), drop_path_rate=0.3, fused=fused).to(dev).eval()
        for fname, (fh, fw) in frames.items():
            imgs = [torch.randn((1, 3, fh, fw), device=dev) for _ in range(3)]
            r = _ab((('fused', nets[True]), ('torch', nets[False])), imgs, 2, max(3, args.repeats // 2), args.passes)
            err = max((a - b).abs().max().item() for a, b in zip(nets[True](imgs[0]), nets[False](imgs[0])))
            (tf, sf), (tt, st) = r['fused'], r['torch']
            lines.append(f'{fname} swin_b whole eval forward B 1: fused {tf:8.3f} (spread {sf:5.1%})  torch {tt:8.3f} (spread {st:5.1%})  torch/fused {tt / tf:5.2f}  |  '
                         f'max |fused - torch| over the four levels {err:.1e}')
            print(lines[-1], flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
