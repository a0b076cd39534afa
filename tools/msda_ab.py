"""Deformable-attention neck, A/B in one process: (a) the sampling core `vkn_msda_sample_f32` (include/vkn_msda.h) against torch's
`F.grid_sample` composition on the same operands, (b) the whole eval forward of `MSDeformAttnPixelDecoder` on the fused path against
its own `forward_torch`, on the same parameters, at the encoder level sizes of a COCO frame (800 x 1344: 100 x 168, 50 x 84, 25 x 42)
and a YouTube-VIS frame (360 x 640: 45 x 80, 23 x 40, 12 x 20), B = 1 and 2, the shipped widths (256 channels, 8 heads, 3 levels,
4 points, 6 layers).

Per size: warm-up of both arms, then `--repeats` rounds that alternate the arms; every call is timed with its own pair of HIP events,
on inputs that rotate through `--sets` seeded sets (so that no arm re-reads what the other left in the caches); the median and the
minimum per arm are reported.  Writes profiles/msda_ab.txt (or --out).

    python tools/msda_ab.py [--warmup 3] [--repeats 20] [--sets 3] [--only coco|ytvis] [--out FILE]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vkn_import  # noqa: E402

FRAMES = {'coco_800x1344': ((200, 336), (100, 168), (50, 84), (25, 42)), 'ytvis_360x640': ((90, 160), (45, 80), (23, 40), (12, 20))}
IN_CHANNELS = (256, 512, 1024, 2048)
M, D, P = 8, 32, 4


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _ab(arms, sets, warmup, repeats):
    """arms: ((name, fn(set)), (name, fn(set))) -> {name: [ms]}, the arms alternating, the input sets rotating"""
    for _ in range(warmup):
        for _, fn in arms:
            fn(sets[0])
    torch.cuda.synchronize()
    times = {name: [] for name, _ in arms}
    for i in range(repeats):
        for j, (name, fn) in enumerate(arms if i % 2 == 0 else arms[::-1]):
            s = sets[(2 * i + j) % len(sets)]
            times[name].append(_time(lambda: fn(s))[0])
    return times


def _report(lines, times, first, second):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(f'    {k:<26} median {med[k]:9.3f}  min {min(v):9.3f}  max {max(v):9.3f}')
    lines.append(f'    {first} / {second} (medians) {med[first] / med[second]:.3f}')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--only', default=None, help='coco or ytvis')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msda_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('msda_ab: needs the GPU (a timing taken elsewhere says nothing)')
    vkn = vkn_import.load()
    from video_k_net_amd.msdeform_decoder import msda_core_torch
    torch.manual_seed(0)
    neck = vkn.MSDeformAttnPixelDecoder()
    neck.init_weights()
    with torch.no_grad():                                    # the init leaves every offset weight at zero: spread the samples as a trained neck does
        for layer in neck.encoder.layers:
            layer.attentions[0].sampling_offsets.weight.normal_(0, 0.05)
            layer.attentions[0].attention_weights.weight.normal_(0, 0.1)
    neck = neck.cuda().eval()
    lines = [f'tool msda_ab  device {torch.cuda.get_device_name(0)}  C 256  heads {M}  levels 3  points {P}  layers 6  warmup {args.warmup}  '
             f'repeats {args.repeats}  input sets {args.sets}', 'ms per call (HIP events around each call; arms alternate)', '']
    shown = 0
    for name, sizes in FRAMES.items():
        if args.only and args.only not in name:
            continue
        shapes = [sizes[3], sizes[2], sizes[1]]              # the encoder's order: low to high resolution
        S = sum(h * w for h, w in shapes)
        for B in (1, 2):
            gen = torch.Generator(device='cuda').manual_seed(1)
            lines.append(f'{name}  B {B}  levels {shapes}  S = Q = {S}  value {B * S * M * D * 4 / 2 ** 20:.1f} MiB')
            # ---- (a) the core alone
            _, ref = neck.shape_constants(shapes, torch.device('cuda', 0))
            wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device='cuda')
            sets = []
            for _ in range(args.sets):
                value = torch.randn((B, S, M * D), device='cuda', generator=gen)
                both = torch.randn((B * S, 3 * M * 3 * P), device='cuda', generator=gen)
                both[:, :2 * M * 3 * P] *= 4.0                # offsets of a few pixels
                sets.append((value, both))

            def core_hip(s):
                return vkn.ops.msda_sample(s[0], shapes, s[1][:, :2 * M * 3 * P], s[1][:, 2 * M * 3 * P:], ref, M, P)

            def core_torch(s):
                off = s[1][:, :2 * M * 3 * P].reshape(B, S, M, 3, P, 2)
                w = s[1][:, 2 * M * 3 * P:].reshape(B, S, M, 3 * P).softmax(-1).view(B, S, M, 3, P)
                loc = ref[None, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
                return msda_core_torch(s[0].view(B, S, M, D), shapes, loc, w)
            with torch.no_grad():
                worst = float((core_hip(sets[0]) - core_torch(sets[0])).abs().max())
                times = _ab((('core vkn_msda_sample_f32', core_hip), ('core grid_sample', core_torch)), sets, args.warmup, args.repeats)
            lines.append(f'  sampling core (largest difference between the arms {worst:.2e})')
            _report(lines, times, 'core vkn_msda_sample_f32', 'core grid_sample')
            # ---- (b) the whole eval forward
            fsets = [[torch.randn((B, c, h, w), device='cuda', generator=gen) for c, (h, w) in zip(IN_CHANNELS, sizes)] for _ in range(args.sets)]
            assert neck.fused_ok(fsets[0])
            with torch.no_grad():
                of, ot = neck.forward_fused(fsets[0]), neck.forward_torch(fsets[0])
                worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(of, ot))
                times = _ab((('forward_fused', neck.forward_fused), ('forward_torch', neck.forward_torch)), fsets, args.warmup, args.repeats)
            lines.append(f'  eval forward of the decoder (largest output difference between the arms, relative to the tensor\'s maximum: {worst:.2e})')
            _report(lines, times, 'forward_fused', 'forward_torch')
            lines.append('')
            print('\n'.join(lines[shown:]), flush=True)
            shown = len(lines)
            del sets, fsets, of, ot
            torch.cuda.empty_cache()
    text = '\n'.join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
