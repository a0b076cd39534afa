"""Deformable-attention neck, TRAINING A/B in one process, at the encoder level sizes of a COCO frame (800 x 1344: 100 x 168, 50 x 84,
25 x 42) and a YouTube-VIS frame (360 x 640: 45 x 80, 23 x 40, 12 x 20), B = 1 and 2, the shipped widths (256 channels, 8 heads,
3 levels, 4 points, 6 layers):
  (a) forward + backward of the sampling core: `autograd.msda_sample` (vkn_msda_sample_f32 + vkn_msda_sample_bwd_f32,
      include/vkn_msda_train.h) against torch's `F.grid_sample` composition and its autograd, on the same operands;
  (b) forward + backward of the whole `MSDeformAttnPixelDecoder`: `fused_backward=True` against `forward_torch` (the flag off), the
      same module and parameters;
  (c) the fixed-point scatter of dvalue alone: its kernel time (torch's profiler; where that finds no kernel, the whole backward entry
      as an upper bound of the time) and the bytes it adds per second, contributions x 8 B, beside the 1.3 TB/s measured for float atomics.

The protocol is tools/msda_ab.py's: warm-up of both arms, then `--repeats` rounds that alternate the arms; every call is timed with
its own pair of HIP events, on inputs that rotate through `--sets` seeded sets; median, minimum, maximum and the 10 % .. 90 % spread
per arm.  The flag qualifies as the default by (b): only if it is faster at all four points by more than the larger of the two arms'
spreads.  The gradient differences printed beside the timings are NOT an accuracy figure: the random offsets put a few of the
millions of points within fp32 rounding of an integer coordinate, where doff is discontinuous and either side is right
(tests/test_gpu_msda_bwd.py judges accuracy, on offsets nudged away from the integers).
Writes profiles/msda_bwd_ab.txt (or --out).

    python tools/msda_bwd_ab.py [--warmup 3] [--repeats 15] [--sets 3] [--only coco|ytvis] [--out FILE]
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
M, D, P, L = 8, 32, 4, 3
FLOAT_ATOMIC_TBS = 1.3


def _time(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def _ab(arms, sets, warmup, repeats):
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


def _spread(v):
    v = sorted(v)
    return v[min(len(v) - 1, round(0.9 * (len(v) - 1)))] - v[round(0.1 * (len(v) - 1))]


def _report(lines, times, first, second):
    med = {k: statistics.median(v) for k, v in times.items()}
    for k, v in times.items():
        lines.append(f'    {k:<34} median {med[k]:9.3f}  min {min(v):9.3f}  max {max(v):9.3f}  10-90 % spread {_spread(v):7.3f}')
    lines.append(f'    {first} / {second} (medians) {med[first] / med[second]:.3f}')
    return med[second] - med[first], max(_spread(v) for v in times.values())


def _contributions(shapes, off, ref):
    """how many (point, corner) pairs lie inside their level: each adds D int64 to the accumulator"""
    n, Q = 0, ref.shape[0]
    for l, (h, w) in enumerate(shapes):
        x = (ref[None, :, None, l, None, 0] + off[:, :, :, l, :, 0] / w) * w - 0.5
        y = (ref[None, :, None, l, None, 1] + off[:, :, :, l, :, 1] / h) * h - 0.5
        ok = (y > -1) & (x > -1) & (y < h) & (x < w)
        x0, y0 = x.floor(), y.floor()
        for dy in (0, 1):
            for dx in (0, 1):
                n += int((ok & (y0 + dy >= 0) & (y0 + dy <= h - 1) & (x0 + dx >= 0) & (x0 + dx <= w - 1)).sum())
    return n


def _scatter_ms(fn, repeats):
    """median kernel time of k_msda_bwd_scatter over `repeats` calls of fn, by torch's profiler; None where it reports no such kernel"""
    try:
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            for _ in range(repeats):
                fn()
            torch.cuda.synchronize()
        us = [e.device_time_total if hasattr(e, 'device_time_total') else e.cuda_time_total for e in prof.events()
              if 'k_msda_bwd_scatter' in e.name]
        us = [u for u in us if u > 0]
        return statistics.median(us) / 1e3 if us else None
    except Exception as e:                                       # noqa: BLE001 — a missing profiler is reported, not fatal: the entry's time bounds it
        print(f'msda_bwd_ab: torch.profiler unavailable ({e!r})', flush=True)
        return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=15)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--only', default=None, help='coco or ytvis')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'msda_bwd_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('msda_bwd_ab: needs the GPU (a timing taken elsewhere says nothing)')
    vkn = vkn_import.load()
    from video_k_net_amd.msdeform_decoder import msda_core_torch
    torch.manual_seed(0)
    neck = vkn.MSDeformAttnPixelDecoder(fused_backward=True)
    neck.init_weights()
    with torch.no_grad():                                        # the init leaves every offset weight at zero: spread the samples as a trained neck does
        for layer in neck.encoder.layers:
            layer.attentions[0].sampling_offsets.weight.normal_(0, 0.05)
            layer.attentions[0].attention_weights.weight.normal_(0, 0.1)
    neck = neck.cuda().train()
    params = [p for p in neck.parameters()]

    def set_flag(on):
        for layer in neck.encoder.layers:
            layer.attentions[0].fused_backward = on

    lines = [f'tool msda_bwd_ab  device {torch.cuda.get_device_name(0)}  C 256  heads {M}  levels {L}  points {P}  layers 6  warmup {args.warmup}  '
             f'repeats {args.repeats}  input sets {args.sets}', 'ms per call of forward + backward (HIP events around each call; arms alternate)',
             'gradient differences between the arms: no accuracy figure (doff is discontinuous at integer coordinates, which random offsets hit)', '']
    shown, verdict = 0, []
    n_off, n_log = 2 * M * L * P, M * L * P
    for name, sizes in FRAMES.items():
        if args.only and args.only not in name:
            continue
        shapes = [sizes[3], sizes[2], sizes[1]]                  # the encoder's order: low to high resolution
        S = sum(h * w for h, w in shapes)
        for B in (1, 2):
            gen = torch.Generator(device='cuda').manual_seed(1)
            lines.append(f'{name}  B {B}  levels {shapes}  S = Q = {S}  accumulator {B * S * M * D * 8 / 2 ** 20:.1f} MiB')
            _, ref = neck.shape_constants(shapes, torch.device('cuda', 0))
            wh = torch.tensor([[w, h] for h, w in shapes], dtype=torch.float32, device='cuda')
            sets = []
            for _ in range(args.sets):
                value = torch.randn((B, S, M * D), device='cuda', generator=gen).requires_grad_(True)
                both = torch.randn((B * S, n_off + n_log), device='cuda', generator=gen)
                both[:, :n_off] *= 4.0                            # offsets of a few pixels
                sets.append((value, both.requires_grad_(True), torch.randn((B, S, M * D), device='cuda', generator=gen)))

            def core_hip(s):
                out = vkn.autograd.msda_sample(s[0], shapes, s[1][:, :n_off], s[1][:, n_off:], ref, M, P)
                return torch.autograd.grad(out, (s[0], s[1]), s[2])

            def core_torch(s):
                off = s[1][:, :n_off].reshape(B, S, M, L, P, 2)
                w = s[1][:, n_off:].reshape(B, S, M, L * P).softmax(-1).view(B, S, M, L, P)
                loc = ref[None, :, None, :, None, :] + off / wh[None, None, None, :, None, :]
                out = msda_core_torch(s[0].view(B, S, M, D), shapes, loc, w)
                return torch.autograd.grad(out, (s[0], s[1]), s[2])
            ga, gb = core_hip(sets[0]), core_torch(sets[0])
            worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(ga, gb))
            times = _ab((('core autograd.msda_sample', core_hip), ('core grid_sample + autograd', core_torch)), sets, args.warmup, args.repeats)
            lines.append(f'  (a) sampling core, forward + backward (largest gradient difference between the arms, relative to the tensor\'s maximum: {worst:.2e})')
            _report(lines, times, 'core autograd.msda_sample', 'core grid_sample + autograd')
            del ga, gb
            # ---- (c) the scatter alone
            with torch.no_grad():
                v, b_, dout = (t.detach() for t in sets[0])
                n = _contributions(shapes, b_[:, :n_off].reshape(B, S, M, L, P, 2), ref) * D
                call = lambda: vkn.ops.msda_sample_bwd(v, shapes, b_[:, :n_off], b_[:, n_off:], ref, dout, M, P)      # noqa: E731
                for _ in range(args.warmup):
                    call()
                entry = statistics.median(_time(call)[0] for _ in range(args.repeats))
                kern = _scatter_ms(call, args.repeats)
            gb_added = n * 8 / 1e9
            lines.append(f'  (c) dvalue scatter: {n} int64 adds = {gb_added:.3f} GB added; whole backward entry (memset, 5 kernels) median {entry:.3f} ms')
            if kern is not None:
                lines.append(f'      k_msda_bwd_scatter alone (profiler) median {kern:.3f} ms -> {gb_added / kern:.3f} TB/s of added bytes '
                             f'(float atomics, measured elsewhere: {FLOAT_ATOMIC_TBS} TB/s)')
            else:
                lines.append(f'      kernel time not available (no profiler record); from the whole entry: >= {gb_added / entry:.3f} TB/s of added bytes '
                             f'(float atomics, measured elsewhere: {FLOAT_ATOMIC_TBS} TB/s)')
            # ---- (b) the whole decoder, forward + backward
            fsets = [[torch.randn((B, c, h, w), device='cuda', generator=gen) for c, (h, w) in zip(IN_CHANNELS, sizes)] for _ in range(args.sets)]

            def step(on):
                def run(feats):
                    set_flag(on)
                    outs = neck(feats)
                    return torch.autograd.grad(sum(o.sum() for o in outs), params)
                return run
            g_on, g_off = step(True)(fsets[0]), step(False)(fsets[0])
            worst = max(float((a - b).abs().max() / b.abs().max().clamp_min(1e-30)) for a, b in zip(g_on, g_off))
            del g_on, g_off
            times = _ab((('decoder fused_backward=True', step(True)), ('decoder forward_torch', step(False))), fsets, args.warmup, args.repeats)
            lines.append(f'  (b) the decoder, forward + backward (largest parameter-gradient difference between the arms, relative to the tensor\'s maximum: {worst:.2e})')
            gain, spread = _report(lines, times, 'decoder fused_backward=True', 'decoder forward_torch')
            verdict.append(gain > spread)
            lines.append(f'    flag on is faster by {gain:.3f} ms; larger 10-90 % spread of the two arms {spread:.3f} ms -> {"faster" if gain > spread else "NOT faster"} beyond the spread')
            lines.append('')
            print('\n'.join(lines[shown:]), flush=True)
            shown = len(lines)
            del sets, fsets
            torch.cuda.empty_cache()
    lines.append(f'(b) faster beyond the spread at {sum(verdict)} of {len(verdict)} points -> the measurement '
                 f'{"qualifies" if len(verdict) == 4 and all(verdict) else "does not qualify"} fused_backward=True as the default')
    print(lines[-1], flush=True)
    text = '\n'.join(lines)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
