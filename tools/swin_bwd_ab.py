"""Swin backbone in training, A/B in one process: forward PLUS backward of the attention span of a `SwinTransformerBlock`
(video-k-net_amd/swin.py) with `fused='train'` (qkv Linear + `vkn_swin_window_attn_f32` + proj forward, `vkn_wattn_bwd_f32` in the backward,
the Linears by torch autograd) against the torch composition's same span (`fused=False`: pad, roll, partition, qkv Linear, bias gather, mask
add, softmax, P V, proj, reverse, roll back, crop, all by torch autograd), from after norm1 to before the residual, on the same parameters;
then forward plus backward of the whole Swin-B backbone in train mode, `fused='train'` against `fused=False`, at B = 1 and 2.

Shapes: the four stage maps of Swin-B (128 ... 1024 channels, 4 ... 32 heads) and Swin-L (192 ... 1536, 6 ... 48) at a KITTI-STEP frame
(384 x 1248) and a COCO frame (800 x 1344), unshifted and shifted blocks, B = 1 and 2.

Per shape: warm-up of both arms, then `--passes` passes of `--repeats` rounds that alternate the arms; every call (forward, backward from a
fixed output gradient, gradients dropped) is timed with its own pair of HIP events (device time), on inputs that rotate through as many
seeded copies as exceed 256 MiB.  Reported per arm: the median of all rounds, the SPREAD = (largest - smallest) / middle of the passes'
medians, and PEAK = `torch.cuda.max_memory_allocated` over one forward + backward minus what was allocated before it (what the step adds:
activations saved for the backward and its temporaries).  The backward kernel alone is timed the same way on rotating (qkv, dout) pairs
and set against its floor: one read of qkv and dout plus one write of dqkv at 8.0 TB/s (the HBM3E specification).

The verdict line says whether the 'train' span is faster at EVERY shape by more than the larger spread of the two arms: `FUSED_DEFAULT`'s
rule, applied to the question whether 'train' would qualify as a default.  Writes profiles/swin_bwd_ab.txt (or --out).

    python tools/swin_bwd_ab.py [--warmup 3] [--repeats 7] [--passes 3] [--quick] [--out FILE]
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


def _peak(fn):
    """MiB that one call of fn adds at its peak to what is allocated before it"""
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def _step(module_params, run, gy):
    """forward + backward from the fixed output gradient(s) gy; the gradients are dropped, not accumulated"""
    def step(x):
        for p in module_params:
            p.grad = None
        x.grad = None
        out = run(x)
        if isinstance(out, tuple):
            torch.autograd.backward(out, gy)
        else:
            out.backward(gy)
    return step


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=7)
    ap.add_argument('--passes', type=int, default=3)
    ap.add_argument('--quick', action='store_true', help='one frame, one model, B = 1: a rehearsal')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'swin_bwd_ab.txt'))
    args = ap.parse_args()
    assert torch.cuda.is_available(), 'swin_bwd_ab.py measures on the MI355X: there is no CPU arm'
    vkn = vkn_import.load()
    from video_k_net_amd import swin
    dev = torch.device('cuda:0')
    lines = [f'swin_bwd_ab: {torch.cuda.get_device_name(0)}; warmup {args.warmup}, {args.passes} passes x {args.repeats} alternating rounds, device events, ms',
             'span = forward + backward of qkv Linear + window attention + proj, after norm1, before the residual; peak = MiB the step adds',
             'kernel = vkn_wattn_bwd_f32 alone (both launches); floor = (qkv + dout + dqkv bytes) / 8.0 TB/s', '']
    frames = dict(list(FRAMES.items())[:1]) if args.quick else FRAMES
    models = dict(list(MODELS.items())[:1]) if args.quick else MODELS

    def emit(line):
        """print the line and rewrite the report: a run that is cut short leaves what it has measured"""
        lines.append(line)
        print(line, flush=True)
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write('\n'.join(lines) + '\n')
    # forward + backward of the whole Swin-B backbone in train mode (stochastic depth at its config rate in both arms)
    embed, depths, heads = MODELS['swin_b']
    nets = {}
    for fused in ('train', False):
        torch.manual_seed(1)
        nets[fused] = swin.SwinTransformerDIY(embed_dims=embed, depths=list(depths), num_heads=list(heads), drop_path_rate=0.3, fused=fused).to(dev).train()
    for fname, (fh, fw) in frames.items():
        for B in ((1,) if args.quick else (1, 2)):
            imgs = [torch.randn((B, 3, fh, fw), device=dev) for _ in range(3)]
            with torch.no_grad():
                gy = tuple(torch.randn_like(o) for o in nets[False](imgs[0]))
            arms = tuple((str(f), _step(list(nets[f].parameters()), nets[f], gy)) for f in ('train', False))
            r = _ab(arms, imgs, 2, max(3, args.repeats // 2), args.passes)
            peaks = {name: _peak(lambda: fn(imgs[0])) for name, fn in arms}
            paths = sorted({b.last_path for b in nets['train'].modules() if isinstance(b, swin.SwinTransformerBlock)})
            (tf, sf), (tt, st) = r['train'], r['False']
            emit(f'{fname} swin_b whole forward + backward B {B}: train {tf:8.3f} (spread {sf:5.1%}, peak {peaks["train"]:8.1f})  torch {tt:8.3f} (spread {st:5.1%}, '
                         f'peak {peaks["False"]:8.1f})  torch/train {tt / tf:5.2f}  |  paths of the train arm {paths}')
            del imgs, gy
    emit('')
    worst, all_faster = None, True
    torch.manual_seed(0)
    for fname, (fh, fw) in frames.items():
        for mname, (embed, _, heads) in models.items():
            for stage, (H, W) in enumerate(stage_maps(fh, fw)):
                dim, nh = embed * 2 ** stage, heads[stage]
                for shift in (0, WINDOW // 2):
                    blk = swin.SwinTransformerBlock(dim=dim, num_heads=nh, window_size=WINDOW, shift_size=shift, fused='train').to(dev).train()
                    torch.nn.init.normal_(blk.attn.relative_position_bias_table, std=0.5)
                    blk.H, blk.W = H, W
                    mask = swin.shift_attention_mask(H, W, WINDOW, WINDOW // 2, dev)
                    params = list(blk.attn.parameters())
                    for B in ((1,) if args.quick else (1, 2)):
                        n = _copies(B * H * W * dim * 4)
                        xs = [torch.randn((B, H * W, dim), device=dev).requires_grad_() for _ in range(n)]
                        assert blk.fused_train_path(xs[0])
                        gy = torch.randn((B, H * W, dim), device=dev)
                        arms = (('train', _step(params, lambda x: blk.attention_fused(x, True), gy)),
                                ('torch', _step(params, lambda x: blk.attention_torch(x, mask), gy)))
                        r = _ab(arms, xs, args.warmup, args.repeats, args.passes)
                        peaks, grads = {}, {}
                        for name, fn in arms:
                            peaks[name] = _peak(lambda: fn(xs[0]))
                            grads[name] = [xs[0].grad.clone()] + [p.grad.clone() for p in params]
                        err = max(((a - b).abs().max() / b.abs().max().clamp_min(1e-30)).item() for a, b in zip(grads['train'], grads['torch']))
                        del xs, grads
                        a = blk.attn
                        m = _copies(B * H * W * 4 * dim * 4)
                        with torch.no_grad():
                            qs = [(torch.randn((B, H * W, 3 * dim), device=dev), torch.randn((B, H * W, dim), device=dev)) for _ in range(m)]
                            k = _ab((('kernel', lambda s: vkn.ops.swin_window_attention_bwd(s[0], a.qkv.bias, a.relative_position_bias_table, s[1], H, W, nh, WINDOW,
                                                                                           shift, a.scale)),), qs, args.warmup, args.repeats, args.passes)['kernel']
                        del qs
                        floor_ms = B * H * W * 7 * dim * 4 / HBM_BYTES_PER_S * 1e3
                        (tf, sf), (tt, st) = r['train'], r['torch']
                        spread = max(sf, st)
                        faster = tf * (1 + spread) < tt
                        all_faster &= faster
                        if worst is None or tt / tf < worst[0]:
                            worst = (tt / tf, f'{fname} {mname} stage {stage} shift {shift} B {B}')
                        emit(f'{fname} {mname} stage {stage} {H:>3}x{W:<3} C {dim:<4} heads {nh:<2} shift {shift} B {B}: train {tf:8.3f} (spread {sf:5.1%}, peak {peaks["train"]:8.1f})  '
                                     f'torch {tt:8.3f} (spread {st:5.1%}, peak {peaks["torch"]:8.1f})  torch/train {tt / tf:5.2f}  {"faster" if faster else "NOT faster"}  |  '
                                     f'kernel {k[0]:7.3f} floor {floor_ms:6.3f} share {floor_ms / k[0]:5.1%}  |  max rel |train - torch| over the gradients {err:.1e}')
    emit('')
    emit(f"'train' span faster than the torch span by more than the spread at every shape: {'YES' if all_faster else 'NO'}; the smallest torch/train is "
              f'{worst[0]:.2f} ({worst[1]})')


if __name__ == '__main__':
    main()
