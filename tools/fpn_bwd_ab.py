"""Localization FPN, one training forward + backward: `SemanticFPNWrapper(fused_backward=True)` (every ConvModule forward and backward in
HIP, include/vkn_fpn_train.h) against `fused_backward=False` (the torch composition: MIOpen convs, torch GroupNorm), on the same
parameters, at the level sizes of a KITTI-STEP (384 x 1248), a Cityscapes (1024 x 2048) and a VIP-Seg (720 x 1280, padded to 736) frame,
C = 256, B = 2.

Per size: warm-up of both arms, then `--repeats` rounds that alternate the arms in one process; every forward + backward is timed
with its own pair of HIP events, on inputs that rotate through `--sets` seeded sets (so that no arm re-reads what the other left in
the caches); the median and the minimum per arm are reported.  Writes profiles/fpn_bwd_ab.txt (or --out).

    python tools/fpn_bwd_ab.py [--warmup 3] [--repeats 20] [--sets 3] [--out FILE]
"""
import argparse
import copy
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vkn_import  # noqa: E402

SHIPPED = dict(type='SemanticFPNWrapper', in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
               upsample_times=2, num_aux_convs=1, cat_coors=False, fuse_by_cat=False,
               positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
               norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
FRAMES = {'kitti_step_384x1248': (384, 1248), 'cityscapes_1024x2048': (1024, 2048), 'vipseg_736x1280': (736, 1280)}
B = 2


def _step(mod, xs, gs):
    for p in mod.parameters():
        p.grad = None
    ins = [x.requires_grad_() for x in xs]
    for x in ins:
        x.grad = None
    outs = mod(ins)
    torch.autograd.backward(outs, gs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--repeats', type=int, default=20)
    ap.add_argument('--sets', type=int, default=3)
    ap.add_argument('--only', default=None, help='one frame name of FRAMES')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'fpn_bwd_ab.txt'))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('fpn_bwd_ab: needs the GPU (a timing taken elsewhere says nothing)')
    vkn = vkn_import.load()
    torch.manual_seed(0)
    plain = vkn.registry.HEADS.build(copy.deepcopy(SHIPPED))
    plain.init_weights()
    plain = plain.cuda().train()
    fused = vkn.registry.HEADS.build(dict(copy.deepcopy(SHIPPED), fused_backward=True)).cuda().train()
    fused.load_state_dict(plain.state_dict())
    arms = (('fused_backward=True', fused), ('fused_backward=False', plain))
    lines = [f'tool fpn_bwd_ab  device {torch.cuda.get_device_name(0)}  C 256  B {B}  warmup {args.warmup}  repeats {args.repeats}  '
             f'input sets {args.sets}', 'one forward + backward of SemanticFPNWrapper, ms (HIP events around each step; arms alternate)', '']
    for name, (H, W) in FRAMES.items():
        if args.only and name != args.only:
            continue
        gen = torch.Generator(device='cuda').manual_seed(1)
        sets = [[torch.randn((B, 256, H // s, W // s), device='cuda', generator=gen) for s in (4, 8, 16, 32)] for _ in range(args.sets)]
        gs = [torch.randn((B, 256, H // 8, W // 8), device='cuda', generator=gen) * 1e-3 for _ in range(2)]
        assert fused.train_fused_ok(sets[0])
        for _ in range(args.warmup):
            for _, mod in arms:
                _step(mod, sets[0], gs)
        vkn.ops.workspace_status()
        torch.cuda.synchronize()
        times = {arm: [] for arm, _ in arms}
        for i in range(args.repeats):
            for j, (arm, mod) in enumerate(arms if i % 2 == 0 else arms[::-1]):
                xs = sets[(2 * i + j) % args.sets]
                a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                a.record()
                _step(mod, xs, gs)
                b.record()
                b.synchronize()
                times[arm].append(a.elapsed_time(b))
        vkn.ops.workspace_status()
        # same parameters, same inputs: the two arms' outputs agree to the kernels' resolution.  (Their gradients are not compared here:
        # among the 10^7 pre-activations of a layer a few lie within rounding of zero, the arms round them to different sides, and one
        # flipped ReLU moves a weight gradient by a whole term; tests/test_gpu_fpn_bwd.py judges the gradients on inputs clear of that edge.)
        with torch.no_grad():
            of, op = fused.forward_train_fused(sets[0]), plain.forward_torch(sets[0])
        worst = max(float((a - b).abs().max() / b.abs().max()) for a, b in zip(of, op))
        med = {arm: statistics.median(t) for arm, t in times.items()}
        lines.append(f'{name}  levels {[(H // s, W // s) for s in (4, 8, 16, 32)]}')
        for arm, t in times.items():
            lines.append(f'  {arm:<22} median {med[arm]:9.3f}  min {min(t):9.3f}  max {max(t):9.3f}')
        lines.append(f'  fused / torch (medians) {med[arms[0][0]] / med[arms[1][0]]:.3f}   largest output difference between the arms, '
                     f'relative to the tensor\'s maximum: {worst:.2e}')
        lines.append('')
        del sets, gs, of, op
        for mod in (fused, plain):
            for p in mod.parameters():
                p.grad = None
        torch.cuda.empty_cache()
    text = '\n'.join(lines)
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write(text + '\n')


if __name__ == '__main__':
    main()
