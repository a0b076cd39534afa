"""Bitwise A/B of the FPN block's kernels (csrc/vkn_fpn.hip, csrc/vkn_fpn_bwd.hip, csrc/vkn_convtile.h): one SHA-256 per output tensor,
to be compared between two builds of libvkn.so.  Run once per library, each in a fresh process; `--lib` makes this tree's Python load
another build (the headers must be the same).  Hashed, all on seeded operands:

  * every GN_CASES and BLOCK_CASES entry of tests/fpn_bwd_ref.py at every DY_SCALES: y, dr, dgamma, dbeta (and r, stats, dw, dx of a block);
  * the COND and STATS shapes of tests/test_gpu_fpn_conv_pins.py: the raw output and the statistics, modes raw / pos / norm / up;
  * vkn_localization_fpn_f32 with and without the loc / seg convs at B = 2, C = 64, levels (7, 135), (4, 68), (2, 34), (1, 17): two runs
    per row at the stride-8 grid, a partial run at every level.
The first line, behind a `#`, names the device and the library that was loaded; compare the rest (profiles/convtile_ab.txt).
BLOCK_CASES has since gained 'k3s1-32to32-33x65-g8-B1' and 'k3s2-32to32-9x131-g8': the tool now emits 8 tensors x 3 scales more for
them than profiles/convtile_ab.txt holds, which was not regenerated (its 501 lines are the A/B of the engine's move, at the cases of then).
The conv-only CONV_CASES of tests/fpn_bwd_ref.py are not hashed.

    python tools/convtile_ab.py [--lib PATH/libvkn.so] [--out FILE]
"""
import argparse
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import vkn_import  # noqa: E402

DEV = 'cuda:0'
FPN_LEVELS = ((7, 135), (4, 68), (2, 34), (1, 17))


def _cuda(*ts):
    return [t.to(DEV).contiguous() if t is not None else None for t in ts]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libvkn.so to load instead of this tree\'s')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('convtile_ab: needs the GPU')
    vkn = vkn_import.load()
    if args.lib:
        vkn._lib.LIBPATH = os.path.abspath(args.lib)
    ops = vkn.ops
    import fpn_bwd_ref as R
    import test_gpu_fpn_conv_pins as pins
    lines = []

    def put(name, **tensors):
        torch.cuda.synchronize()
        ops.workspace_status(DEV)
        for k, t in tensors.items():
            lines.append(f'{hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()}  {name} {k} {tuple(t.shape)}')

    for name in R.GN_CASES:
        c = R.gn_case(name)
        for scale in R.DY_SCALES:
            r, stats, gamma, beta, dy = _cuda(c['r'], c['stats'], c['gamma'], c['beta'], c['dy'] * scale)
            y = ops.gn_relu_apply(r, stats, gamma, beta)
            dr, dgamma, dbeta = ops.gn_relu_bwd(dy, r, stats, gamma, beta)
            put(f'gn[{name}-{scale:g}]', y=y, dr=dr, dgamma=dgamma, dbeta=dbeta)
    for name, shape in R.BLOCK_CASES.items():
        B, Cin, Cout, H, W, k, s, G = shape
        ops_cpu = R._block_operands(shape, R.SEEDS[0])
        for scale in R.DY_SCALES:
            x, w, gamma, beta, dy = _cuda(*ops_cpu[:4], ops_cpu[4] * scale)
            r, stats = ops.conv_gn(x, ops.conv_prepare(w), Cout, k, s, G)
            y = ops.gn_relu_apply(r, stats, gamma, beta)
            dr, dgamma, dbeta = ops.gn_relu_bwd(dy, r, stats, gamma, beta)
            dw = ops.conv_wgrad(dr, x, k, s)
            dx = ops.conv_dgrad(dr, ops.conv_prepare(w.flip(2, 3).transpose(0, 1).contiguous()), Cin, H, W, k, s)
            put(f'block[{name}-{scale:g}]', r=r, stats=stats, y=y, dr=dr, dgamma=dgamma, dbeta=dbeta, dw=dw, dx=dx)
    for mode, B, Ci, Co, H, W, ks, stride in pins.COND:
        x, pos, stats, gamma, beta, w = _cuda(*pins._cond_operands(mode, B, Ci, Co, H, W, ks, pins._g(900 + Ci + Co + len(mode))))
        out, st = ops.conv_gn(x, ops.conv_prepare(w), Co, ks, stride, 32, pos=pos, in_stats=stats, in_gamma=gamma, in_beta=beta, upsample=mode == 'up')
        put(f'cond[{mode}-{B}-{Ci}to{Co}-{H}x{W}-k{ks}s{stride}]', out=out, stats=st)
    for B, Ci, Co, H, W, ks, stride in pins.STATS:
        x, w = _cuda(*pins._stats_operands(B, Ci, Co, H, W, ks, pins._g(1700 + Co + W)))
        img = ops.conv_prepare(w)
        for G in (1, Co // 8, Co):
            out, st = ops.conv_gn(x, img, Co, ks, stride, G)
            put(f'stats[{B}-{Ci}to{Co}-{H}x{W}-k{ks}s{stride}-G{G}]', image=img, out=out, stats=st)
    B, C, G = 2, 64, 8
    g = torch.Generator().manual_seed(5150)
    ps = _cuda(*[torch.randn(B, C, h, w, generator=g) for h, w in FPN_LEVELS])
    pos5, = _cuda(0.5 * torch.randn(C, *FPN_LEVELS[3], generator=g))
    rows = [C] * 7 + [2 * C] + [C] * 2
    ws = _cuda(*[0.05 * torch.randn(n, C, k, k, generator=g) for n, k in zip(rows, [3] * 7 + [1] * 3)])
    gammas = _cuda(*[(0.5 + torch.rand(n, generator=g)) * (torch.randint(0, 2, (n,), generator=g) * 2 - 1) for n in rows])
    betas = _cuda(*[0.3 * torch.randn(n, generator=g) for n in rows])
    imgs = [ops.conv_prepare(w) for w in ws]
    for n in (8, 10):
        loc, sem = ops.localization_fpn(*ps, pos5, imgs[:n], gammas[:n], betas[:n], G)
        put(f'localization_fpn[{n} images]', loc=loc, sem=sem)
    path = vkn._lib.lib()._name
    with open(path, 'rb') as f:
        lines.insert(0, f'# {torch.cuda.get_device_name(0)}  library {os.path.relpath(path, ROOT)}  sha256 of the file {hashlib.sha256(f.read()).hexdigest()[:16]}')
    text = '\n'.join(lines)
    print(text)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as f:
            f.write(text + '\n')


if __name__ == '__main__':
    main()
