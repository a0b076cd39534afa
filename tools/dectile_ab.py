"""Bitwise and timing A/B of the decode tile engine's kernels (csrc/vkn_dectile.h: k_decode_mfma of csrc/vkn_decode.hip and
k_init_pass of csrc/vkn_init.hip), to be compared between two builds of libvkn.so.  Run once per library, each in a fresh process;
`--lib` makes this tree's Python load another build (the headers must be the same).

Default: one SHA-256 per output tensor, all on seeded operands:
  * mask_decode_planes at every arm of the engine (ARMS below: staging with few / many items and dead rows, one to four n-blocks, a
    ragged last n-block, two launches, the row split over blockIdx.z at 1 and 2 n-blocks and off, a ragged last pixel tile), and at
    N = 117, C = 256 with x in fp32, f16 and bf16;
  * mask_decode_planes_wg under budgets 1, 192 and 100000; mask_decode with out_scale;
  * kernel_init at the six cases of test_kernel_init_one_pass_equals_the_separate_form_bit_for_bit, one pass and the separate form (whose
    decodes run on frame-shared planes), all four outputs;
  * the video_cfg golden head under VKN_FLAG_BITS_HANDOFF (vkn_launch_decode_bits) and VKN_FLAG_LOGITS_HANDOFF.
`--time`: instead, the median in us of 20 timed calls after 5 (HIP events around each call) of mask_decode_planes at N = 117, C = 256,
128 x 256, B = 1, 8, 32 with fp32 and bf16 x, and of kernel_init at Np = 100, ncls = 19, C = 256, 128 x 256, B = 1, 8, 32.
The first line, behind a `#`, names the device and the library that was loaded; compare the rest (profiles/dectile_ab.txt).

    python tools/dectile_ab.py [--time] [--lib PATH/libvkn.so] [--out FILE]
"""
import argparse
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import torch  # noqa: E402

import vkn_import  # noqa: E402

DEV = 'cuda:0'
# (B, N, C, P): what of the engine the shape reaches
ARMS = [(1, 20, 32, 128),      # staging with fewer items than threads, one n-block
        (1, 100, 32, 128),     # row split over blockIdx.z, one n-block per workgroup (B G2 <= 64)
        (65, 100, 32, 128),    # ... two n-blocks per workgroup (B G2 <= 128)
        (129, 100, 32, 128),   # ... off (B G2 > 128): four n-blocks
        (2, 33, 64, 66),       # two n-blocks, the second ragged; a ragged pixel tile
        (2, 96, 64, 2048),     # three n-blocks, several tiles per wave
        (3, 129, 256, 130),    # two launches (4 + 1 n-blocks), more than 4 x 512 staging items, dead rows, ragged last pixel tile
        (1, 117, 256, 7488),   # a KITTI-STEP frame
        (2, 117, 256, 32768)]  # two cfg2 frames: the row split at two n-blocks at the real size
INIT = [(2, 100, 19, 2, 256, 128, 256, True, True), (3, 100, 19, 2, 256, 16, 32, True, False), (1, 127, 1, 0, 256, 8, 16, False, True),
        (2, 97, 31, 11, 128, 8, 24, True, True), (2, 12, 5, 2, 64, 8, 16, True, True), (1, 20, 12, 3, 256, 16, 16, False, False)]
XDT = dict(fp32=torch.float32, f16=torch.float16, bf16=torch.bfloat16)


def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _decode_operands(ops, B, N, C, P, seed, dt=torch.float32):
    x = _rand((B, C, 1, P), seed).to(dt)
    hi, lo = ops.split_planes(_rand((B, N, C), seed + 1, 0.05))
    return x, hi, lo, _rand((B, N), seed + 2)


def _init_operands(B, Np, ncls, C, H, W):
    return (_rand((B, C, H, W), 511), _rand((B, C, H, W), 512), _rand((Np, C, 1, 1), 513, 0.05), _rand((ncls, C, 1, 1), 514, 0.05),
            _rand((ncls,), 515))


def hashes(vkn, put):
    ops = vkn.ops
    for i, (B, N, C, P) in enumerate(ARMS):
        x, hi, lo, kb = _decode_operands(ops, B, N, C, P, 100 + 10 * i)
        put(f'decode_planes[B{B} N{N} C{C} P{P}]', bias=ops.mask_decode_planes(x, hi, lo, N, kb), nobias=ops.mask_decode_planes(x, hi, lo, N))
    for name, dt in XDT.items():
        for B, P in ((2, 512), (1, 32768)):
            x, hi, lo, kb = _decode_operands(ops, B, 117, 256, P, 300, dt)
            put(f'decode_planes[{name} B{B} N117 C256 P{P}]', out=ops.mask_decode_planes(x, hi, lo, 117, kb))
    x, hi, lo, kb = _decode_operands(ops, 2, 117, 256, 2560, 400)
    for budget in (1, 192, 100000):
        put(f'decode_planes_wg[budget {budget} B2 N117 C256 P2560]', out=ops.mask_decode_planes_wg(x, hi, lo, 117, budget, bias=kb))
    for B, N, C, P in ((2, 117, 256, 512), (1, 33, 64, 130)):
        x, k, kb = _rand((B, C, 1, P), 500), _rand((B, N, C), 501, 0.05), _rand((B, N), 502)
        put(f'decode[out_scale 2^-7 B{B} N{N} C{C} P{P}]', out=ops.mask_decode(x, k, kb, out_scale=torch.tensor(2.0 ** -7, device=DEV)))
    for B, Np, ncls, nth, C, H, W, cat, seg in INIT:
        loc, sem, iw, sw, sb = _init_operands(B, Np, ncls, C, H, W)
        for form, fl in (('onepass', 0), ('separate', ops.FLAG_INIT_SEPARATE)):
            out = ops.kernel_init(loc, sem, iw, sw, sb, nth, cat, True, want_seg_preds=seg, flags=fl)
            put(f'kernel_init[{form} B{B} Np{Np} ncls{ncls} nth{nth} C{C} {H}x{W} cat{int(cat)} seg{int(seg)}]',
                **{k: v for k, v in zip(('proposal_feats', 'x_feats', 'mask_preds', 'seg_preds'), out) if v is not None})
    from helpers import load_golden, make_case
    from test_host_logic import _cfg
    _, case = load_golden('video_cfg')
    head = vkn.build_head(_cfg(True, C=case['C'], heads=case['heads'], ffn=case['ffn'], ncls=case['ncls'], n_thing=case['n_thing'],
                               n_stuff=case['n_stuff'], S=case['S'], up=case['up'], nprop=case['nprop']))
    _, sd, x, pf, mp, prev = make_case(case)
    head.load_state_dict(sd, strict=True)
    head = head.to(DEV).eval()
    with torch.no_grad():
        for name, fl in (('bits', ops.FLAG_BITS_HANDOFF), ('logits', ops.FLAG_LOGITS_HANDOFF)):
            out = head._head_forward(x.to(DEV), pf.to(DEV), mp.to(DEV), prev.to(DEV), want_track=True, flags=fl)
            put(f'head[video_cfg {name} hand-off]', **{k: v for k, v in zip(('obj', 'cls', 'masks', 'scaled', 'track'), out) if v is not None})


def _median_us(fn, iters=20, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    return statistics.median(ts)


def timings(vkn, lines):
    ops = vkn.ops
    H, W = 128, 256
    for name in ('fp32', 'bf16'):
        for B in (1, 8, 32):
            x, hi, lo, kb = _decode_operands(ops, B, 117, 256, H * W, 700, XDT[name])
            out = torch.empty((B, 117, 1, H * W), dtype=torch.float32, device=DEV)
            lines.append(f'{_median_us(lambda: ops.mask_decode_planes(x, hi, lo, 117, kb, out=out)):10.1f}  decode_planes {name} B{B}')
            del x, out
    for B in (1, 8, 32):
        loc, sem, iw, sw, sb = _init_operands(B, 100, 19, 256, H, W)
        lines.append(f'{_median_us(lambda: ops.kernel_init(loc, sem, iw, sw, sb, 2, True, True)):10.1f}  kernel_init B{B}')
        del loc, sem


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libvkn.so to load instead of this tree\'s')
    ap.add_argument('--time', action='store_true', help='the timing rows (median us) instead of the hashes')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('dectile_ab: needs the GPU')
    vkn = vkn_import.load()
    if args.lib:
        vkn._lib.LIBPATH = os.path.abspath(args.lib)
    lines = []

    def put(name, **tensors):
        torch.cuda.synchronize()
        vkn.ops.workspace_status(DEV)
        for k, t in tensors.items():
            lines.append(f'{hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()}  {name} {k} {tuple(t.shape)}')

    if args.time:
        timings(vkn, lines)
    else:
        hashes(vkn, put)
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
