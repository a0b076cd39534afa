"""The tracking link beside the last decode: whole head steps of bench.py's workload (one clip call: 3 stages + link + x4 upsample),
back-to-back, by how many workgroups the last decode takes and where the side-stream link joins.

  --probe   the prize before the code (debug library): VKN_DECODE_PXWG narrows the last decode, VKN_FLAG_JOIN_EARLY joins the link
            before the upsample.  Variants alternate inside one process; ms per call.
  --ab      the built policy (release library): default / VKN_FLAG_LINK_RESERVE (forced) / VKN_FLAG_LINK_NO_RESERVE (the parent's launches)
  --trace V run variant V alone for a few steps (under rocprofv3 --kernel-trace; summarise with tools/summarize_prof.py)

python tools/link_beside_decode.py --probe [--frames 32,16,8] [--rounds 3]"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402  (the flagship's head and inputs)
import vkn_import  # noqa: E402

vkn = vkn_import.load()
DEV = torch.device('cuda', 0)
P = bench.CFG2['H'] * bench.CFG2['W']


def pxwg_for(B, wgs):
    """pixels per decode workgroup for at most `wgs` workgroups over B frames, in the kernel's 512-px granularity"""
    g2 = max(1, wgs // B)
    return (-(-P // g2) + 511) // 512 * 512


def timeit(fn, iters, warm):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters   # ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--probe', action='store_true')
    ap.add_argument('--ab', action='store_true')
    ap.add_argument('--trace', default=None, help='variant name, e.g. default, wg224+early, reserve, noreserve')
    ap.add_argument('--frames', default='32,16,8')
    ap.add_argument('--rounds', type=int, default=3)
    ap.add_argument('--iters', type=int, default=60)
    ap.add_argument('--x-storage', default='fp32', choices=['fp32', 'fp16', 'bf16'], help='storage type of the feature map')
    args = ap.parse_args()
    debug = args.probe or (args.trace and args.trace.startswith(('wg', 'default-debug')))
    if debug:
        if not os.path.exists(vkn._lib.DEBUG_LIBPATH):
            vkn._lib.build_debug()
        vkn._lib.use_debug()
    ops = vkn.ops
    head = bench.build_head(vkn, DEV)
    N, C = bench.CFG2['N'], bench.CFG2['C']
    packs = [h.stage_pack(DEV) for h in head.mask_head]
    first_prev = torch.zeros(1, N, C, device=DEV)
    print(f'device: {torch.cuda.get_device_name(0)}; library: {"debug" if debug else "release"} build; x stored as {args.x_storage}')
    for B in [int(f) for f in args.frames.split(',')]:
        x, pf, mp = bench.synth_inputs(B, DEV, 0)
        pf = pf.reshape(B, N, C)
        x = x.to({'fp32': torch.float32, 'fp16': torch.float16, 'bf16': torch.bfloat16}[args.x_storage])
        dims = head.mask_head[-1].make_dims(B, N, bench.CFG2['H'], bench.CFG2['W'])
        if debug:
            variants = [('default-debug', 0, 0)]
            for wgs in (224, 192, 160):
                px = pxwg_for(B, wgs)
                real = B * (-(-P // px))
                variants.append((f'wg{wgs}+early', px, ops.FLAG_JOIN_EARLY))
                variants.append((f'wg{wgs}', px, 0))
                print(f'B={B}: budget {wgs} -> VKN_DECODE_PXWG={px}: {real} workgroups')
        else:
            variants = [('default', 0, 0), ('reserve', 0, ops.FLAG_LINK_RESERVE), ('noreserve', 0, ops.FLAG_LINK_NO_RESERVE),
                        ('reserve+early', 0, ops.FLAG_LINK_RESERVE | ops.FLAG_JOIN_EARLY), ('noreserve+early', 0, ops.FLAG_LINK_NO_RESERVE | ops.FLAG_JOIN_EARLY)]

        def run(v):
            _, px, fl = v
            if debug:
                os.environ['VKN_DECODE_PXWG'] = str(px)
            with torch.no_grad():
                return ops.head_forward(dims, packs, x, pf, mp, None, bench.CFG2['up'], clip_first_prev=first_prev, flags=fl)

        if args.trace:
            v = [v for v in variants if v[0] == args.trace][0]
            timeit(lambda: run(v), 8, 4)
            print(f'traced {v[0]} at B={B}')
            continue
        for r in range(args.rounds):
            row = []
            for v in variants:
                t = timeit(lambda: run(v), args.iters, 10)
                row.append(f'{v[0]} {t:6.3f}')
            print(f'B={B:3d} round {r}  ' + '   '.join(row), flush=True)
    os.environ.pop('VKN_DECODE_PXWG', None)


if __name__ == '__main__':
    main()
