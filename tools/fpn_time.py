"""Localization FPN + loc / seg convs: ms per frame of the HIP call (vkn_localization_fpn_f32) and of the same module's torch
composition (fp32, MIOpen), at B = 1 and 8, on a Cityscapes (1024 x 2048) and a KITTI-STEP (384 x 1248) frame.  Prints one JSON line.

    python tools/fpn_time.py [--warmup 3] [--iters 10] [--out FILE]
"""
import argparse
import copy
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

import vkn_import  # noqa: E402

SHIPPED = dict(type='SemanticFPNWrapper', in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
               upsample_times=2, num_aux_convs=1, cat_coors=False, fuse_by_cat=False,
               positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
               norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
FRAMES = {'cityscapes_1024x2048': (1024, 2048), 'kitti_step_384x1248': (384, 1248)}


def _time(fn, warmup, iters):
    for _ in range(warmup):
        fn()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--warmup', type=int, default=3)
    ap.add_argument('--iters', type=int, default=10)
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    vkn = vkn_import.load()
    from importlib import import_module
    kh = import_module('video_k_net_amd.kernel_head')
    torch.manual_seed(0)
    m = vkn.registry.HEADS.build(copy.deepcopy(SHIPPED))
    m.init_weights()
    m = m.cuda().eval()
    ls = [kh._ConvGNReLU(256, 256, 1).cuda().eval() for _ in range(2)]
    res = {}
    with torch.no_grad():
        for name, (H, W) in FRAMES.items():
            for B in (1, 8):
                x = [torch.randn(B, 256, H // s, W // s, device='cuda') for s in (4, 8, 16, 32)]
                hip = _time(lambda: m.forward_fused(x, *ls), args.warmup, args.iters)
                vkn.ops.workspace_status()

                def torch_path():
                    out, aux = m.forward_torch(x)
                    return ls[0](out), ls[1](aux)
                tor = _time(torch_path, args.warmup, args.iters)
                res[f'{name}_B{B}'] = dict(hip_ms_per_frame=round(hip / B, 4), torch_ms_per_frame=round(tor / B, 4),
                                           speedup=round(tor / hip, 2))
                del x
                torch.cuda.empty_cache()
    line = json.dumps(dict(tool='fpn_time', device=torch.cuda.get_device_name(0), warmup=args.warmup, iters=args.iters, results=res))
    print(line)
    if args.out:
        with open(args.out, 'w') as f:
            f.write(line + '\n')


if __name__ == '__main__':
    main()
