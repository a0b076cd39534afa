"""A/B of the ground-truth preparation of one training step, from the same HOST inputs, upload included: `GtPrep`'s fused path
(csrc/vkn_gtprep.hip: byte upload, class presence, one host read, one bank fill) against this package's own torch composition (the
reference's ops: pad, `torch.unique` + a `==` pass per class, bilinear `F.interpolate`; it also uploads bytes, where the reference
uploads fp32 masks).  Wall time per call with a device synchronisation at its end, after a warm-up; the values are compared first.  A third figure
is the fused call on bytes that already live on the device: the difference is the upload.

    KITTI-STEP  384 x 1248, stride 2, 2 images, 10 things and 12 stuff classes per image
    Cityscapes  1024 x 2048, stride 4, 1 image, 20 things and 11 stuff classes

Each shape runs in a child process of its own under a time limit; the first failure ends the run.

    python tools/gt_prep_ab.py [--calls 200] [--warmup 20] [--out profiles/gt_prep_ab.txt]
"""
import argparse
import datetime
import os
import statistics
import subprocess
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import vkn_import  # noqa: E402

HBM = 6.3e12      # bytes / s: the rate the other floors of DESIGN.md use
SHAPES = {
    'kitti_step': dict(dataset='kitti_step', pad=(384, 1248), stride=2, B=2, G=10, T=2, S=17,
                       classes=[0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 12, 11, 13, 255]),
    'cityscapes': dict(dataset='cityscapes', pad=(1024, 2048), stride=4, B=1, G=20, T=8, S=11, classes=list(range(19)) + [255]),
}


class Bitmap:
    def __init__(self, masks):
        self.masks, self.height, self.width = masks, int(masks.shape[1]), int(masks.shape[2])


def inputs(cfg):
    rng = np.random.default_rng(1)
    B, (H, W), G = cfg['B'], cfg['pad'], cfg['G']
    masks = []
    for _ in range(B):
        m = np.zeros((G, H, W), np.uint8)
        for g in range(G):
            y, x = rng.integers(0, H - 64), rng.integers(0, W - 64)
            m[g, y:y + rng.integers(16, H // 2), x:x + rng.integers(16, W // 2)] = 1
        masks.append(m)
    classes = np.asarray(cfg['classes'])
    coarse = classes[rng.integers(0, len(classes), (B, H // 32, W // 32))]
    sem = np.repeat(np.repeat(coarse, 32, 1), 32, 2).astype(np.uint8)
    for b in range(B):                                     # every class of the list is there, whatever the draw
        sem[b, :8, :8 * len(classes)] = np.repeat(classes, 8)[None]
    metas = [dict(batch_input_shape=(H, W), img_shape=(H, W, 3)) for _ in range(B)]
    return masks, torch.from_numpy(sem)[:, None], metas


def timed(fn, calls, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    us = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        us.append((time.perf_counter() - t0) * 1e6)
    return min(us), statistics.median(us)


def one_shape(name, calls, warmup):
    vkn = vkn_import.load()
    cfg = SHAPES[name]
    dev = torch.device('cuda:0')
    masks, sem, metas = inputs(cfg)
    labels = [torch.zeros(cfg['G'], dtype=torch.int64, device=dev) for _ in masks]
    prep = vkn.GtPrep(cfg['stride'], cfg['T'], cfg['S'], dataset=cfg['dataset'])
    bitmaps = [Bitmap(m) for m in masks]
    cpu_masks = [torch.from_numpy(m) for m in masks]
    valid = [cfg['pad']] * cfg['B']

    def fused():
        return prep.preprocess_gt_masks(metas, bitmaps, labels, sem)

    def composed():
        return prep._compose(dev, cpu_masks, sem, valid, *cfg['pad'])

    dev_masks, dev_sem = [m.to(dev) for m in cpu_masks], sem.to(dev)

    def fused_resident():                                  # the same call without the upload: where the fused time goes
        return prep.preprocess_gt_masks(metas, dev_masks, labels, dev_sem)

    a, b = fused(), composed()
    assert prep.n_sem != [] and all(torch.equal(x, y) for i in range(3) for x, y in zip(a[i], b[i]))
    fused()
    n_sem, rows = list(prep.n_sem), int(prep.bank.shape[0])
    f_min, f_med = timed(fused, calls, warmup)
    assert prep.fused is True
    c_min, c_med = timed(composed, calls, warmup)
    r_min, r_med = timed(fused_resident, calls, warmup)
    src = sum(m.nbytes for m in masks) + sem.numel()
    bank = rows * (cfg['pad'][0] // cfg['stride']) * (cfg['pad'][1] // cfg['stride']) * 4
    floor = (2 * src + bank) / HBM * 1e6
    shape = (f'{name} {cfg["pad"][0]}x{cfg["pad"][1]} stride={cfg["stride"]} B={cfg["B"]} things={cfg["G"]} stuff={n_sem} '
             f'bank_rows={rows} calls={calls}')
    stamp, box = datetime.date.today().isoformat(), torch.cuda.get_device_name(0)
    return [f'{stamp} {box} {shape} composition per call: min {c_min:.1f} us  median {c_med:.1f} us',
            f'{stamp} {box} {shape} fused       per call: min {f_min:.1f} us  median {f_med:.1f} us  '
            f'(composition / fused: min {c_min / f_min:.2f}x median {c_med / f_med:.2f}x)',
            f'{stamp} {box} {shape} fused, bytes already on the device: min {r_min:.1f} us  median {r_med:.1f} us',
            f'{stamp} {box} {shape} floor: {src} B uploaded and written, {src} B read once, {bank} B of bank written at '
            f'{HBM / 1e12:.1f} TB/s = {floor:.2f} us']


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--calls', type=int, default=200)
    ap.add_argument('--warmup', type=int, default=20)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gt_prep_ab.txt'))
    ap.add_argument('--shape', choices=sorted(SHAPES), help='(internal) measure this shape in this process and print its lines')
    ap.add_argument('--limit', type=int, default=240, help='seconds per shape')
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit('gt_prep_ab.py measures on the GPU; there is none here')
    if args.shape:
        print('\n'.join(one_shape(args.shape, args.calls, args.warmup)))
        return
    lines = []
    for name in ('kitti_step', 'cityscapes'):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), '--shape', name, '--calls', str(args.calls), '--warmup',
                            str(args.warmup)], capture_output=True, text=True, timeout=args.limit)
        if r.returncode != 0:
            sys.exit(f'{name}: exit status {r.returncode}\n{r.stdout}{r.stderr}')
        lines += [l for l in r.stdout.split('\n') if l.strip()]
    print('\n'.join(lines))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, 'w') as f:
        f.write('\n'.join(lines) + '\n')


if __name__ == '__main__':
    main()
