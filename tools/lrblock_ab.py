"""Bitwise and timing A/B of the four kernels with the low-res block geometry (k_ml_fwd_lr / k_ml_bwd_lr of csrc/vkn_loss.hip, k_seg_fwd /
k_seg_bwd of csrc/vkn_segloss.hip), to be compared between two builds of libvkn.so: what an edit of these kernels has to pass, since their
last bits follow hipcc's contraction of their text (docs/LAB_NOTEBOOK.md, 2026-10-21).  Run once per library, each in a fresh process;
`--lib` makes this tree's Python load another build (the headers must be the same).

Default: one SHA-256 per output tensor, all on seeded operands made on the CPU:
  * mask pair (vkn_mask_losses_fwd_lowres_f32 / _bwd_lowres_f32): row_partial, rank_partial, lse, top; grad_low.  The backward is fed
    seeded lse / top / dice sums of its own, not the forward's, so that a difference names its kernel.  MASK below: the ragged maps of
    tests/test_gpu_lowres_tail_kernels.py, the backward's tile edges (w = 63 / 64, h = 7 / 8), the forward's chunk edge ((h + 1)(w + 1) =
    256 and 258 — 257 is prime, no map has it), Ns = 2 (two of the four row parts empty) and 23, a 48 x 156 frame; each at S = 2 and 4,
    with and without the rank loss; and the +-600 spread that takes the forward's online-logsumexp redo path.
  * seg pair (vkn_seg_loss_fwd_f32 / _bwd_f32): loss, the state buffer (zeroed first), grad_low.  SEG below x S = 1, 2, 4 x focal (gamma
    2 and 1.5) and CE x ncls = 5 (nsplit 1) and 19 (nsplit 4); a tenth of the pixels ignored.
`--time`: instead, the median in us of 20 timed calls after 5 (HIP events around each call) at 128 x 256, S = 4, B = 2 and 4: the mask pair
at Ns = 117, K = 60 (the cfg3 loss shape of bench.py --train), the seg pair at ncls = 19 in both modes.
The first line, behind a `#`, names the device and the library that was loaded; compare the rest.

    python tools/lrblock_ab.py [--time] [--lib PATH/libvkn.so] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]

import torch  # noqa: E402

import vkn_import  # noqa: E402

DEV = 'cuda:0'
# (B, Ns, h, w, K): what of the engine the shape reaches
MASK = [(1, 117, 1, 9, 5), (2, 9, 11, 1, 4), (2, 23, 7, 13, 9), (3, 40, 5, 70, 17), (1, 256, 6, 10, 30),      # the ragged maps
        (1, 5, 3, 63, 2), (1, 5, 3, 64, 2),          # one tile of the backward exactly / one column into the second
        (1, 5, 7, 5, 2), (1, 5, 8, 5, 2),            # NW - 1 rows / NW
        (1, 5, 15, 15, 2), (1, 5, 1, 128, 2),        # 256 blocks: one chunk of the forward exactly / 258
        (2, 2, 6, 10, 2),                            # two of the backward's four row parts are empty
        (1, 117, 48, 156, 30)]                       # a KITTI-STEP frame
SPREAD = (2, 31, 9, 20, 3)                           # test_lowres_forward_logsumexp_survives_a_huge_spread: logits x 200, S = 4
SEG = [(3, 63), (4, 64), (1, 9), (11, 1)]            # h x w: SEG_NW - 1 rows and one backward tile / SEG_NW rows and a second tile / ragged
p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None   # noqa: E731


def mask_case(B, Ns, h, w, S, K, scale=3.0, seed=None):
    g = torch.Generator().manual_seed(1000 * h + w + S if seed is None else seed)
    low = torch.randn(B, Ns, h, w, generator=g) * scale
    bank = (torch.rand(K, S * h, S * w, generator=g) > 0.6).float()
    pos = torch.randperm(B * Ns, generator=g)[:K].sort()[0]
    if Ns == 256:
        pos[-1] = B * Ns - 1                         # top = 255 is a real row index
        pos = pos.unique()
        K = int(pos.numel())
        bank = bank[:K].contiguous()
    rowk, tgt = torch.full((B * Ns,), -1, dtype=torch.int32), torch.zeros(B * Ns, dtype=torch.int32)
    rowk[pos] = torch.arange(K, dtype=torch.int32)
    tgt[pos] = torch.arange(K, dtype=torch.int32)
    P = S * h * S * w
    a, bc = torch.rand(K, generator=g) * 50, torch.rand(K, generator=g) * 50 + 60
    lse = torch.randn(B, P, generator=g) + 8.0
    top = torch.randint(-1, Ns, (B, P), generator=g, dtype=torch.int32)
    return K, [t.to(DEV) for t in (low, bank, rowk, tgt, a, bc, lse, top)]


def mask_pair(L, B, Ns, h, w, S, K, with_rank, ops):
    """-> the forward's and the backward's outputs, every buffer pre-filled so that an unwritten element shows"""
    low, bank, rowk, tgt, a, bc, lse_in, top_in = ops
    P, st = S * h * S * w, ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    ncl = L.vkn_mask_losses_lowres_chunks(h, w)
    rp, rk = torch.zeros(K, ncl, 4, device=DEV), torch.zeros(B, ncl, device=DEV)
    lse, top = torch.full((B, P), -3.0, device=DEV), torch.full((B, P), -7, dtype=torch.int32, device=DEV)
    one, grad = torch.ones(1, device=DEV), torch.full_like(low, -3.0)

    def fwd():
        assert L.vkn_mask_losses_fwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), K, B, Ns, h, w, S, with_rank, p(rp), p(lse), p(top), p(rk), st) == 0

    def bwd():
        assert L.vkn_mask_losses_bwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), p(a), p(bc), p(one), p(one), p(one), 1.0, 4.0, 0.1, K, p(lse_in),
                                                p(top_in), B, Ns, h, w, S, with_rank, p(grad), st) == 0
    return fwd, bwd, dict(row_partial=rp, rank_partial=rk, lse=lse, top=top), dict(grad_low=grad)


def seg_case(B, ncls, h, w, S):
    g = torch.Generator().manual_seed(77 * h + w + 1000 * S + ncls)
    low = torch.randn(B, ncls, h, w, generator=g) * 2
    tgt = torch.randint(0, ncls, (B, S * h, S * w), generator=g).to(torch.uint8)
    tgt[torch.rand(B, S * h, S * w, generator=g) < 0.1] = ncls            # ignored pixels
    dp = (tgt < ncls).sum().to(torch.int32).reshape(1)
    return [t.to(DEV) for t in (low, tgt, dp)]


def seg_pair(L, mode, B, ncls, h, w, S, gamma, ops):
    low, tgt, dp = ops
    state = torch.zeros((max(L.vkn_seg_loss_state_bytes(mode, B, h, w, S), 64),), dtype=torch.uint8, device=DEV)
    loss, gout, grad = torch.full((1,), -3.0, device=DEV), torch.full((1,), 0.7, device=DEV), torch.full_like(low, -3.0)
    st = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def fwd():
        assert L.vkn_seg_loss_fwd_f32(p(low), p(tgt), p(dp), mode, B, ncls, h, w, S, 0.25, gamma, 1.0, p(loss), p(state), st) == 0

    def bwd():
        assert L.vkn_seg_loss_bwd_f32(p(low), p(tgt), p(gout), mode, B, ncls, h, w, S, 0.25, gamma, p(state), p(grad), st) == 0
    return fwd, bwd, dict(loss=loss, state=state), dict(grad_low=grad)


def hashes(L, put):
    for S in (2, 4):
        for B, Ns, h, w, K in MASK:
            K, ops = mask_case(B, Ns, h, w, S, K)
            for wr in (1, 0):
                fwd, bwd, fo, bo = mask_pair(L, B, Ns, h, w, S, K, wr, ops)
                fwd()
                bwd()
                if not wr:
                    fo = dict(row_partial=fo['row_partial'])
                put(f'mask[S{S} B{B} Ns{Ns} {h}x{w} K{K} rank{wr}]', **fo, **bo)
    B, Ns, h, w, K = SPREAD
    K, ops = mask_case(B, Ns, h, w, 4, K, scale=200.0, seed=9)
    fwd, bwd, fo, bo = mask_pair(L, B, Ns, h, w, 4, K, 1, ops)
    fwd()
    bwd()
    put(f'mask[S4 B{B} Ns{Ns} {h}x{w} K{K} rank1 spread]', **fo, **bo)
    for S in (1, 2, 4):
        for ncls in (5, 19):
            for h, w in SEG:
                ops = seg_case(2, ncls, h, w, S)
                for mode, gamma, name in ((0, 2.0, 'focal g2'), (0, 1.5, 'focal g1.5'), (1, 0.0, 'ce')):
                    fwd, bwd, fo, bo = seg_pair(L, mode, 2, ncls, h, w, S, gamma, ops)
                    fwd()
                    bwd()
                    put(f'seg[S{S} {name} ncls{ncls} {h}x{w}]', **fo, **bo)


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


def timings(L, lines):
    h, w, S = 128, 256, 4
    for B in (2, 4):
        K, ops = mask_case(B, 117, h, w, S, 60)
        fwd, bwd, _, _ = mask_pair(L, B, 117, h, w, S, K, 1, ops)
        lines.append(f'{_median_us(fwd):10.1f}  k_ml_fwd_lr<4> B{B} Ns117 K60 128x256')
        lines.append(f'{_median_us(bwd):10.1f}  k_ml_bwd_lr<4> B{B} Ns117 K60 128x256')
        del ops, fwd, bwd
    for B in (2, 4):
        ops = seg_case(B, 19, h, w, S)
        for mode, name in ((0, 'focal'), (1, 'ce')):
            fwd, bwd, _, _ = seg_pair(L, mode, B, 19, h, w, S, 2.0, ops)
            lines.append(f'{_median_us(fwd):10.1f}  k_seg_fwd<4, {name}> + finish B{B} ncls19 128x256')
            lines.append(f'{_median_us(bwd):10.1f}  k_seg_bwd<4, {name}> B{B} ncls19 128x256')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libvkn.so to load instead of this tree\'s')
    ap.add_argument('--time', action='store_true', help='the timing rows (median us) instead of the hashes')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('lrblock_ab: needs the GPU')
    vkn = vkn_import.load()
    if args.lib:
        vkn._lib.LIBPATH = os.path.abspath(args.lib)
    L = vkn._lib.lib()
    lines = []

    def put(name, **tensors):
        torch.cuda.synchronize()
        for k, t in tensors.items():
            lines.append(f'{hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()}  {name} {k} {tuple(t.shape)}')

    if args.time:
        timings(L, lines)
    else:
        hashes(L, put)
    path = L._name
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
