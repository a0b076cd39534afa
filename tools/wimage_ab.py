"""Bitwise and timing A/B of the split weight tile images (csrc/vkn_wimage.h; writer csrc/vkn_wimage.hip; readers k_gemm_s3 / k_ffn_fused /
k_attn_mfma of csrc/vkn_update.hip, k_gemm_t3 / k_chain_a / k_chain_c of csrc/vkn_chain.hip in both builds, k_gemm_ks of
csrc/vkn_ksplit.hip), to be compared between two builds of libvkn.so.  Run once per library, each in a fresh process; `--lib` makes this
tree's Python load another build (the headers must be the same).

Default: one SHA-256 per output, all on seeded non-integer operands:
  * the images of every writer case of tests/test_gpu_wimage.py (output buffers pre-filled);
  * the whole pre-filled prepared buffer of vkn_prepare_stage_f32 at C = 256, ff = 2048, with and without fc_cls: every bf16 and fp16
    image the chain reads, the composite weights and the constant block;
  * vkn_linear_f32 on split weights at M = 1, 33, 117: K = 64, 96 (k_gemm_s3), 256 (k_gemm_ks), 512, 768 (k_gemm_t3), 1024 (k_gemm_s3 past
    k_gemm_t3's range) and K = 512 with ksplit 2;
  * vkn_stage_chain_f32 at N = 117, C = 256 as one launch per GEMM (with the fused FFN), persistent bf16x3, persistent fp16 (B = 3) and the
    few-row chain (B = 1, 2), and a two-stage video head forward under the same four forms;
  * one training stage's chain forward + backward through chain_train.py (the batch writer in both orientations): outputs and every gradient.
`--time`: instead, the median in us of 20 timed calls after 5 (HIP events around each call) of vkn_split_weights_batch_f32 on the item
list chain_train.py builds for one cfg3 stage (the recorded calls, replayed) and of vkn_prepare_stage_f32 at C = 256, ff = 2048.
The first line, behind a `#`, names the device and the library that was loaded; compare the rest (profiles/wimage_ab.txt).

    python tools/wimage_ab.py [--time] [--lib PATH/libvkn.so] [--out FILE]
"""
import argparse
import ctypes
import hashlib
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, 'tests')]

import numpy as np  # noqa: E402
import torch  # noqa: E402

import vkn_import  # noqa: E402
import wimage_ref as wr  # noqa: E402

DEV = 'cuda:0'
FILL = 0xA5


def _rand(shape, seed, scale=1.0):
    return (torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * scale).to(DEV)


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _img_bytes(nout, k):
    return 6 * ((nout + 255) // 256 * 256) * k


def writer_hashes(vkn, put):
    L, I = vkn._lib.lib(), vkn._lib.VknSplitItem
    for nout, k in wr.SHAPES:
        W = torch.from_numpy(wr.matrix(nout, k, 4200 + nout)).to(DEV)
        Wt = W.t().contiguous()
        a, b = (torch.full((_img_bytes(nout, k),), FILL, dtype=torch.uint8, device=DEV) for _ in range(2))
        vkn._lib.check(L.vkn_split_weight_f32(W.data_ptr(), a.data_ptr(), nout, k, _stream()))
        vkn._lib.check(L.vkn_split_weight_t_f32(Wt.data_ptr(), b.data_ptr(), nout, k, _stream()))
        put(f'split_weight[{nout} x {k}]', plain=a, transposed=b)
    A = wr.matrix(300, 64, 4402)
    stride65 = np.full((300, 65), 7.5, dtype=np.float32)
    stride65[:, :64] = A
    negz = wr.matrix(256, 32, 4404)
    negz[3, 5] = -0.0
    Bm = wr.matrix(70, 40, 4406)
    dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)  # noqa: E731
    # name -> [(stored tensor, element offset, ldn, ldk, Nout, K, kvalid)]
    cases = {'kvalid 40 of 64': [(dev(wr.matrix(300, 40, 4401)), 0, 40, 1, 300, 64, 40)],
             'row stride 65': [(dev(stride65), 0, 65, 1, 300, 64, 64)],
             'base off by one float': [(dev(np.concatenate([np.float32([7.5]), A.reshape(-1)])), 1, 64, 1, 300, 64, 64)],
             'negative zero': [(dev(negz), 0, 32, 1, 256, 32, 32)],
             'two items': [(dev(A), 0, 64, 1, 300, 64, 64), (dev(Bm.T), 0, 1, 70, 70, 64, 40)]}
    for name, items in cases.items():
        outs = [torch.full((_img_bytes(it[4], it[5]),), FILL, dtype=torch.uint8, device=DEV) for it in items]
        arr = (I * len(items))(*[I(t.data_ptr() + 4 * off, o.data_ptr(), ldn, ldk, nout, K, kv, 0) for (t, off, ldn, ldk, nout, K, kv), o in zip(items, outs)])
        vkn._lib.check(L.vkn_split_weights_batch_f32(arr, len(items), _stream()))
        put(f'split_weights_batch[{name}]', **{f'item{i}': o for i, o in enumerate(outs)})


def _video_head(vkn, S, seed=0):
    torch.manual_seed(seed)                    # torch's own default initialisation of the biases draws from the global generator
    head = vkn.build_head(vkn.configs.roi_head_cfg(True, C=256, heads=8, ffn=2048, ncls=19, n_thing=2, n_stuff=17, S=S, up=1, nprop=100))
    head.init_weights()
    with torch.no_grad():                      # biases and LayerNorm parameters off their init values
        for i, p in enumerate(head.parameters()):
            if p.dim() == 1:
                p.add_(torch.randn(p.shape, generator=torch.Generator().manual_seed(900 + i)) * 0.2)
    return head.to(DEV).eval()


def _prepare(vkn, dims, w):
    """(buffer, call): the prepared buffer of (dims, w), pre-filled, and the call that fills it again"""
    L = vkn._lib.lib()
    nb = L.vkn_prepared_bytes(ctypes.byref(dims), ctypes.byref(w))
    buf = torch.full((nb,), FILL, dtype=torch.uint8, device=DEV)
    call = lambda: vkn._lib.check(L.vkn_prepare_stage_f32(ctypes.byref(dims), ctypes.byref(w), buf.data_ptr(), nb, _stream()))  # noqa: E731
    return buf, call


def hashes(vkn, put):
    ops = vkn.ops
    writer_hashes(vkn, put)
    N, C = 117, 256
    head = _video_head(vkn, 2)
    stage = head.mask_head[0]
    pack = stage.stage_pack(torch.device(DEV))
    dims = stage.make_dims(2, N, 16, 32)
    buf, call = _prepare(vkn, dims, pack.w)
    call()
    put('prepare_stage[C256 ff2048 fc_cls]', prepared=buf)
    nocls = type(pack.w).from_buffer_copy(pack.w)
    nocls.fc_cls_w = nocls.fc_cls_b = None
    buf, call = _prepare(vkn, dims, nocls)
    call()
    put('prepare_stage[C256 ff2048 no fc_cls]', prepared=buf)
    for K, nout, ks in ((64, 300, 1), (96, 19, 1), (256, 256, 1), (512, 768, 1), (768, 256, 1), (1024, 64, 1), (512, 256, 2)):
        W, bias = _rand((nout, K), 5000 + K + ks, 0.1), _rand((nout,), 5001 + K)
        img = ops.split_weight(W)
        for M in (1, 33, 117):
            put(f'linear[M{M} K{K} N{nout} ksplit{ks}]', y=ops.linear(_rand((M, K), 5100 + M), W, bias, w_split=img, act=M % 2, ksplit=ks))
    forms = (('launches', ops.FLAG_CHAIN_LAUNCHES, (3,)), ('persistent bf16x3', ops.FLAG_CHAIN_PERSISTENT | ops.FLAG_CHAIN_BF16X3, (3,)),
             ('persistent fp16', ops.FLAG_CHAIN_PERSISTENT, (3,)), ('few-row', ops.FLAG_CHAIN_KSPLIT, (1, 2)))
    for name, fl, frames in forms:
        for B in frames:
            d = stage.make_dims(B, N, 16, 32)
            out = ops.stage_chain(d, pack, _rand((B, N, C), 5200 + B, 30.0), _rand((B, N, C), 5201 + B), flags=fl)
            put(f'stage_chain[{name} B{B}]', **dict(zip(('cls', 'kernels', 'bias', 'obj'), out)))
    with torch.no_grad():
        for name, fl, frames in forms:
            B = frames[-1]
            x, pf, mp, prev = _rand((B, C, 16, 32), 5300), _rand((B, N, C, 1, 1), 5301), _rand((B, N, 16, 32), 5302, 4.0), _rand((B, N, C, 1, 1), 5303)
            out = head._head_forward(x, pf, mp, prev, want_track=True, flags=fl)
            put(f'head[2 stages, {name} B{B}]', **{k: v for k, v in zip(('obj', 'cls', 'masks', 'scaled', 'track'), out) if v is not None})
    import test_gpu_chain_train as T
    torch.manual_seed(7)
    tstage = T._head(vkn, True)
    ins = [T._rand((4, N, C), 71, 3.0).requires_grad_(True), T._rand((4, N, C, 1, 1), 72).requires_grad_(True), T._rand((4, N, C, 1, 1), 73).requires_grad_(True)]
    outs = [o for o in vkn.chain_train.chain_forward(tstage, *ins) if o is not None]
    torch.autograd.backward(outs, [T._rand(tuple(o.shape), 80 + i, 1e-3) for i, o in enumerate(outs)])
    put('chain_train[forward]', **{f'out{i}': o for i, o in enumerate(outs)})
    put('chain_train[backward, inputs]', **{f'in{i}': t.grad for i, t in enumerate(ins)})
    put('chain_train[backward, parameters]', **{n.replace('.', '_'): p.grad for n, p in tstage.named_parameters() if p.grad is not None})


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
    import test_gpu_chain_train as T
    L = vkn._lib.lib()
    real, calls = L.vkn_split_weights_batch_f32, []
    L.vkn_split_weights_batch_f32 = lambda arr, n, st: (calls.append((arr, n)), real(arr, n, st))[1]      # record chain_train.py's own calls
    tstage = T._head(vkn, True)
    imgs = vkn.chain_train.WeightImages([w for w, _ in vkn.chain_train.chain_linears(tstage, True)])    # (kept: the items point into it)
    L.vkn_split_weights_batch_f32 = real
    nitems = sum(n for _, n in calls)

    def replay():
        for arr, n in calls:
            vkn._lib.check(real(arr, n, _stream()))
    lines.append(f'{_median_us(replay):10.1f}  split_weights_batch, one cfg3 stage: {nitems} items in {len(calls)} launch(es)')
    del imgs
    head = _video_head(vkn, 1)
    stage = head.mask_head[0]
    buf, call = _prepare(vkn, stage.make_dims(2, 117, 16, 32), stage.stage_pack(torch.device(DEV)).w)
    lines.append(f'{_median_us(call):10.1f}  prepare_stage C256 ff2048')


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--lib', default=None, help='another build of libvkn.so to load instead of this tree\'s')
    ap.add_argument('--time', action='store_true', help='the timing rows (median us) instead of the hashes')
    ap.add_argument('--out', default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit('wimage_ab: needs the GPU')
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
