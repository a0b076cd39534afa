"""Python <-> C-ABI glue for the kernel-update head ops: torch is used only for device memory and streams.

Every function enqueues HIP kernels of libvkn.so on the CURRENT torch stream, on the tensors' device, and returns
torch tensors.  Inputs must be CUDA(=HIP) fp32 tensors; there is no CPU path here by design — the CPU restatement
lives in `oracle/` and is test infrastructure only.
"""
import contextlib
import ctypes
import struct
import threading

import torch

from . import _lib
from ._lib import VknDims, VknStageWeights, check

_H = _lib.CONSTS      # the integer #defines of include/vkn.h
FLAG_REF_KERNELS = _H['VKN_FLAG_REF_KERNELS']
FLAG_EXACT_GEMM = _H['VKN_FLAG_EXACT_GEMM']
FLAG_LOGITS_HANDOFF = _H['VKN_FLAG_LOGITS_HANDOFF']
FLAG_BITS_HANDOFF = _H['VKN_FLAG_BITS_HANDOFF']
FLAG_CHAIN_LAUNCHES = _H['VKN_FLAG_CHAIN_LAUNCHES']      # the [N x C] chain always as one launch per GEMM (default: by row count, include/vkn.h)
FLAG_CHAIN_PERSISTENT = _H['VKN_FLAG_CHAIN_PERSISTENT']  # ... always as the two persistent row-owner kernels (vkn_chain.hip)
FLAG_JOIN_EARLY = _H['VKN_FLAG_JOIN_EARLY']              # head_forward: the side-stream link joins BEFORE the upsample (single-call latency; 1.3-2.5 % slower in throughput)
FLAG_LINK_RESERVE = _H['VKN_FLAG_LINK_RESERVE']          # head_forward: the last decode on 3/4 of its default grid (at most 192 workgroups) at ANY size with a side-stream link (default: 192 of 256 from 8 frames on; tests, A/B)
FLAG_LINK_NO_RESERVE = _H['VKN_FLAG_LINK_NO_RESERVE']    # head_forward: ... never (A/B against the default grid of the last decode)
FLAG_SCALED_F16 = _H['VKN_FLAG_SCALED_F16']              # head_forward: the up-scaled logits as fp16 (vkn_upsample_bilinear_f16out)
FLAG_CHAIN_BF16X3 = _H['VKN_FLAG_CHAIN_BF16X3']          # ... the persistent kernels on the three-term bf16 split of rounds 2-4 (default since round 5: the two-term fp16 split, vkn_chain_h2.hip)
FLAG_INIT_SEPARATE = _H['VKN_FLAG_INIT_SEPARATE']        # vkn_kernel_init_f32: the round-5 form of pass 0 (separate decodes + add + logits gather) instead of the one-pass kernel (A/B)
FLAG_CHAIN_KSPLIT = _H['VKN_FLAG_CHAIN_KSPLIT']          # ... always as the few-row chain: column-spread GEMM phases, normalisation in the consumer (vkn_ksplit.hip)
FLAG_SERIAL_LINK = _H['VKN_FLAG_SERIAL_LINK']            # tracking link on the caller's stream instead of the library's side stream (A/B; same results)

_tls = threading.local()


def _ptr(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _req(t, name):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.VknLibraryError(f'{name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if t.dtype != torch.float32:
        raise TypeError(f'{name}: expected float32, got {t.dtype}')
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


_X_DTYPES = {torch.float32: _H['VKN_X_F32'], torch.float16: _H['VKN_X_F16'], torch.bfloat16: _H['VKN_X_BF16']}
FLAG_X_F16, FLAG_X_BF16 = _H['VKN_FLAG_X_F16'], _H['VKN_FLAG_X_BF16']


def _req_x(t, name='x'):
    """The feature map: fp32, or fp16 / bf16 STORAGE (VKN_X_*; the head still computes in fp32).  Returns (tensor, x_dtype code)."""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.VknLibraryError(f'{name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if t.dtype not in _X_DTYPES:
        raise TypeError(f'{name}: expected float32, float16 or bfloat16, got {t.dtype}')
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t, _X_DTYPES[t.dtype]


def _workspace(nbytes, device, scratch=False):
    """Grow-only per-(thread, device, stream) scratch buffer handed to the C ABI (the library never allocates).  Keyed by the
    current stream so that calls enqueued on different streams never share scratch memory.
    The first 256 bytes are the HEADER of the stage / head / chain entry points (their status word, include/vkn.h: they carve it
    first and only ever OR into it).  Every other entry point uses its workspace from offset 0 — `scratch=True` hands those the
    buffer BEHIND the header, so that a gather / decode / kernel-init / assignment call between two head calls cannot leave its
    scratch data where `workspace_status` reads the status word (found by the soak: a spurious error after the kernel-init pass)."""
    cache = getattr(_tls, 'ws', None)
    if cache is None:
        cache = _tls.ws = {}
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    buf = cache.get(key)
    need = int(nbytes) + 256
    if buf is None or buf.numel() < need:
        old = buf
        buf = torch.empty(max(need, 512), dtype=torch.uint8, device=device)
        if old is None:
            buf[:256].zero_()      # the workspace header: its first word is the status word the kernels OR into (include/vkn.h)
        else:
            buf[:256].copy_(old[:256])   # regrow: a sticky VKN_STATUS_RANGE nobody has read yet moves with the header (same stream: ordered)
        cache[key] = buf
        gen = getattr(_tls, 'ws_gen', None)
        if gen is None:
            gen = _tls.ws_gen = {}
        gen[key] = gen.get(key, 0) + 1   # `workspace_generation`: state kept in the buffer between calls (PHASE_A/B/C) dies with a regrow
    return buf[256:] if scratch else buf


def workspace_cache():
    """This thread's workspace cache (one buffer per (device, stream), with its status header) as a handle for `adopt_workspace`."""
    if getattr(_tls, 'ws', None) is None:
        _tls.ws = {}
    if getattr(_tls, 'ws_gen', None) is None:
        _tls.ws_gen = {}
    return _tls.ws, _tls.ws_gen


@contextlib.contextmanager
def adopt_workspace(cache):
    """Run the block on the workspace cache of ANOTHER thread (`workspace_cache()` taken there).  autograd runs a backward on a thread
    of its own, on the forward's stream, while the thread that called it waits: a backward that adopts the forward thread's cache
    ORs its status bits into the word that thread's `workspace_status` reads, instead of a header nobody looks at."""
    old = getattr(_tls, 'ws', None), getattr(_tls, 'ws_gen', None)
    _tls.ws, _tls.ws_gen = cache
    try:
        yield
    finally:
        _tls.ws, _tls.ws_gen = old


def workspace_generation(device):
    """How often this (thread, device, stream)'s workspace has been (re)allocated.  The phased clip call (PHASE_A / B / C) keeps state
    in the workspace between its three calls: a caller compares the generation before B / C with the one after A."""
    gen = getattr(_tls, 'ws_gen', None) or {}
    return gen.get((device, torch.cuda.current_stream(device).cuda_stream), 0)


def workspace_status(device=None):
    """Synchronise the current stream and read-and-clear the status word of this (thread, device, stream)'s workspace: raises
    `VknError` (VKN_E_RANGE) when a mask gather of a stage / head call since the last check produced non-finite sums — some
    |x| >= 65504 or a non-finite x entered the f16 split (include/vkn.h: VKN_STATUS_RANGE).  Costs one stream synchronisation: call it
    when you would look at the results anyway (per video, per evaluation step), not per frame."""
    device = torch.device(device if device is not None else torch.cuda.current_device())
    if device.index is None:
        device = torch.device('cuda', torch.cuda.current_device())
    cache = getattr(_tls, 'ws', None) or {}
    buf = cache.get((device, torch.cuda.current_stream(device).cuda_stream))
    if buf is None:
        return
    with torch.cuda.device(device):
        check(_lib.lib().vkn_workspace_status(_ptr(buf), buf.numel(), _stream()))


_THR_CACHE = {}


def thr_logit(hard_mask_thr=0.5):
    """Smallest fp32 z with `torch.sigmoid(z) > hard_mask_thr` as ATen's CPU fp32 sigmoid evaluates it — the reference's
    `(mask_preds.sigmoid() > hard_mask_thr)` (knet/det/kernel_update_head.py:190-191) becomes `z >= thr_logit`.
    For 0.5 this is 8.940697e-08, NOT 0 (1/(1+exp(-z)) rounds to exactly 0.5 for smaller positive z).
    Found by bisection over the ordered fp32 bit patterns (sigmoid is monotone)."""
    key = float(hard_mask_thr)
    if key in _THR_CACHE:
        return _THR_CACHE[key]
    if not 0.0 < key < 1.0:
        raise ValueError('hard_mask_thr must be in (0, 1)')

    def f2o(f):  # float -> monotone integer key
        u = struct.unpack('<I', struct.pack('<f', f))[0]
        return u ^ 0xFFFFFFFF if u & 0x80000000 else u | 0x80000000

    def o2f(o):
        u = o & 0x7FFFFFFF if o & 0x80000000 else o ^ 0xFFFFFFFF
        return struct.unpack('<f', struct.pack('<I', u & 0xFFFFFFFF))[0]

    def on(o):
        # evaluate through a padded vector so the vectorised kernel (not only the scalar tail) is exercised
        t = torch.full((16,), o2f(o), dtype=torch.float32)
        return bool((t.sigmoid() > key)[0])

    lo, hi = f2o(-200.0), f2o(200.0)
    assert not on(lo) and on(hi)
    while hi - lo > 1:
        mid = (lo + hi) // 2
        if on(mid):
            hi = mid
        else:
            lo = mid
    _THR_CACHE[key] = o2f(hi)
    return _THR_CACHE[key]


def mask_gather(x, mask_logits, hard_mask_thr=0.5, flags=0):
    """(xraw [B,N,C], cnt [B,N]) = sum_p bit(mask)[b,n,p] * x[b,c,p] and the ON-pixel count.
    Replaces `einsum('bnhw,bchw->bnc', (mask.sigmoid() > thr).float(), x)` (knet/det/kernel_update_head.py:190-195)."""
    (x, xdt), m = _req_x(x), _req(mask_logits, 'mask_logits')
    flags |= (0, FLAG_X_F16, FLAG_X_BF16)[xdt]
    B, C = x.shape[0], x.shape[1]
    N = m.shape[1]
    P = x[0, 0].numel()
    if m.shape[0] != B or m[0, 0].numel() != P:
        raise ValueError('x and mask_logits disagree on batch or spatial size')
    L = _lib.lib()
    xraw = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
    cnt = torch.empty((B, N), dtype=torch.float32, device=x.device)
    nb = L.vkn_gather_workspace_bytes(B, N, C, P)
    ws = _workspace(nb, x.device, scratch=True)
    with torch.cuda.device(x.device):
        check(L.vkn_mask_gather_f32(_ptr(x), _ptr(m), thr_logit(hard_mask_thr), _ptr(xraw), _ptr(cnt), B, N, C, P, _ptr(ws),
                                    ws.numel(), flags, _stream()))
    return xraw, cnt


def mask_gather_real(x, a):
    """(out [B,N,C], asum [B,N]) = sum_p a[b,n,p] * x[b,c,p] and sum_p a — the gather with a REAL-valued left operand
    (`einsum('bnhw,bchw->bnc', a, x)`): decode backward w.r.t. the kernels, soft gather weights, soft ground-truth masks."""
    x, a = _req(x, 'x'), _req(a, 'a')
    B, C = x.shape[0], x.shape[1]
    N = a.shape[1]
    P = x[0, 0].numel()
    if a.shape[0] != B or a[0, 0].numel() != P:
        raise ValueError('x and a disagree on batch or spatial size')
    L = _lib.lib()
    out = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
    asum = torch.empty((B, N), dtype=torch.float32, device=x.device)
    ws = _workspace(L.vkn_gather_workspace_bytes(B, N, C, P), x.device, scratch=True)
    with torch.cuda.device(x.device):
        check(L.vkn_mask_gather_real_f32(_ptr(x), _ptr(a), _ptr(out), _ptr(asum), B, N, C, P, _ptr(ws), ws.numel(), _stream()))
    return out, asum


def mask_decode(x, kernels, bias=None, flags=0, out_scale=None):
    """out[b,n,h,w] = sum_c kernels[b,n,c] x[b,c,h,w] (+ bias[b,n]).
    Replaces the per-image `F.conv2d(x[i:i+1], mask_feat[i])`, K=1 (knet/det/kernel_update_head.py:247-260).
    `out_scale` (a DEVICE scalar tensor): every output times it, inside the kernel (the backward passes' power-of-two unscaling)."""
    (x, xdt), k = _req_x(x), _req(kernels.reshape(kernels.shape[0], kernels.shape[1], -1), 'kernels')
    flags |= (0, FLAG_X_F16, FLAG_X_BF16)[xdt]
    B, C, H, W = x.shape
    N = k.shape[1]
    if k.shape[0] != B or k.shape[2] != C:
        raise ValueError('kernels must be [B, N, C] (conv_kernel_size == 1)')
    bias = _req(bias, 'bias') if bias is not None else None
    L = _lib.lib()
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
    nb = L.vkn_decode_workspace_bytes(B, N, C)
    ws = _workspace(nb, x.device, scratch=True)
    with torch.cuda.device(x.device):
        if out_scale is not None:
            sc = _req(out_scale.reshape(1), 'out_scale')
            check(L.vkn_mask_decode_scaled_f32(_ptr(x), _ptr(k), _ptr(bias), _ptr(sc), _ptr(out), B, N, C, H * W, _ptr(ws), ws.numel(),
                                               flags, _stream()))
        else:
            check(L.vkn_mask_decode_f32(_ptr(x), _ptr(k), _ptr(bias), _ptr(out), B, N, C, H * W, _ptr(ws), ws.numel(), flags,
                                        _stream()))
    return out


def upsample_bilinear(masks, scale, out_f16=False):
    """`F.interpolate(masks, scale_factor=scale, mode='bilinear', align_corners=False)` (knet/det/kernel_iter_head.py:122-130).
    out_f16 (opt-in; scale 2 / 4): the result as fp16 — the same fp32 interpolation rounded once at the store, half the bytes."""
    m = _req(masks, 'masks')
    B, N, H, W = m.shape
    out = torch.empty((B, N, H * scale, W * scale), dtype=torch.float16 if out_f16 else torch.float32, device=m.device)
    with torch.cuda.device(m.device):
        if out_f16:
            check(_lib.lib().vkn_upsample_bilinear_f16out(_ptr(m), _ptr(out), B * N, H, W, int(scale), _stream()))
        else:
            check(_lib.lib().vkn_upsample_bilinear_f32(_ptr(m), _ptr(out), B * N, H, W, int(scale), _stream()))
    return out


def upsample_bilinear_bwd(grad_out, scale):
    """Adjoint of `upsample_bilinear`: grad_out [B, N, H*scale, W*scale] -> [B, N, H, W] (vkn_upsample_bilinear_bwd_f32)."""
    g = _req(grad_out, 'grad_out')
    B, N, OH, OW = g.shape
    H, W = OH // scale, OW // scale
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=g.device)
    with torch.cuda.device(g.device):
        check(_lib.lib().vkn_upsample_bilinear_bwd_f32(_ptr(g), _ptr(out), B * N, H, W, int(scale), _stream()))
    return out


class StagePack:
    """Device pointers of one stage's parameters in the C-ABI struct, plus the derived folded tensor `ft_wT`.
    Holds references to every tensor it points to.  Rebuilt when any parameter is replaced or modified in place
    (tracked through `Tensor._version` and `data_ptr`)."""

    def __init__(self, named: dict, device):
        self.keep = []
        self.w = VknStageWeights()
        self.sig = None

        def P(key):
            t = named.get(key)
            if t is None:
                return 0
            t = t.detach()
            if t.device != device or t.dtype != torch.float32 or not t.is_contiguous():
                t = t.to(device=device, dtype=torch.float32).contiguous()
            self.keep.append(t)
            return t.data_ptr()

        w = self.w
        if 'feat_transform.conv.weight' in named:
            ft = named['feat_transform.conv.weight'].detach().to(device=device, dtype=torch.float32)
            ft2 = ft.reshape(ft.shape[0], ft.shape[1]).contiguous()
            ftT = ft2.t().contiguous()
            self.keep += [ft2, ftT]
            w.ft_w, w.ft_wT = ft2.data_ptr(), ftT.data_ptr()
            w.ft_b = P('feat_transform.conv.bias')
        ku = 'kernel_update_conv.'
        w.dyn_w, w.dyn_b = P(ku + 'dynamic_layer.weight'), P(ku + 'dynamic_layer.bias')
        w.inp_w, w.inp_b = P(ku + 'input_layer.weight'), P(ku + 'input_layer.bias')
        w.ig_w, w.ig_b = P(ku + 'input_gate.weight'), P(ku + 'input_gate.bias')
        w.ug_w, w.ug_b = P(ku + 'update_gate.weight'), P(ku + 'update_gate.bias')
        w.norm_in_w, w.norm_in_b = P(ku + 'norm_in.weight'), P(ku + 'norm_in.bias')
        w.norm_out_w, w.norm_out_b = P(ku + 'norm_out.weight'), P(ku + 'norm_out.bias')
        w.inorm_in_w, w.inorm_in_b = P(ku + 'input_norm_in.weight'), P(ku + 'input_norm_in.bias')
        w.inorm_out_w, w.inorm_out_b = P(ku + 'input_norm_out.weight'), P(ku + 'input_norm_out.bias')
        w.fc_w, w.fc_b = P(ku + 'fc_layer.weight'), P(ku + 'fc_layer.bias')
        w.fc_norm_w, w.fc_norm_b = P(ku + 'fc_norm.weight'), P(ku + 'fc_norm.bias')
        w.attn_in_w, w.attn_in_b = P('attention.attn.in_proj_weight'), P('attention.attn.in_proj_bias')
        w.attn_out_w, w.attn_out_b = P('attention.attn.out_proj.weight'), P('attention.attn.out_proj.bias')
        w.attn_norm_w, w.attn_norm_b = P('attention_norm.weight'), P('attention_norm.bias')
        w.ffn1_w, w.ffn1_b = P('ffn.layers.0.0.weight'), P('ffn.layers.0.0.bias')
        w.ffn2_w, w.ffn2_b = P('ffn.layers.1.weight'), P('ffn.layers.1.bias')
        w.ffn_norm_w, w.ffn_norm_b = P('ffn_norm.weight'), P('ffn_norm.bias')
        i = 0
        while f'cls_fcs.{3 * i}.weight' in named:
            w.cls_fc_w[i] = P(f'cls_fcs.{3 * i}.weight')
            w.cls_ln_w[i], w.cls_ln_b[i] = P(f'cls_fcs.{3 * i + 1}.weight'), P(f'cls_fcs.{3 * i + 1}.bias')
            i += 1
        self.n_cls_fcs = i
        i = 0
        while f'mask_fcs.{3 * i}.weight' in named:
            w.mask_fc_w[i] = P(f'mask_fcs.{3 * i}.weight')
            w.mask_ln_w[i], w.mask_ln_b[i] = P(f'mask_fcs.{3 * i + 1}.weight'), P(f'mask_fcs.{3 * i + 1}.bias')
            i += 1
        self.n_mask_fcs = i
        w.fc_cls_w, w.fc_cls_b = P('fc_cls.weight'), P('fc_cls.bias')
        w.fc_mask_w, w.fc_mask_b = P('fc_mask.weight'), P('fc_mask.bias')
        pa = 'attention_previous.attn.'
        w.pa_in_w, w.pa_in_b = P(pa + 'in_proj_weight'), P(pa + 'in_proj_bias')
        w.pa_out_w, w.pa_out_b = P(pa + 'out_proj.weight'), P(pa + 'out_proj.bias')
        w.pa_norm_w, w.pa_norm_b = P('attention_previous_norm.weight'), P('attention_previous_norm.bias')
        w.lffn1_w, w.lffn1_b = P('link_ffn.layers.0.0.weight'), P('link_ffn.layers.0.0.bias')
        w.lffn2_w, w.lffn2_b = P('link_ffn.layers.1.weight'), P('link_ffn.layers.1.bias')
        w.lffn_norm_w, w.lffn_norm_b = P('link_ffn_norm.weight'), P('link_ffn_norm.bias')
        self.has_link = bool(w.pa_in_w and w.lffn1_w)
        self.device = device
        self._prep = None
        self._prep_key = None
        self._ready = None      # event recorded after vkn_prepare_stage_f32: other streams wait on it before using `prepared`

    def ensure_prepared(self, dims):
        """Pre-split every Linear weight into three bf16 terms (vkn_prepare_stage_f32) once per (pack, shape): the
        [N x C] GEMMs then run on bf16 MFMA with fp32-class accuracy instead of exact-fp32 MFMA."""
        key = (dims.C, dims.ff, dims.ncls, dims.n_cls_fcs, dims.n_mask_fcs)
        if self._prep is not None and self._prep_key == key:
            if self._ready is not None and not self._ready.query():
                torch.cuda.current_stream(self.device).wait_event(self._ready)   # prepared on another stream, still in flight
            return
        L = _lib.lib()
        self.w.prepared, self.w.prepared_bytes = None, 0
        nb = L.vkn_prepared_bytes(ctypes.byref(dims), ctypes.byref(self.w))
        if nb == 0:
            return
        buf = torch.empty(nb, dtype=torch.uint8, device=self.device)
        with torch.cuda.device(self.device):
            check(L.vkn_prepare_stage_f32(ctypes.byref(dims), ctypes.byref(self.w), _ptr(buf), nb, _stream()))
            self._ready = torch.cuda.Event()
            self._ready.record(torch.cuda.current_stream(self.device))
        self._prep, self._prep_key = buf, key
        self.w.prepared, self.w.prepared_bytes = buf.data_ptr(), nb

    @staticmethod
    def signature(named: dict, device):
        return (str(device),) + tuple((k, t.data_ptr(), t._version) for k, t in sorted(named.items()))


def link_pack(named: dict, device, updator=None, attention='attention_previous', norm='attention_previous_norm', ffn='link_ffn',
              ffn_norm='link_ffn_norm'):
    """The weights of one previous-frame LINK BLOCK (include/vkn.h: vkn_link_block_f32) as a `StagePack`: `named` are the
    owning stage's parameters, the arguments name the sub-modules the block is made of (`updator` None = no KernelUpdator).
    E.g. previous_link="update_dynamic_cov": updator='attention_previous_update_link', attention='attention_previous_link',
    norm='attention_previous_norm_link', ffn='link_ffn_link', ffn_norm='link_ffn_norm_link'
    (knet/video/kernel_update_head.py:216-236)."""
    remap = {}
    for src, dst in ((updator, 'kernel_update_conv'), (attention, 'attention_previous'), (norm, 'attention_previous_norm'),
                     (ffn, 'link_ffn'), (ffn_norm, 'link_ffn_norm')):
        if src is None:
            continue
        for k, v in named.items():
            if k.startswith(src + '.'):
                remap[dst + k[len(src):]] = v
    return StagePack(remap, device)


def _pw(pack):
    return ctypes.byref(pack.w) if pack is not None else None


def link_block(dims: VknDims, pack: StagePack, cur, prev, update_feature=None):
    """One link block on [B,N,C] kernel sets (see `link_pack`): out = LN(FFN(LN(cur + MHA(cur, kv)))), kv = prev or
    KernelUpdator(update_feature, prev) when the pack carries an updator."""
    cur, prev = _req(cur, 'cur'), _req(prev, 'prev')
    uf = _req(update_feature, 'update_feature') if update_feature is not None else None
    L = _lib.lib()
    pack.ensure_prepared(dims)
    out = torch.empty_like(cur)
    ws = _workspace(max(L.vkn_stage_workspace_bytes(ctypes.byref(dims)), 256), cur.device)
    with torch.cuda.device(cur.device):
        check(L.vkn_link_block_f32(ctypes.byref(dims), ctypes.byref(pack.w), _ptr(uf), _ptr(cur), _ptr(prev), _ptr(out), _ptr(ws),
                                   ws.numel(), _stream()))
    return out


def query_merge(dims: VknDims, pack: StagePack, query, keys, pos=None):
    """Clip-level attention query merge (include/vkn.h: vkn_query_merge_f32): query [B,N,C], keys [B,F*N,C] frame-major, pos [N,C] | None
    -> [B,N,C].  `pack`: `link_pack(named, dev, None, 'query_merge_attn', 'query_merge_norm', 'query_merge_ffn',
    'query_merge_ffn_norm')`; dims.ff is the merge FFN's width."""
    query, keys = _req(query, 'query'), _req(keys, 'keys')
    pos = _req(pos, 'pos') if pos is not None else None
    B, N, C = query.shape
    if keys.shape[0] != B or keys.shape[2] != C or keys.shape[1] % N or (pos is not None and tuple(pos.shape) != (N, C)):
        raise ValueError(f'query {tuple(query.shape)}, keys {tuple(keys.shape)}, pos {None if pos is None else tuple(pos.shape)}')
    F = keys.shape[1] // N
    L = _lib.lib()
    pack.ensure_prepared(dims)
    out = torch.empty_like(query)
    ws = _workspace(max(L.vkn_query_merge_workspace_bytes(ctypes.byref(dims), F), 256), query.device)
    with torch.cuda.device(query.device):
        check(L.vkn_query_merge_f32(ctypes.byref(dims), F, ctypes.byref(pack.w), _ptr(query), _ptr(keys), _ptr(pos), _ptr(out),
                                    _ptr(ws), ws.numel(), _stream()))
    return out


def make_dims(B, N, C, H, W, heads, ff, ncls, n_cls_fcs, n_mask_fcs, hard_mask_thr=0.5, ln_eps=1e-5):
    return VknDims(B, N, C, H, W, heads, ff, ncls, n_cls_fcs, n_mask_fcs, thr_logit(hard_mask_thr), ln_eps)


def stage_forward(dims: VknDims, pack: StagePack, x, obj_in, masks_in, prev_obj=None, want_track=False, flags=0, link_pre=None,
                  link_track=None, track_src=0):
    """One `KernelUpdateHead.forward` on the GPU.  Returns (cls_logits [B,N,ncls], masks [B,N,H,W], obj [B,N,C],
    x_feat [B,N,C], track [B,N,C] | None).  link_pre / link_track: `link_pack`s of the previous_link / previous_type="update"
    blocks (vkn_stage_forward_link_f32)."""
    (x, xdt), obj_in, masks_in = _req_x(x), _req(obj_in, 'proposal_feat'), _req(masks_in, 'mask_preds')
    flags |= (0, FLAG_X_F16, FLAG_X_BF16)[xdt]
    B, N, C, H, W = dims.B, dims.N, dims.C, dims.H, dims.W
    dev = x.device
    L = _lib.lib()
    cls = torch.empty((B, N, dims.ncls), dtype=torch.float32, device=dev)
    masks = torch.empty((B, N, H, W), dtype=torch.float32, device=dev)
    obj = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    xfeat = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    track = None
    if prev_obj is not None and (want_track or link_pre is not None):
        prev_obj = _req(prev_obj, 'previous_obj_feats')
        if want_track:
            track = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    else:
        prev_obj = None
        link_pre = link_track = None
    pack.ensure_prepared(dims)
    for lp in (link_pre, link_track):
        if lp is not None:
            lp.ensure_prepared(dims)
    nb = L.vkn_stage_workspace_bytes(ctypes.byref(dims))  # 0 for unsupported dims: the call below reports the reason
    ws = _workspace(max(nb, 256), dev)
    with torch.cuda.device(dev):
        if link_pre is not None or link_track is not None:
            check(L.vkn_stage_forward_link_f32(ctypes.byref(dims), ctypes.byref(pack.w), _pw(link_pre), _pw(link_track),
                                               int(track_src) if link_track is not None else 0, _ptr(x), _ptr(obj_in), _ptr(masks_in),
                                               _ptr(prev_obj), _ptr(cls), _ptr(masks), _ptr(obj), _ptr(xfeat), _ptr(track),
                                               _ptr(ws), ws.numel(), flags, _stream()))
        else:
            check(L.vkn_stage_forward_f32(ctypes.byref(dims), ctypes.byref(pack.w), _ptr(x), _ptr(obj_in), _ptr(masks_in),
                                          _ptr(prev_obj), _ptr(cls), _ptr(masks), _ptr(obj), _ptr(xfeat), _ptr(track),
                                          _ptr(ws), ws.numel(), flags, _stream()))
    return cls, masks, obj, xfeat, track


def stage_chain(dims: VknDims, pack: StagePack, x_feat, obj_in, want_cls=True, flags=0):
    """The [B*N, C] chain of one stage alone (no gather, no decode): x_feat [B,N,C] (feat-transformed), obj_in [B,N,C] ->
    (cls_logits [B,N,ncls] | None, folded decode kernels [B,N,C], decode bias [B,N], obj [B,N,C])."""
    xf, obj_in = _req(x_feat, 'x_feat'), _req(obj_in, 'proposal_feat')
    B, N, C = dims.B, dims.N, dims.C
    dev = xf.device
    L = _lib.lib()
    cls = torch.empty((B, N, dims.ncls), dtype=torch.float32, device=dev) if want_cls else None
    kern = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    kb = torch.empty((B, N), dtype=torch.float32, device=dev)
    obj = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    pack.ensure_prepared(dims)
    ws = _workspace(max(L.vkn_stage_workspace_bytes(ctypes.byref(dims)), 256), dev)
    with torch.cuda.device(dev):
        check(L.vkn_stage_chain_f32(ctypes.byref(dims), ctypes.byref(pack.w), _ptr(xf), _ptr(obj_in), _ptr(cls), _ptr(kern), _ptr(kb),
                                    _ptr(obj), _ptr(ws), ws.numel(), flags, _stream()))
    return cls, kern, kb, obj


PHASE_A, PHASE_B, PHASE_C = _H['VKN_FLAG_PHASE_A'], _H['VKN_FLAG_PHASE_B'], _H['VKN_FLAG_PHASE_C']


def head_forward(dims: VknDims, packs, x, proposal_feats, mask_preds, prev_obj=None, upsample_stride=1, want_track=False,
                 want_scaled=True, flags=0, clip_first_prev=None, decode_events=None, link_pre=None, link_track=None, track_src=0,
                 phase=0, out=None):
    """The S-stage loop in one C call.  Returns (obj [B,N,C], cls_prob [B,N,ncls], mask_preds [B,N,H,W],
    scaled_mask_preds [B,N,H*s,W*s] | None, track [B,N,C] | None).  link_pre / link_track / track_src: the LAST stage's
    previous_link / previous_type="update" blocks (`link_pack`; vkn_head_forward_link_f32) — they need prev_obj / clip_first_prev."""
    (x, xdt), pf, mp = _req_x(x), _req(proposal_feats, 'proposal_feats'), _req(mask_preds, 'mask_preds')
    flags |= (0, FLAG_X_F16, FLAG_X_BF16)[xdt]
    B, N, C, H, W = dims.B, dims.N, dims.C, dims.H, dims.W
    dev = x.device
    L = _lib.lib()
    S = len(packs)
    for p in packs:
        p.ensure_prepared(dims)
    arr = (VknStageWeights * S)(*[p.w for p in packs])
    # `phase` (PHASE_A | PHASE_B | PHASE_C, previous_link heads in clip mode only) runs a part of the call; `out` = the tuple a previous
    # phase returned: the later phases write the SAME tensors and continue from the state the earlier ones left in the workspace
    if out is not None:
        obj, cls, masks, scaled, track = out
        scaled = scaled if (want_scaled and upsample_stride > 1) else None
    else:
        obj = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        cls = torch.empty((B, N, dims.ncls), dtype=torch.float32, device=dev)
        masks = torch.empty((B, N, H, W), dtype=torch.float32, device=dev)
        scaled = None
        if want_scaled and upsample_stride > 1:
            scaled = torch.empty((B, N, H * upsample_stride, W * upsample_stride),
                                 dtype=torch.float16 if (flags & FLAG_SCALED_F16) else torch.float32, device=dev)
        track = None
    flags |= int(phase)
    if clip_first_prev is not None:
        # the B frames are consecutive frames of one video: frame b links to frame b - 1 of this call, frame 0 to `clip_first_prev`
        # [1,N,C] (VKN_FLAG_CLIP_LINK) — the whole clip step is one C call
        prev_obj = _req(clip_first_prev.reshape(1, N, C), 'clip_first_prev')
        if track is None:
            track = torch.empty((B, N, C), dtype=torch.float32, device=dev)
        flags |= _H['VKN_FLAG_CLIP_LINK']
    elif prev_obj is not None and (want_track or link_pre is not None):
        prev_obj = _req(prev_obj, 'previous_obj_feats')
        if want_track:
            track = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    else:
        prev_obj = None
        link_pre = link_track = None
    for lp in (link_pre, link_track):
        if lp is not None:
            lp.ensure_prepared(dims)
    nb = L.vkn_head_workspace_bytes(ctypes.byref(dims))
    ws = _workspace(max(nb, 256), dev)
    with torch.cuda.device(dev):
        if link_pre is not None or link_track is not None:
            check(L.vkn_head_forward_link_f32(ctypes.byref(dims), S, arr, _pw(link_pre), _pw(link_track),
                                              int(track_src) if link_track is not None else 0, _ptr(x), _ptr(pf), _ptr(mp),
                                              _ptr(prev_obj), _ptr(obj), _ptr(cls), _ptr(masks), _ptr(scaled), int(upsample_stride),
                                              _ptr(track), _ptr(ws), ws.numel(), flags, _stream()))
        elif decode_events is not None:
            # (start, stop) torch.cuda.Event(enable_timing=True) pair, each recorded once before (that creates the HIP event): the
            # library records them around the last stage's mask-decode launch on the current stream
            e0, e1 = decode_events
            check(L.vkn_head_forward_prof_f32(ctypes.byref(dims), S, arr, _ptr(x), _ptr(pf), _ptr(mp), _ptr(prev_obj), _ptr(obj),
                                              _ptr(cls), _ptr(masks), _ptr(scaled), int(upsample_stride), _ptr(track), _ptr(ws),
                                              ws.numel(), flags, _stream(), ctypes.c_void_p(e0.cuda_event),
                                              ctypes.c_void_p(e1.cuda_event)))
        else:
            check(L.vkn_head_forward_f32(ctypes.byref(dims), S, arr, _ptr(x), _ptr(pf), _ptr(mp), _ptr(prev_obj), _ptr(obj),
                                         _ptr(cls), _ptr(masks), _ptr(scaled), int(upsample_stride), _ptr(track), _ptr(ws),
                                         ws.numel(), flags, _stream()))
    return obj, cls, masks, (scaled if scaled is not None else masks), track


def split_planes(kernels):
    """fp32 kernels [B,N,C] -> (hi, lo) f16 planes [B, roundup(N,32), C] with hi + lo ~= kernels (2^-22 relative)."""
    k = _req(kernels.reshape(kernels.shape[0], kernels.shape[1], -1), 'kernels')
    B, N, C = k.shape
    npt = (N + 31) // 32 * 32
    hi = torch.zeros((B, npt, C), dtype=torch.float16, device=k.device)
    lo = torch.zeros((B, npt, C), dtype=torch.float16, device=k.device)
    with torch.cuda.device(k.device):
        check(_lib.lib().vkn_split_planes_f32(_ptr(k), _ptr(hi), _ptr(lo), B, N, C, _stream()))
    return hi, lo


def mask_decode_planes(x, hi, lo, N, bias=None, out=None):
    """The MFMA decode kernel alone on pre-split kernel planes (what runs inside a stage); `out` may be preallocated."""
    x, xdt = _req_x(x)
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vkn_mask_decode_planes_x(_ptr(x), xdt, _ptr(hi), _ptr(lo), _ptr(bias), _ptr(out), B, N, C, H * W,
                                                  _stream()))
    return out


def mask_decode_planes_wg(x, hi, lo, N, max_workgroups, bias=None, out=None):
    """mask_decode_planes on at most `max_workgroups` workgroups (0: the default split): bit-identical output whatever the split."""
    x, xdt = _req_x(x)
    B, C, H, W = x.shape
    if out is None:
        out = torch.empty((B, N, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        check(_lib.lib().vkn_mask_decode_planes_wg_x(_ptr(x), xdt, _ptr(hi), _ptr(lo), _ptr(bias), _ptr(out), B, N, C, H * W,
                                                     int(max_workgroups), _stream()))
    return out


def decode_px_per_wg(B, P, max_workgroups=0):
    """Pixels per workgroup of a decode launch over B frames of P pixels under a workgroup budget (host arithmetic only)."""
    r = _lib.lib().vkn_decode_px_per_wg(int(B), int(P), int(max_workgroups))
    if r < 0:
        check(r)
    return r


def decode_gather(x, hi, lo, N, bias=None, hard_mask_thr=0.5):
    """Stage s decode fused with the stage s + 1 gather, one pass over x: (xraw [B,N,C], cnt [B,N]) of the masks
    `bias + K.x >= thr` without materialising them (bit-identical to mask_decode_planes + mask_gather)."""
    x, xdt = _req_x(x)
    B, C, H, W = x.shape
    P = H * W
    L = _lib.lib()
    xraw = torch.empty((B, N, C), dtype=torch.float32, device=x.device)
    cnt = torch.empty((B, N), dtype=torch.float32, device=x.device)
    ws = _workspace(L.vkn_gather_workspace_bytes(B, N, C, P), x.device, scratch=True)
    with torch.cuda.device(x.device):
        check(L.vkn_decode_gather_x(_ptr(x), xdt, _ptr(hi), _ptr(lo), _ptr(bias), thr_logit(hard_mask_thr), _ptr(xraw), _ptr(cnt),
                                    B, N, C, P, _ptr(ws), ws.numel(), _stream()))
    return xraw, cnt


def track_link(dims: VknDims, pack: StagePack, cur_obj, prev_obj, flags=0):
    """Tracking embedding of the video head's last stage for a batch of (cur, prev) kernel sets:
    knet/video/kernel_update_head.py:394-415.  cur_obj, prev_obj [B,N,C] -> [B,N,C].  `flags`: FLAG_CHAIN_KSPLIT / _LAUNCHES pin the
    link's arithmetic to the form a larger call took (a hand-over re-link of one frame; include/vkn.h: vkn_track_link_flags_f32)."""
    cur, prev = _req(cur_obj, 'cur_obj'), _req(prev_obj, 'prev_obj')
    L = _lib.lib()
    pack.ensure_prepared(dims)
    out = torch.empty_like(cur)
    ws = _workspace(max(L.vkn_stage_workspace_bytes(ctypes.byref(dims)), 256), cur.device)
    with torch.cuda.device(cur.device):
        check(L.vkn_track_link_flags_f32(ctypes.byref(dims), ctypes.byref(pack.w), _ptr(cur), _ptr(prev), _ptr(out), _ptr(ws),
                                         ws.numel(), int(flags), _stream()))
    return out


def split_weight(W):
    """fp32 Linear weight [Nout, K] -> bf16x3 tile images (opaque uint8 buffer, 6 * roundup(Nout,256) * K bytes) for
    `linear(..., w_split=...)`."""
    W = _req(W, 'W')
    Nout, K = W.shape
    buf = torch.empty(6 * ((Nout + 255) // 256 * 256) * K, dtype=torch.uint8, device=W.device)   # 256-row tile images
    with torch.cuda.device(W.device):
        check(_lib.lib().vkn_split_weight_f32(_ptr(W), _ptr(buf), Nout, K, _stream()))
    return buf


def linear(A, W, bias=None, w_split=None, act=0, ksplit=1):
    """act(A @ W.T + bias) through the library's GEMM kernel (exact-fp32 MFMA, or bf16x3 split MFMA when `w_split` is given)."""
    A, W = _req(A, 'A'), _req(W, 'W')
    M, K = A.shape
    Nout = W.shape[0]
    out = torch.empty((M, Nout), dtype=torch.float32, device=A.device)
    ws = _workspace(max(ksplit * M * Nout * 4, 256), A.device, scratch=True)
    with torch.cuda.device(A.device):
        check(_lib.lib().vkn_linear_f32(_ptr(A), _ptr(W), _ptr(w_split), _ptr(bias), _ptr(out), M, K, Nout, int(act), int(ksplit),
                                        _ptr(ws), ws.numel(), _stream()))
    return out


def kernel_init(loc_feats, semantic_feats, init_w, seg_w=None, seg_b=None, num_thing_classes=0, cat_stuff_mask=False,
                proposal_feats_with_obj=True, hard_mask_thr=0.5, want_seg_preds=True, flags=0, use_binary=True):
    """Kernel initialisation ("pass 0"), `ConvKernelHead._decode_init_proposals` after its loc / seg convs
    (knet/det/kernel_head.py:204-263), use_binary semantics.  Returns (proposal_feats [B,N,C], x_feats [B,C,H,W],
    mask_preds [B,N,H,W], seg_preds [B,ncls,H,W] | None)."""
    loc, xdt = _req_x(loc_feats, 'loc_feats')       # fp32, or fp16 / bf16 STORAGE (x_feats then has the same type; the head reads it as is)
    flags = int(flags) | {1: FLAG_X_F16, 2: FLAG_X_BF16}.get(xdt, 0)
    B, C, H, W = loc.shape
    P = H * W
    dev = loc.device
    iw = _req(init_w.reshape(init_w.shape[0], -1), 'init_kernels.weight')
    Np = iw.shape[0]
    if iw.shape[1] != C:
        raise ValueError('init_kernels.weight must be [num_proposals, C, 1, 1] (conv_kernel_size == 1)')
    sem = sw = sb = None
    ncls = 0
    if semantic_feats is not None:
        sem, sdt = _req_x(semantic_feats, 'semantic_feats')
        if sem.shape != loc.shape or sdt != xdt:
            raise ValueError('semantic_feats and loc_feats must have the same shape and storage type')
        sw = _req(seg_w.reshape(seg_w.shape[0], -1), 'conv_seg.weight')
        sb = _req(seg_b, 'conv_seg.bias') if seg_b is not None else None
        ncls = sw.shape[0]
    elif cat_stuff_mask:
        raise ValueError('cat_stuff_mask needs the semantic branch')
    nstuff = ncls - num_thing_classes if cat_stuff_mask else 0
    N = Np + nstuff
    L = _lib.lib()
    x_feats = torch.empty_like(loc) if sem is not None else loc
    masks = torch.empty((B, N, H, W), dtype=torch.float32, device=dev)
    seg = torch.empty((B, ncls, H, W), dtype=torch.float32, device=dev) if (sem is not None and want_seg_preds) else None
    prop = torch.empty((B, N, C), dtype=torch.float32, device=dev)
    nb = L.vkn_kernel_init_workspace_bytes(B, Np, ncls, C, P)
    ws = _workspace(max(nb, 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_kernel_init_f32(_ptr(loc), _ptr(sem), _ptr(iw), _ptr(sw), _ptr(sb), int(num_thing_classes),
                                    int(bool(cat_stuff_mask)), (1 if use_binary else 2) if proposal_feats_with_obj else 0,
                                    thr_logit(hard_mask_thr),
                                    _ptr(x_feats), _ptr(masks), _ptr(seg), _ptr(prop), B, Np, ncls, C, P, _ptr(ws), ws.numel(),
                                    flags, _stream()))
    return prop, x_feats, masks, seg


def panoptic_joint(cls_prob, mask_logits, num_proposals, num_thing_classes, max_per_img, instance_score_thr, overlap_thr,
                   img_shape, batch_input_shape, ori_shape, upsample_stride=1, want_bbox=False):
    """Joint panoptic merge of a batch of frames sharing one img_meta, straight from the head's low-res mask logits
    (`get_panoptic` + `merge_stuff_thing_stuff_joint` + `rescale_masks`, knet/det/kernel_iter_head.py:332-370, 467-524).
    Returns device tensors (panoptic_seg int32 [B,Ho,Wo], info int32 [B,K,6], nseg int32 [B]) and, with `want_bbox`, a fourth
    one: bbox int32 [B,K,4] = (xmin, ymin, xmax, ymax) of every accepted segment (what the tracker consumes); see include/vkn.h."""
    cls, m = _req(cls_prob, 'cls_prob'), _req(mask_logits, 'mask_logits')
    B, N, ncls = cls.shape
    if m.shape[0] != B or m.shape[1] != N:
        raise ValueError('cls_prob [B,N,ncls] and mask_logits [B,N,Hm,Wm] disagree')
    Hm, Wm = int(m.shape[2]), int(m.shape[3])
    cfg = _lib.VknPanopticCfg(int(num_proposals), int(num_thing_classes), int(max_per_img), float(instance_score_thr),
                              float(overlap_thr), int(upsample_stride), Hm, Wm, int(batch_input_shape[0]),
                              int(batch_input_shape[1]), int(img_shape[0]), int(img_shape[1]), int(ori_shape[0]),
                              int(ori_shape[1]))
    K = int(max_per_img) + (N - int(num_proposals))
    dev = cls.device
    L = _lib.lib()
    seg = torch.empty((B, cfg.Ho, cfg.Wo), dtype=torch.int32, device=dev)
    info = torch.empty((B, K, 6), dtype=torch.int32, device=dev)
    nseg = torch.empty((B,), dtype=torch.int32, device=dev)
    bbox = torch.empty((B, K, 4), dtype=torch.int32, device=dev) if want_bbox else None
    nb = L.vkn_panoptic_workspace_bytes(ctypes.byref(cfg), B, N)
    ws = _workspace(max(nb, 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_panoptic_joint_f32(ctypes.byref(cfg), _ptr(cls), _ptr(m), B, N, ncls, seg.data_ptr(), info.data_ptr(),
                                       nseg.data_ptr(), bbox.data_ptr() if want_bbox else None, _ptr(ws), ws.numel(), _stream()))
    return (seg, info, nseg, bbox) if want_bbox else (seg, info, nseg)


def _req_int(t, name, dtype=torch.int32):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.VknLibraryError(f'{name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t


def track_boxes(panoptic_seg, info, nseg, num_thing_classes, sem_logits=None, want_thing_mask=False):
    """What the video detector hands its tracker, for the frames [B] of one geometry, straight from `panoptic_joint`'s outputs
    (`get_things_id_for_tracking` + the semantic filter + `tensor_mask2box`, knet/video/knet_quansi_dense_embed_fc_joint_train.py:
    541-584, 673-685).  `sem_logits` [B,Cs,hs,ws] fp32 (the kernel-init head's `seg_preds`) switches the semantic filter on.
    Returns device tensors (det fp32 [B,K,5], labels int64 [B,K], rows int32 [B,K], segid int32 [B,K], count int32 [B]) and, with
    `want_thing_mask`, a sixth one: thing_mask uint8 [B,Ho,Wo]; see include/vkn_track.h."""
    seg, inf, ns = _req_int(panoptic_seg, 'panoptic_seg'), _req_int(info, 'info'), _req_int(nseg, 'nseg')
    if seg.dim() != 3 or inf.dim() != 3 or inf.shape[0] != seg.shape[0] or inf.shape[2] != 6 or ns.numel() != seg.shape[0]:
        raise ValueError('panoptic_seg [B,Ho,Wo], info [B,K,6] and nseg [B] disagree')
    B, Ho, Wo = (int(v) for v in seg.shape)
    K = int(inf.shape[1])
    Cs = hs = ws_w = 0
    sem = None
    if sem_logits is not None:
        sem = _req(sem_logits, 'sem_logits')
        if sem.dim() != 4 or sem.shape[0] != B:
            raise ValueError('sem_logits must be [B,Cs,hs,ws]')
        Cs, hs, ws_w = (int(v) for v in sem.shape[1:])
    dev = seg.device
    L = _lib.lib()
    det = torch.empty((B, K, 5), dtype=torch.float32, device=dev)
    labels = torch.empty((B, K), dtype=torch.int64, device=dev)
    rows = torch.empty((B, K), dtype=torch.int32, device=dev)
    segid = torch.empty((B, K), dtype=torch.int32, device=dev)
    count = torch.empty((B,), dtype=torch.int32, device=dev)
    tmask = torch.empty((B, Ho, Wo), dtype=torch.uint8, device=dev) if want_thing_mask else None
    ws = _workspace(max(L.vkn_track_boxes_workspace_bytes(B, K), 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_track_boxes_f32(_ptr(seg), _ptr(inf), _ptr(ns), _ptr(sem), Cs, hs, ws_w, int(num_thing_classes), B, K, Ho, Wo,
                                    _ptr(det), _ptr(labels), _ptr(rows), _ptr(segid), _ptr(count), _ptr(tmask), _ptr(ws), ws.numel(),
                                    _stream()))
    return (det, labels, rows, segid, count, tmask) if want_thing_mask else (det, labels, rows, segid, count)


def track_maps(panoptic_seg, segid, count, ids, n_ids, info, sem_of_label):
    """The two maps the video detector returns (`generate_track_id_maps` + `get_semantic_seg`,
    knet/video/knet_quansi_dense_embed_fc_joint_train.py:591-592, 698-736) as int32 device tensors [B,Ho,Wo]:
    (track_map, semantic_map).  `ids` int64 [B,max_dets] / `n_ids` int32 [B] are the tracker's padded outputs, `segid` / `count` those of
    `track_boxes`, `sem_of_label` int32 [num_thing_classes + num_stuff_classes] a device table; see include/vkn_track.h."""
    seg, inf = _req_int(panoptic_seg, 'panoptic_seg'), _req_int(info, 'info')
    sg, ct = _req_int(segid, 'segid'), _req_int(count, 'count')
    ii, ni, tab = _req_int(ids, 'ids', torch.int64), _req_int(n_ids, 'n_ids'), _req_int(sem_of_label, 'sem_of_label')
    B, Ho, Wo = (int(v) for v in seg.shape)
    K = int(inf.shape[1])
    if sg.shape != (B, K) or ct.numel() != B or ii.dim() != 2 or ii.shape[0] != B or ni.numel() != B or inf.shape[0] != B:
        raise ValueError('segid [B,K], count [B], ids [B,max_dets], n_ids [B] and info [B,K,6] disagree')
    dev = seg.device
    L = _lib.lib()
    track_map = torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev)
    semantic_map = torch.empty((B, Ho, Wo), dtype=torch.int32, device=dev)
    ws = _workspace(max(L.vkn_track_maps_workspace_bytes(B, K), 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_track_maps_i32(_ptr(seg), _ptr(sg), _ptr(ct), _ptr(ii), _ptr(ni), int(ii.shape[1]), _ptr(inf), _ptr(tab),
                                   int(tab.numel()), B, K, Ho, Wo, _ptr(track_map), _ptr(semantic_map), _ptr(ws), ws.numel(), _stream()))
    return track_map, semantic_map


TRACK_LOSS_MAX_ROWS = _lib.TRACK_LOSS_MAX_ROWS


def track_loss_supported(N, E, B=1):
    """The envelope of `track_loss_fwd` (include/vkn_track_train.h)."""
    return 1 <= N <= TRACK_LOSS_MAX_ROWS and 4 <= E <= 1024 and E % 4 == 0 and 1 <= B <= 65535


def track_loss_cfg(softmax_temp=-1.0, has_aux=True, w_track=1.0, w_aux=1.0, neg_pos_ub=-1, pos_margin=-1.0, neg_margin=-1.0):
    if int(neg_pos_ub) != neg_pos_ub:
        raise ValueError(f'neg_pos_ub must be an integer ratio, got {neg_pos_ub}')
    return _lib.VknTrackLossCfg(float(softmax_temp), int(bool(has_aux)), float(w_track), float(w_aux), int(neg_pos_ub), float(pos_margin),
                                float(neg_margin))


def track_match_offsets(lengths, device):
    """int64 [B+1] offsets of the concatenated `gt_match_indices` as a device tensor, built from the host-known lengths with fill
    kernels only (no host-to-device copy: usable under stream capture)."""
    off = torch.zeros((len(lengths) + 1,), dtype=torch.int64, device=device)
    for i, n in enumerate(lengths):
        if n:
            off[i + 1:] += int(n)
    return off


def track_loss_fwd(cfg, key_embeds, ref_embeds, key_gt, ref_gt, match, match_off, want_kept=False):
    """The tracking loss of B images in one launch sequence (include/vkn_track_train.h: vkn_track_loss_fwd_f32).  key_embeds, ref_embeds
    fp32 [B,N,E]; key_gt, ref_gt int64 [B,N] (`gt_inds`: 0 = no ground truth); match int64 [n] / match_off int64 [B+1]: the images'
    `gt_match_indices` concatenated and their offsets; cfg: `track_loss_cfg(...)`.
    -> (losses fp32 [2] = (loss_track, loss_track_aux), stats int32 [B,4], aux_kept uint8 [B,N,N] | None, state): `state` is the
    workspace `track_loss_bwd` reads — a tensor of its own, so that it survives until the backward.  Out-of-range gt / match entries set
    VKN_STATUS_RANGE in this stream's status word (`workspace_status`)."""
    ke, re_ = _req(key_embeds, 'key_embeds'), _req(ref_embeds, 'ref_embeds')
    if ke.dim() != 3 or ke.shape != re_.shape:
        raise ValueError('key_embeds and ref_embeds must both be [B,N,E]')
    B, N, E = (int(v) for v in ke.shape)
    kg, rg = _req_int(key_gt, 'key_gt', torch.int64), _req_int(ref_gt, 'ref_gt', torch.int64)
    mt, mo = _req_int(match, 'match', torch.int64), _req_int(match_off, 'match_off', torch.int64)
    if kg.shape != (B, N) or rg.shape != (B, N) or mt.dim() != 1 or mo.shape != (B + 1,):
        raise ValueError('key_gt / ref_gt must be [B,N], match [n] and match_off [B+1]')
    dev = ke.device
    L = _lib.lib()
    losses = torch.empty((2,), dtype=torch.float32, device=dev)
    stats = torch.empty((B, 4), dtype=torch.int32, device=dev)
    kept = torch.empty((B, N, N), dtype=torch.uint8, device=dev) if want_kept else None
    state = torch.empty((max(L.vkn_track_loss_workspace_bytes(B, N), 256),), dtype=torch.uint8, device=dev)
    status = _workspace(256, dev)          # the header of this stream's workspace: its first word is the status word
    with torch.cuda.device(dev):
        check(L.vkn_track_loss_fwd_f32(ctypes.byref(cfg), _ptr(ke), _ptr(re_), _ptr(kg), _ptr(rg), _ptr(mt), _ptr(mo), int(mt.numel()), B, N, E,
                                       _ptr(losses), _ptr(stats), _ptr(kept), _ptr(status), _ptr(state), state.numel(), _stream()))
    return losses, stats, kept, state


def track_loss_bwd(cfg, key_embeds, ref_embeds, state, gout):
    """Gradients of `gout[0] * loss_track + gout[1] * loss_track_aux` w.r.t. the two embedding tensors (vkn_track_loss_bwd_f32).  gout:
    DEVICE fp32 [2]; state: the forward's.  -> (d_key, d_ref) fp32 [B,N,E], zero on rows without ground truth."""
    ke, re_, g = _req(key_embeds, 'key_embeds'), _req(ref_embeds, 'ref_embeds'), _req(gout, 'gout')
    B, N, E = (int(v) for v in ke.shape)
    if g.numel() != 2:
        raise ValueError('gout must hold the two upstream gradients')
    d_key, d_ref = torch.empty_like(ke), torch.empty_like(re_)
    with torch.cuda.device(ke.device):
        check(_lib.lib().vkn_track_loss_bwd_f32(ctypes.byref(cfg), _ptr(ke), _ptr(re_), _ptr(g), B, N, E, _ptr(d_key), _ptr(d_ref), _ptr(state),
                                                state.numel(), _stream()))
    return d_key, d_ref


GT_MAX_IMAGES, GT_MAX_CLASSES, GT_MAX_IDS = _lib.GT_MAX_IMAGES, _lib.GT_MAX_CLASSES, _lib.GT_MAX_IDS


def gt_prep_supported(B, Hp, Wp, stride):
    """The envelope of `gt_classes` / `gt_bank_fill` (include/vkn_gt.h) as far as shapes decide it."""
    return (1 <= B <= GT_MAX_IMAGES and stride in (1, 2, 4, 8) and Hp >= 1 and Wp >= 1 and Hp % stride == 0 and Wp % stride == 0
            and Hp * Wp < 2 ** 31 and Hp // stride <= 4 * 65535 and Hp <= 8 * 65535)     # the last two: the grids of the fill / the presence pass


def _req_bytes(t, name, dtypes=(torch.uint8,)):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.VknLibraryError(f'{name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if t.dtype == torch.bool:
        t = t.view(torch.uint8) if t.is_contiguous() else t.contiguous().view(torch.uint8)
    if t.dtype not in dtypes:
        raise TypeError(f'{name}: expected one of {dtypes}, got {t.dtype}')
    return t.contiguous()


def gt_classes(sem, valid, label_of_class):
    """Class presence and stuff labels of B semantic maps (vkn_gt_classes).  sem uint8 / int64 [B,Hp,Wp]; valid: per image
    (valid_h, valid_w); label_of_class: 256 ints, -1 = skip.  -> (n_sem int32 [B], classes uint8 [B,256], labels int64 [B,256],
    status int32 [1], raw): the first four are views of / next to `raw`, ONE uint8 buffer that holds status, counts and class lists, so
    that a caller reads all of them with one copy.  Nothing here synchronises."""
    sem = _req_bytes(sem, 'sem', (torch.uint8, torch.int64))
    B, Hp, Wp = (int(v) for v in sem.shape)
    if len(valid) != B or len(label_of_class) != GT_MAX_CLASSES:
        raise ValueError('gt_classes: one (valid_h, valid_w) per image and 256 labels')
    dev = sem.device
    step = Hp * Wp * sem.element_size()
    imgs = (_lib.VknGtImage * B)()
    for b, (vh, vw) in enumerate(valid):
        imgs[b] = _lib.VknGtImage(None, sem.data_ptr() + b * step, None, 0, 0, 0, int(vh), int(vw), 0, 0, 0)
    o_n, o_f, o_c = 4, 4 + 4 * B, 4 + 36 * B
    raw = torch.zeros(o_c + GT_MAX_CLASSES * B, dtype=torch.uint8, device=dev)      # status, n_sem [B], flags [B][8], classes [B][256]
    labels = torch.empty((B, GT_MAX_CLASSES), dtype=torch.int64, device=dev)
    table = (ctypes.c_int * GT_MAX_CLASSES)(*[int(v) for v in label_of_class])
    base = raw.data_ptr()
    with torch.cuda.device(dev):
        check(_lib.lib().vkn_gt_classes(imgs, B, Hp, Wp, int(sem.dtype == torch.int64), table, base + o_f, base + o_n, base + o_c,
                                        _ptr(labels), base, _stream()))
    return raw[o_n:o_f].view(torch.int32), raw[o_c:].view(B, GT_MAX_CLASSES), labels, raw[:4].view(torch.int32), raw


def gt_bank_fill(masks, sem, valid, n_sem, classes, stride, pad_shape, bank=None, device=None):
    """The fp32 bank [G_total, Hp / stride, Wp / stride] of a step in the training tail's row order (vkn_gt_bank_fill_f32): per image
    its thing rows, then its stuff rows.  masks: per image uint8 / bool [G_b,Hm_b,Wm_b] or None; sem uint8 / int64 [B,Hp,Wp] or None;
    valid: per image (valid_h, valid_w); n_sem: per image the HOST count of stuff rows, classes uint8 [B,256] their device class lists
    (`gt_classes`); pad_shape (Hp, Wp).  -> (bank, thing row0 per image, stuff row0 per image); `bank`: write into this tensor; `device`: where an
    empty bank lives when there is neither a mask nor a stuff row."""
    B, (Hp, Wp), s = len(masks), (int(v) for v in pad_shape), int(stride)
    masks = [None if m is None or m.shape[0] == 0 else _req_bytes(m, 'gt_masks') for m in masks]
    with_sem = sem is not None and any(n_sem)
    if with_sem:
        sem = _req_bytes(sem, 'sem', (torch.uint8, torch.int64))
        classes = _req_bytes(classes, 'classes')
        step = Hp * Wp * sem.element_size()
    dev = next((t.device for t in masks + [sem if with_sem else None, bank] if t is not None), device)
    imgs = (_lib.VknGtImage * B)()
    row, row0, sem_row0 = 0, [], []
    for b, m in enumerate(masks):
        G, ns = (int(m.shape[0]) if m is not None else 0), (int(n_sem[b]) if with_sem else 0)
        row0.append(row)
        sem_row0.append(row + G)
        imgs[b] = _lib.VknGtImage(m.data_ptr() if G else None, sem.data_ptr() + b * step if ns else None,
                                  classes.data_ptr() + b * GT_MAX_CLASSES if ns else None, G, int(m.shape[1]) if G else 0,
                                  int(m.shape[2]) if G else 0, int(valid[b][0]), int(valid[b][1]), ns, row, row + G)
        row += G + ns
    if bank is None:
        bank = torch.empty((row, Hp // s, Wp // s), dtype=torch.float32, device=dev)
    elif tuple(bank.shape) != (row, Hp // s, Wp // s) or bank.dtype != torch.float32 or not bank.is_contiguous() or not bank.is_cuda:
        raise ValueError(f'gt_bank_fill: bank must be a contiguous CUDA fp32 [{row}, {Hp // s}, {Wp // s}]')
    if row:
        with torch.cuda.device(bank.device):
            check(_lib.lib().vkn_gt_bank_fill_f32(imgs, B, Hp, Wp, s, int(with_sem and sem.dtype == torch.int64), _ptr(bank), row,
                                                  _stream()))
    return bank, row0, sem_row0


def gt_match_indices(key_ids, ref_ids):
    """`gt_match_indices` of B images in one launch (vkn_gt_match_indices): key_ids, ref_ids: per image an int64 tensor of instance
    ids.  -> (match int64 [sum], match_off int64 [B+1]): per key id the FIRST position among the image's reference ids, else -1 — the
    pair `track_loss_fwd` takes."""
    B = len(key_ids)
    if B != len(ref_ids) or B == 0:
        raise ValueError('gt_match_indices: one key and one reference id tensor per image')
    keys = [_req_int(k.reshape(-1), 'key_ids', torch.int64) for k in key_ids]
    refs = [_req_int(r.reshape(-1), 'ref_ids', torch.int64) for r in ref_ids]
    dev = keys[0].device
    kcat = torch.cat(keys) if B > 1 else keys[0]
    rcat = torch.cat(refs) if B > 1 else refs[0]
    match = torch.empty_like(kcat)
    off = torch.empty((B + 1,), dtype=torch.int64, device=dev)
    klen = (ctypes.c_int * B)(*[int(k.numel()) for k in keys])
    rlen = (ctypes.c_int * B)(*[int(r.numel()) for r in refs])
    with torch.cuda.device(dev):
        check(_lib.lib().vkn_gt_match_indices(_ptr(kcat) if kcat.numel() else None, klen, _ptr(rcat) if rcat.numel() else None, rlen, B,
                                              _ptr(match) if match.numel() else None, _ptr(off), _stream()))
    return match, off


# ---- the dense semantic loss of the kernel-initialisation head from the low-res logits (include/vkn_seg_loss.h)
_SEG = _lib.SEG
SEG_LOSS_FOCAL, SEG_LOSS_CE = _SEG['VKN_SEG_LOSS_FOCAL'], _SEG['VKN_SEG_LOSS_CE']
SEG_MAX_IMAGES, SEG_MAX_CLASSES, SEG_MAX_ROWS = _SEG['VKN_SEG_MAX_IMAGES'], _SEG['VKN_SEG_MAX_CLASSES'], _SEG['VKN_SEG_MAX_ROWS']


def seg_loss_supported(B, ncls, h, w, stride):
    """The envelope of `seg_targets` / `seg_loss_fwd` / `seg_loss_bwd` (include/vkn_seg_loss.h) as far as shapes decide it."""
    return (stride in (1, 2, 4) and 1 <= ncls <= SEG_MAX_CLASSES and 1 <= B <= SEG_MAX_IMAGES and h >= 1 and w >= 1
            and ncls * h * w * 4 < 2 ** 31 and stride * stride * h * w < 2 ** 31 and h <= 3 * 65535 and stride * h <= 4 * 65535)     # the last two: the grids of the backward / the targets


def _req_plain(t, name, dtype):
    """contiguous CUDA tensor of `dtype`, wherever it starts: views into a bank are taken as they are (4 / 8-byte alignment is theirs)"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.VknLibraryError(f'{name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if t.dtype != dtype:
        raise TypeError(f'{name}: expected {dtype}, got {t.dtype}')
    return t.contiguous()


def seg_targets(gt_masks, gt_labels, gt_sem_seg, gt_sem_cls, gt_inds, num_classes, shape, tgt=None, status=None):
    """The painted dense target map of B images in one launch (vkn_seg_targets_u8): per image gt_masks fp32 [G_b,H,W], gt_labels int64
    [G_b], gt_sem_seg fp32 [n_b,H,W] / gt_sem_cls int64 [n_b] (or None for both lists / entries: no stuff layer) and gt_inds int64 [Np]
    (the assigner's: 0 = unmatched).  shape = (H, W).  -> (tgt uint8 [B,H,W], dense_pos int32 [1]); `tgt`: write into this tensor;
    `status`: the int32 status word to use (default: this stream's, `workspace_status`).  Nothing here synchronises; the tensors named
    in the per-image array are kept alive by the caller until the stream has run the launch (they are the step's ground truth)."""
    B, (H, W) = len(gt_masks), (int(v) for v in shape)
    if not (len(gt_labels) == len(gt_inds) == B) or B == 0:
        raise ValueError('seg_targets: one mask, label and gt_inds tensor per image')
    imgs = (_lib.VknSegImage * B)()
    keep = []
    dev = gt_inds[0].device
    for b in range(B):
        gi = _req_plain(gt_inds[b].reshape(-1), 'gt_inds', torch.int64)
        G = int(gt_masks[b].shape[0]) if gt_masks[b] is not None else 0
        m = lab = s = sc = None
        if G:
            m, lab = _req_plain(gt_masks[b], 'gt_masks', torch.float32), _req_plain(gt_labels[b].reshape(-1), 'gt_labels', torch.int64)
            if tuple(m.shape[1:]) != (H, W) or lab.numel() != G:
                raise ValueError(f'seg_targets: gt_masks[{b}] must be [G, {H}, {W}] with G labels')
        ns = 0
        if gt_sem_seg is not None and gt_sem_cls is not None and gt_sem_seg[b] is not None and gt_sem_cls[b] is not None:
            ns = int(gt_sem_cls[b].numel())
        if ns:
            s, sc = _req_plain(gt_sem_seg[b], 'gt_sem_seg', torch.float32), _req_plain(gt_sem_cls[b].reshape(-1), 'gt_sem_cls', torch.int64)
            if tuple(s.shape) != (ns, H, W):
                raise ValueError(f'seg_targets: gt_sem_seg[{b}] must be [{ns}, {H}, {W}]')
        keep += [gi, m, lab, s, sc]
        imgs[b] = _lib.VknSegImage(m.data_ptr() if G else None, s.data_ptr() if ns else None, lab.data_ptr() if G else None,
                                   sc.data_ptr() if ns else None, gi.data_ptr() if gi.numel() else None, G, ns, int(gi.numel()))
    if tgt is None:
        tgt = torch.empty((B, H, W), dtype=torch.uint8, device=dev)
    elif tuple(tgt.shape) != (B, H, W) or tgt.dtype != torch.uint8 or not tgt.is_contiguous() or not tgt.is_cuda:
        raise ValueError(f'seg_targets: tgt must be a contiguous CUDA uint8 [{B}, {H}, {W}]')
    dense_pos = torch.empty((1,), dtype=torch.int32, device=dev)
    if status is None:
        status = _workspace(256, dev)          # the header of this stream's workspace: its first word is the status word
    with torch.cuda.device(dev):
        check(_lib.lib().vkn_seg_targets_u8(imgs, B, H, W, int(num_classes), _ptr(tgt), _ptr(dense_pos), _ptr(status), _stream()))
    return tgt, dense_pos


def seg_loss_fwd(low, tgt, dense_pos, mode, stride, alpha=0.25, gamma=2.0, loss_weight=1.0):
    """`loss_rpn_seg` from the low-res logits (vkn_seg_loss_fwd_f32).  low fp32 [B,ncls,h,w]; tgt uint8 [B,S h,S w] and dense_pos int32
    [1] as `seg_targets` returns them; mode SEG_LOSS_FOCAL / SEG_LOSS_CE.  -> (loss fp32 0-d, state): `state` is what `seg_loss_bwd`
    reads, a tensor of its own so that it survives until the backward."""
    low = _req_plain(low, 'low', torch.float32)
    B, ncls, h, w = (int(v) for v in low.shape)
    S = int(stride)
    tgt = _req_plain(tgt, 'tgt', torch.uint8)
    if tuple(tgt.shape) != (B, S * h, S * w):
        raise ValueError(f'seg_loss_fwd: tgt must be [{B}, {S * h}, {S * w}], got {tuple(tgt.shape)}')
    dp = _req_plain(dense_pos, 'dense_pos', torch.int32) if dense_pos is not None else None
    L = _lib.lib()
    loss = torch.empty((), dtype=torch.float32, device=low.device)
    state = torch.empty((max(L.vkn_seg_loss_state_bytes(int(mode), B, h, w, S), 64),), dtype=torch.uint8, device=low.device)
    with torch.cuda.device(low.device):
        check(L.vkn_seg_loss_fwd_f32(_ptr(low), _ptr(tgt), _ptr(dp), int(mode), B, ncls, h, w, S, float(alpha), float(gamma),
                                     float(loss_weight), _ptr(loss), _ptr(state), _stream()))
    return loss, state


def seg_loss_bwd(low, tgt, gout, state, mode, stride, alpha=0.25, gamma=2.0, grad_low=None):
    """gout x d loss / d low (vkn_seg_loss_bwd_f32).  gout: DEVICE fp32 scalar; state: the forward's.  -> grad_low fp32 [B,ncls,h,w]
    (`grad_low`: write into this contiguous tensor), every element written once."""
    low, tgt, g = _req_plain(low, 'low', torch.float32), _req_plain(tgt, 'tgt', torch.uint8), _req_plain(gout.reshape(-1), 'gout', torch.float32)
    B, ncls, h, w = (int(v) for v in low.shape)
    if g.numel() != 1:
        raise ValueError('gout must hold the one upstream gradient')
    if grad_low is None:
        grad_low = torch.empty_like(low)
    elif grad_low.shape != low.shape or grad_low.dtype != torch.float32 or not grad_low.is_contiguous() or not grad_low.is_cuda:
        raise ValueError('seg_loss_bwd: grad_low must be a contiguous CUDA fp32 tensor of the shape of low')
    with torch.cuda.device(low.device):
        check(_lib.lib().vkn_seg_loss_bwd_f32(_ptr(low), _ptr(tgt), _ptr(g), int(mode), B, ncls, h, w, int(stride), float(alpha), float(gamma),
                                              _ptr(state), _ptr(grad_low), _stream()))
    return grad_low


def panoptic_thing_first(thing_masks, thing_scores, thing_labels, thing_order, stuff_masks, stuff_labels, stuff_order,
                         instance_score_thr, iou_thr, stuff_max_area):
    """Thing-first panoptic merge of ONE image on the device (`merge_stuff_thing`, knet/det/kernel_iter_head.py:385-465).
    thing_masks [Kt,H,W] / stuff_masks [Ks,H,W] bool, scores fp32, labels / orders int; `*_order` = the paste order (indices into
    the mask arrays).  Returns device tensors (panoptic_seg int32 [H,W], info int32 [Kt+Ks,5], nseg int32 [1]); see include/vkn.h."""
    dev = thing_masks.device
    if not thing_masks.is_cuda:
        raise _lib.VknLibraryError('panoptic_thing_first: expected CUDA/HIP tensors — the MI355X path has no CPU fallback')
    H, W = thing_masks.shape[-2:]
    HW = H * W
    Kt, Ks = thing_masks.shape[0], stuff_masks.shape[0]
    tm = thing_masks.to(torch.uint8).contiguous()
    sm = stuff_masks.to(torch.uint8).contiguous()
    i32 = lambda t: t.to(device=dev, dtype=torch.int32).contiguous()  # noqa: E731
    ts, tl, to, sl, so = thing_scores.float().contiguous(), i32(thing_labels), i32(thing_order), i32(stuff_labels), i32(stuff_order)
    L = _lib.lib()
    seg = torch.empty((H, W), dtype=torch.int32, device=dev)
    info = torch.zeros((Kt + Ks, 5), dtype=torch.int32, device=dev)
    nseg = torch.zeros((1,), dtype=torch.int32, device=dev)
    ws = _workspace(max(L.vkn_merge_workspace_bytes(Kt, Ks), 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_panoptic_thing_first_u8(_ptr(tm), _ptr(ts), tl.data_ptr(), to.data_ptr(), Kt, _ptr(sm), sl.data_ptr(), so.data_ptr(),
                                            Ks, HW, float(instance_score_thr), float(iou_thr), int(stuff_max_area), seg.data_ptr(),
                                            info.data_ptr(), nseg.data_ptr(), _ptr(ws), ws.numel(), _stream()))
    return seg, info, nseg


def assign_costs(mask_logits, cls_logits, gt_masks, gt_labels, cls_weight=2.0, dice_weight=4.0, mask_weight=1.0,
                 focal_alpha=0.25, focal_gamma=2.0, focal_eps=1e-12, dice_eps=1e-3, dice_pred_min=1e-3, mask_pred_min=1e-2,
                 labels_checked=False):
    """Cost matrix [N, G] of `MaskHungarianAssigner.assign` (knet/det/mask_hungarian_assigner.py:222-241) on the GPU.
    dice_pred_min / mask_pred_min: the lower clamp of sigmoid(logits) in DiceCost / MaskCost (knet: 1e-3 / 1e-2; knet_vis: none)."""
    m = _req(mask_logits.reshape(mask_logits.shape[0], -1), 'mask_preds')
    g = _req(gt_masks.reshape(gt_masks.shape[0], -1).float(), 'gt_masks')
    N, P = m.shape
    G = g.shape[0]
    if g.shape[1] != P:
        raise ValueError('mask_preds and gt_masks must have the same spatial size')
    cls = _req(cls_logits, 'cls_pred') if cls_logits is not None else None
    ncls = cls.shape[1] if cls is not None else 0
    lab = gt_labels.to(device=m.device, dtype=torch.int32).contiguous()
    if cls is not None and lab.numel() and not labels_checked:
        # the reference's `cls_pred[:, gt_labels]` raises an IndexError for labels outside the logits (ignore label 255, stuff label
        # against thing-only logits); an unchecked device read would silently produce garbage costs.  Host labels are checked on the
        # host; device labels cost ONE combined read (the cost matrix itself goes to the host for the LSAP right after)
        src = gt_labels if not gt_labels.is_cuda else torch.stack(torch.aminmax(lab))
        lo, hi = (int(v) for v in (src.min(), src.max())) if not gt_labels.is_cuda else (int(v) for v in src.tolist())
        if lo < 0 or hi >= ncls:
            raise IndexError(f'gt_labels outside [0, {ncls}): {lo} .. {hi}')
    cfg = _lib.VknAssignCfg(float(cls_weight), float(dice_weight), float(mask_weight), float(focal_alpha), float(focal_gamma),
                            float(focal_eps), float(dice_eps), float(dice_pred_min), float(mask_pred_min))
    L = _lib.lib()
    cost = torch.empty((N, G), dtype=torch.float32, device=m.device)
    nb = L.vkn_assign_workspace_bytes(N, G, P)
    ws = _workspace(max(nb, 256), m.device, scratch=True)
    with torch.cuda.device(m.device):
        check(L.vkn_assign_costs_f32(ctypes.byref(cfg), _ptr(m), _ptr(cls), _ptr(g), lab.data_ptr(), N, G, ncls, P, _ptr(cost),
                                     _ptr(ws), ws.numel(), _stream()))
    return cost


_LABS32 = {}


def _labels_i32(gt_labels, dev):
    """the batch's labels as ONE int32 tensor — the same tensors arrive once per stage: built once per (tensor identities, versions)"""
    import weakref
    key = tuple((l.data_ptr(), l._version, tuple(l.shape), str(l.device)) for l in gt_labels) + (str(dev),)
    hit = _LABS32.get(key)
    if hit is not None and all(r() is l for r, l in zip(hit[0], gt_labels)):
        return hit[1]
    if len(_LABS32) > 16:
        _LABS32.clear()
    labs = torch.cat([l.reshape(-1) for l in gt_labels]).to(device=dev, dtype=torch.int32)
    _LABS32[key] = ([weakref.ref(l) for l in gt_labels], labs)
    return labs


def assign_costs_batch(mask_logits, cls_logits, gt_masks, gt_labels, cls_weight=2.0, dice_weight=4.0, mask_weight=1.0,
                       focal_alpha=0.25, focal_gamma=2.0, focal_eps=1e-12, dice_eps=1e-3, dice_pred_min=1e-3, mask_pred_min=1e-2):
    """`assign_costs` for the images of a batch in ONE C call (vkn_assign_costs_batch_f32): lists of per-image [N, H, W] logits,
    [N, ncls] class logits (or None for all), [G_b, H, W] float ground-truth masks and [G_b] labels — ALREADY range-checked (the
    per-image entry point checks; this one is the training loop's).  -> list of [N, G_b] cost matrices (views of one allocation)."""
    n = len(mask_logits)
    N = mask_logits[0].shape[0]
    P = mask_logits[0][0].numel()
    dev = mask_logits[0].device
    use_cls = cls_logits is not None and cls_logits[0] is not None and cls_weight != 0
    ncls = cls_logits[0].shape[1] if use_cls else 0
    Gs = [int(g.shape[0]) for g in gt_masks]
    labs = _labels_i32(gt_labels, dev) if use_cls else None
    cost = torch.empty((N * sum(Gs),), dtype=torch.float32, device=dev)
    probs = (_lib.VknAssignProblem * n)()
    keep, out, off = [], [], 0
    for b in range(n):
        m = _req(mask_logits[b].reshape(N, P), 'mask_preds')
        g = gt_masks[b].reshape(Gs[b], -1)
        if g.dtype != torch.float32:
            g = g.float()
        g = _req(g, 'gt_masks')
        if g.shape[1] != P or m.shape[0] != N:
            raise ValueError('mask_preds and gt_masks must have the same spatial size, and every image the same number of predictions')
        c = _req(cls_logits[b], 'cls_pred') if use_cls else None
        cb = cost[N * off:N * (off + Gs[b])].view(N, Gs[b])
        probs[b] = _lib.VknAssignProblem(m.data_ptr(), c.data_ptr() if use_cls else None, g.data_ptr(),
                                         labs.data_ptr() + 4 * off if use_cls else None, Gs[b], cb.data_ptr())
        keep += [m, g, c]
        out.append(cb)
        off += Gs[b]
    cfg = _lib.VknAssignCfg(float(cls_weight if use_cls else 0.0), float(dice_weight), float(mask_weight), float(focal_alpha),
                            float(focal_gamma), float(focal_eps), float(dice_eps), float(dice_pred_min), float(mask_pred_min))
    L = _lib.lib()
    ws = _workspace(max(L.vkn_assign_workspace_bytes(N, max(Gs), P), 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_assign_costs_batch_f32(ctypes.byref(cfg), probs, n, N, ncls, P, _ptr(ws), ws.numel(), _stream()))
    return out


def assign_costs_lowres_supported(N, Gs, h, w, stride):
    """Does `assign_costs_lowres_batch` take this shape?  (include/vkn.h: vkn_assign_costs_lowres_batch_f32)"""
    return bool(Gs) and len(Gs) <= 16 and min(Gs) > 0 and \
        _lib.lib().vkn_assign_lowres_workspace_bytes(len(Gs), int(N), max(Gs), int(h), int(w), int(stride)) > 0


def assign_costs_lowres_batch(low_logits, stride, cls_logits, gt_masks, gt_labels, cls_weight=2.0, dice_weight=4.0, mask_weight=1.0,
                              focal_alpha=0.25, focal_gamma=2.0, focal_eps=1e-12, dice_eps=1e-3, dice_pred_min=1e-3, mask_pred_min=1e-2):
    """`assign_costs_batch` on the LOW-RES logits: per-image [N, h, w] logits whose x`stride` bilinear up-scaling the reference assigns
    on, [G_b, stride h, stride w] ground truths — interpolation, activation and contraction in one kernel for the whole batch
    (vkn_assign_costs_lowres_batch_f32: the up-scaled predictions are never read).  Labels ALREADY range-checked.
    -> list of [N, G_b] cost matrices (views of one allocation)."""
    n = len(low_logits)
    N, h, w = (int(v) for v in low_logits[0].shape)
    dev = low_logits[0].device
    use_cls = cls_logits is not None and cls_logits[0] is not None and cls_weight != 0
    ncls = cls_logits[0].shape[1] if use_cls else 0
    Gs = [int(g.shape[0]) for g in gt_masks]
    labs = _labels_i32(gt_labels, dev) if use_cls else None
    cost = torch.empty((N * sum(Gs),), dtype=torch.float32, device=dev)
    probs = (_lib.VknAssignProblem * n)()
    keep, out, off = [], [], 0
    for b in range(n):
        m = _req(low_logits[b], 'mask_preds')
        g = gt_masks[b]
        if g.dtype != torch.float32:
            g = g.float()
        g = _req(g, 'gt_masks')
        if tuple(m.shape) != (N, h, w) or tuple(g.shape[1:]) != (stride * h, stride * w):
            raise ValueError('every image needs [N, h, w] logits and [G, stride h, stride w] ground-truth masks')
        c = _req(cls_logits[b], 'cls_pred') if use_cls else None
        cb = cost[N * off:N * (off + Gs[b])].view(N, Gs[b])
        probs[b] = _lib.VknAssignProblem(m.data_ptr(), c.data_ptr() if use_cls else None, g.data_ptr(),
                                         labs.data_ptr() + 4 * off if use_cls else None, Gs[b], cb.data_ptr())
        keep += [m, g, c]
        out.append(cb)
        off += Gs[b]
    cfg = _lib.VknAssignCfg(float(cls_weight if use_cls else 0.0), float(dice_weight), float(mask_weight), float(focal_alpha),
                            float(focal_gamma), float(focal_eps), float(dice_eps), float(dice_pred_min), float(mask_pred_min))
    L = _lib.lib()
    nb = L.vkn_assign_lowres_workspace_bytes(n, N, max(Gs), h, w, int(stride))
    if nb == 0:
        raise ValueError('shape outside vkn_assign_costs_lowres_batch_f32 (ops.assign_costs_lowres_supported)')
    ws = _workspace(max(nb, 256), dev, scratch=True)
    with torch.cuda.device(dev):
        check(L.vkn_assign_costs_lowres_batch_f32(ctypes.byref(cfg), probs, n, N, ncls, h, w, int(stride), _ptr(ws), ws.numel(), _stream()))
    return out


def focal_loss_fwd(logits, labels, row_weight, alpha, gamma):
    """Sigmoid focal loss in one pass (include/vkn.h: vkn_focal_loss_f32).  logits [M, ncls] fp32, labels int64 [M], row_weight [M] |
    [M, ncls] | None -> (sum of the weighted element losses: 0-d tensor, d sum / d logits [M, ncls])."""
    z = _req(logits, 'cls_score')
    M, ncls = z.shape
    lab = labels.to(device=z.device, dtype=torch.int64).contiguous()
    ew = row_weight is not None and row_weight.numel() == M * ncls and ncls > 1
    w = None
    if row_weight is not None:
        w = _req(row_weight.reshape((M, ncls) if ew else (M,)).float(), 'label_weights')
    L = _lib.lib()
    part = torch.empty((L.vkn_focal_loss_blocks(M, ncls),), dtype=torch.float32, device=z.device)
    grad = torch.empty_like(z)
    with torch.cuda.device(z.device):
        check(L.vkn_focal_loss_f32(_ptr(z), lab.data_ptr(), _ptr(w), int(ew), M, ncls, float(alpha), float(gamma), _ptr(part), _ptr(grad),
                                   _stream()))
    return part.sum(), grad


def mask_losses_fwd(pred, target, pos_rows, rowk, B, with_rank):
    """Forward sums of the three mask losses (include/vkn.h: vkn_mask_losses_fwd_f32).  pred, target [R, P]; pos_rows int64 [K]; rowk
    int32 [R].  -> (rowstats [K, 4] = (sum bce, sum p t, sum p^2, sum t^2), lse [B, P] | None, top int32 [B, P] | None,
    rank_sum scalar tensor | None)."""
    pred, target = _req(pred, 'pred'), _req(target, 'target')
    R, P = pred.shape
    K, Ns = int(pos_rows.shape[0]), R // B
    L = _lib.lib()
    nch, nbl = L.vkn_mask_losses_chunks(P), L.vkn_mask_losses_blocks(P)
    dev = pred.device
    rp = torch.empty((K, nch, 4), dtype=torch.float32, device=dev)
    lse = torch.empty((B, P), dtype=torch.float32, device=dev) if with_rank else None
    top = torch.empty((B, P), dtype=torch.int32, device=dev) if with_rank else None
    rkp = torch.empty((B, nbl), dtype=torch.float32, device=dev) if with_rank else None
    with torch.cuda.device(dev):
        check(L.vkn_mask_losses_fwd_f32(_ptr(pred), _ptr(target), pos_rows.data_ptr() if K else None, rowk.data_ptr(), K, B, Ns, P,
                                        1 if with_rank else 0, _ptr(rp) if K else None, _ptr(lse), top.data_ptr() if with_rank else None,
                                        _ptr(rkp), _stream()))
    return rp.sum(dim=1), lse, top, (rkp.sum() if with_rank else None)


def mask_losses_bwd(pred, target, rowk, rowcoef, coef, lse, top, B, with_rank):
    """Gradient of the three mask losses w.r.t. pred [R, P] in one pass (vkn_mask_losses_bwd_f32)."""
    pred, target = _req(pred, 'pred'), _req(target, 'target')
    R, P = pred.shape
    grad = torch.empty_like(pred)
    with torch.cuda.device(pred.device):
        check(_lib.lib().vkn_mask_losses_bwd_f32(_ptr(pred), _ptr(target), rowk.data_ptr(), _ptr(rowcoef), _ptr(coef), _ptr(lse),
                                                 top.data_ptr() if with_rank else None, B, R // B, P, 1 if with_rank else 0,
                                                 _ptr(grad), _stream()))
    return grad


_POW2_SCRATCH = {}


def pow2_scale(t, target_log2=10):
    """-> device float32 [8] with [0] = the power of two s putting max|t| into [2^(target_log2 - 1), 2^target_log2) and [4] = 1 / s
    (vkn_pow2_scale_f32: one launch, nothing read on the host).  `scale_of(s8)` / `inv_of(s8)` give the two as 16-byte aligned views."""
    t = _req(t.detach(), 't')
    dev = t.device
    key = (dev, torch.cuda.current_stream(dev).cuda_stream)
    scr = _POW2_SCRATCH.get(key)
    if scr is None:
        scr = _POW2_SCRATCH[key] = torch.zeros(2, dtype=torch.int32, device=dev)     # the kernel leaves it zero again
    out = torch.empty(8, dtype=torch.float32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().vkn_pow2_scale_f32(_ptr(t), t.numel(), int(target_log2), _ptr(out), scr.data_ptr(), _stream()))
    return out


def scale_of(s8):
    return s8[0:1]


def inv_of(s8):
    return s8[4:5]


def scale_pad_rows(t, scale, mult=32):
    """t [B, R, ...] * scale (device scalar or None) with the rows zero-padded to a multiple of `mult` (vkn_scale_pad_rows_f32)."""
    t = _req(t, 't')
    B, R = t.shape[:2]
    P = t[0, 0].numel()
    Rp = (R + mult - 1) // mult * mult
    out = torch.empty((B, Rp) + tuple(t.shape[2:]), dtype=torch.float32, device=t.device)
    with torch.cuda.device(t.device):
        check(_lib.lib().vkn_scale_pad_rows_f32(_ptr(t), _ptr(scale), B, R, Rp, P, _ptr(out), _stream()))
    return out


def transpose_pad(k, scale, Np):
    """k [B, N, C] -> [B, C, Np] = k^T * scale (device scalar or None), columns N .. Np zero (vkn_transpose_pad_f32)."""
    k = _req(k, 'k')
    B, N, C = k.shape
    out = torch.empty((B, C, Np), dtype=torch.float32, device=k.device)
    with torch.cuda.device(k.device):
        check(_lib.lib().vkn_transpose_pad_f32(_ptr(k), _ptr(scale), B, N, C, int(Np), _ptr(out), _stream()))
    return out


def threshold_rows_f16(mask_logits, hard_mask_thr, mult=32):
    """[B, N, H, W] logits -> fp16 [B, Np, H, W] = (logit >= thr_logit(hard_mask_thr)), rows padded with zeros to a multiple of `mult`."""
    m = _req(mask_logits, 'mask_logits')
    B, N = m.shape[:2]
    P = m[0, 0].numel()
    Np = (N + mult - 1) // mult * mult
    out = torch.empty((B, Np) + tuple(m.shape[2:]), dtype=torch.float16, device=m.device)
    with torch.cuda.device(m.device):
        check(_lib.lib().vkn_threshold_rows_f16(_ptr(m), thr_logit(hard_mask_thr), B, N, Np, P, _ptr(out), _stream()))
    return out


def unscale_rows(dk_p, dkb_p, scale, N):
    """(dk_p [B, Np, C], dkb_p [B, Np]) -> (dk [B, N, C], dkb [B, N]) = the first N rows times the device scalar (vkn_unscale_rows_f32)."""
    dk_p, dkb_p = _req(dk_p, 'dk'), _req(dkb_p, 'dkb')
    B, Np, C = dk_p.shape
    dk = torch.empty((B, N, C), dtype=torch.float32, device=dk_p.device)
    dkb = torch.empty((B, N), dtype=torch.float32, device=dk_p.device)
    with torch.cuda.device(dk_p.device):
        check(_lib.lib().vkn_unscale_rows_f32(_ptr(dk_p), _ptr(dkb_p), _ptr(scale), B, int(N), Np, C, _ptr(dk), _ptr(dkb), _stream()))
    return dk, dkb


SUM_MAX = _H['VKN_SUM_MAX']


def sum_tensors(parts):
    """parts[0] + parts[1] + ... (same shape; in that order) in ONE pass for fp32 CUDA tensors (vkn_sum_n_f32), else torch adds."""
    if len(parts) == 1:
        return parts[0]
    p0 = parts[0]
    if not (p0.is_cuda and all(p.dtype == torch.float32 and p.shape == p0.shape and p.device == p0.device for p in parts)):
        out = parts[0] + parts[1]
        for p in parts[2:]:
            out = out + p
        return out
    out = None
    while len(parts) > 1:
        take = [_req(p, 'part') for p in parts[:SUM_MAX]]
        arr = (ctypes.c_void_p * len(take))(*[p.data_ptr() for p in take])
        out = torch.empty_like(take[0])
        with torch.cuda.device(p0.device):
            check(_lib.lib().vkn_sum_n_f32(arr, len(take), out.numel(), _ptr(out), _stream()))
        parts = [out] + list(parts[SUM_MAX:])
    return out


def check_range(values, lo, hi, flag, status):
    """*status (device int32 [1]) |= flag when an element of the integer tensor `values` lies outside [lo, hi) (vkn_check_range_i64)."""
    v = values.reshape(-1)
    if v.dtype != torch.int64 or not v.is_contiguous():
        v = v.to(torch.int64).contiguous()
    with torch.cuda.device(v.device):
        check(_lib.lib().vkn_check_range_i64(v.data_ptr(), v.numel(), int(lo), int(hi), int(flag), status.data_ptr(), _stream()))


def lsap_device(costs):
    """`scipy.optimize.linear_sum_assignment` for a batch of DEVICE cost matrices [nr_b, nc_b] (fp32) without leaving the device:
    one launch, one wavefront per matrix (include/vkn.h: vkn_lsap_batch_f32).  -> (gt_inds, row_ind, col_ind, status):
    per matrix gt_inds int64 [nr] (matched column + 1, 0 = unmatched: the reference's `assigned_gt_inds`), the min(nr, nc) matched
    (row, col) pairs sorted by row (int32), and ONE int32 status tensor [batch] (0 ok, 1 invalid entries, 2 infeasible) that
    the caller may read whenever it wants to pay for the synchronisation."""
    if not costs:
        return [], [], [], None
    dev = costs[0].device
    probs = (_lib.VknLsapProblem * len(costs))()
    gts, rows, cols, keep = [], [], [], []
    for b, c in enumerate(costs):
        c = _req(c, 'cost')
        if c.dim() != 2 or c.shape[0] == 0 or c.shape[1] == 0:
            raise ValueError(f'cost {b}: expected a non-empty 2-D matrix, got {tuple(c.shape)}')
        nr, nc = c.shape
        k = min(nr, nc)
        g = torch.empty(nr, dtype=torch.int64, device=dev)
        r = torch.empty(k, dtype=torch.int32, device=dev)
        cc = torch.empty(k, dtype=torch.int32, device=dev)
        probs[b] = _lib.VknLsapProblem(c.data_ptr(), nr, nc, g.data_ptr(), r.data_ptr(), cc.data_ptr())
        gts.append(g); rows.append(r); cols.append(cc); keep.append(c)
    status = torch.empty(len(costs), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        check(_lib.lib().vkn_lsap_batch_f32(probs, len(costs), status.data_ptr(), _stream()))
    for c in keep:                       # the launch is asynchronous: the matrices must outlive it on this stream
        c.record_stream(torch.cuda.current_stream(dev))
    return gts, rows, cols, status


def lsap(cost):
    """`scipy.optimize.linear_sum_assignment(cost)` on a host fp32 matrix through libvkn's C++ solver -> (row_ind, col_ind)
    int64 numpy arrays (knet/det/mask_hungarian_assigner.py:244-251)."""
    import numpy as np
    c = np.ascontiguousarray(cost.detach().cpu().numpy() if torch.is_tensor(cost) else cost, dtype=np.float32)
    nr, nc = c.shape
    k = min(nr, nc)
    rows, cols = np.empty(k, dtype=np.int32), np.empty(k, dtype=np.int32)
    n = _lib.lib().vkn_lsap_f32(c.ctypes.data, nr, nc, rows.ctypes.data, cols.ctypes.data)
    if n < 0:
        check(n)
    return rows[:n].astype(np.int64), cols[:n].astype(np.int64)


# ---------------------------------------------------------------------------------------------------------- localization FPN
def _conv_out(n, stride):
    """Output size of the block's convs (3x3 pad 1, 1x1 pad 0): ceil(n / stride)"""
    return (n - 1) // stride + 1


def conv_prepare(weight):
    """One conv weight [Cout, Cin, k, k] -> its prepared image (uint8 tensor of vkn_conv_weight_bytes): f16 hi / lo MFMA fragments,
    pre-scaled by a power of two (include/vkn.h: vkn_conv_prepare_f32).  Regenerate whenever the weight changes."""
    w = _req(weight.detach(), 'conv weight')
    Cout, Cin, kh, kw = w.shape
    L = _lib.lib()
    nb = L.vkn_conv_weight_bytes(Cout, Cin, kh) if kh == kw else 0
    if not nb:
        raise ValueError(f'conv weight {tuple(w.shape)}: needs k in (1, 3), Cout and Cin multiples of 32')
    img = torch.empty(nb, dtype=torch.uint8, device=w.device)
    with torch.cuda.device(w.device):
        check(L.vkn_conv_prepare_f32(_ptr(w), Cout, Cin, kh, _ptr(img), nb, _stream()))
    return img


def conv_gn(x, image, Cout, ksize, stride=1, groups=32, pos=None, in_stats=None, in_gamma=None, in_beta=None, upsample=False):
    """The building block (include/vkn.h: vkn_conv_gn_f32): a 3x3 (or 1x1) conv of `x` — raw (+ `pos`), or a previous conv's RAW
    output GroupNorm'ed (in_stats [B, G_in, 2] = (mean, rstd), in_gamma / in_beta) and ReLU'd on load, optionally bilinear x2 on load —
    returning (raw output [B, Cout, Ho, Wo], its (mean, rstd) per (frame, group) [B, groups, 2])."""
    x = _req(x, 'x')
    B, Cin, H, W = x.shape
    Hin, Win = (2 * H, 2 * W) if upsample else (H, W)
    Ho, Wo = _conv_out(Hin, stride), _conv_out(Win, stride)
    dev = x.device
    out = torch.empty((B, Cout, Ho, Wo), dtype=torch.float32, device=dev)
    st = torch.empty((B, groups, 2), dtype=torch.float32, device=dev)
    ins = _req(in_stats, 'in_stats') if in_stats is not None else None
    L = _lib.lib()
    nb = L.vkn_conv_gn_workspace_bytes(B, Cout, H, W, stride, int(bool(upsample)))
    if not nb:
        raise ValueError('conv_gn: shape outside the envelope')
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        check(L.vkn_conv_gn_f32(_ptr(x), _ptr(_req(pos, 'pos') if pos is not None else None), _ptr(ins),
                                _ptr(_req(in_gamma, 'in_gamma') if ins is not None else None),
                                _ptr(_req(in_beta, 'in_beta') if ins is not None else None), ins.shape[1] if ins is not None else 0,
                                int(bool(upsample)), _ptr(image), int(ksize), int(stride), int(groups), _ptr(out), _ptr(st),
                                B, Cin, H, W, int(Cout), _ptr(ws), ws.numel(), _stream()))
    return out, st


def localization_fpn(p2, p3, p4, p5, pos5, images, gammas, betas, groups):
    """`SemanticFPNWrapper` of the shipped configs (+ the head's loc / seg convs when `images` has ten entries) in ONE C-ABI call
    (include/vkn.h: vkn_localization_fpn_f32).  images / gammas / betas in the header's order; returns (loc, sem) [B, C, H3, W3]
    — with eight images the module's own outputs (out, aux).  Range violations are reported through `workspace_status`."""
    ps = [_req(p, f'P{i + 2}') for i, p in enumerate((p2, p3, p4, p5))]
    B, C = ps[0].shape[:2]
    if any(p.shape[:2] != (B, C) for p in ps):
        raise ValueError('P2..P5 must share batch and channel counts')
    dims = [int(d) for p in ps for d in p.shape[2:]]
    dev = ps[0].device
    L = _lib.lib()
    nb = L.vkn_localization_fpn_workspace_bytes(B, C, *dims)
    if not nb:
        raise _lib.VknError(-2, 'localization_fpn: the levels do not reach one stride-8 grid (ceil(H2/2) = H3 = 2 H4 = 4 H5)')
    H3, W3 = dims[2], dims[3]
    loc = torch.empty((B, C, H3, W3), dtype=torch.float32, device=dev)
    sem = torch.empty_like(loc)
    n = len(images)
    if n not in (8, 10):
        raise ValueError('localization_fpn takes 8 or 10 prepared images')
    arr = lambda ts: (ctypes.c_void_p * 10)(*[t.data_ptr() for t in ts], *([None] * (10 - len(ts))))  # noqa: E731
    gs = [_req(g, 'gn.weight') for g in gammas]
    bs = [_req(b, 'gn.bias') for b in betas]
    pos = _req(pos5, 'pos') if pos5 is not None else None
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        check(L.vkn_localization_fpn_f32(*[_ptr(p) for p in ps], _ptr(pos), arr(images), arr(gs), arr(bs), int(groups),
                                         _ptr(loc), _ptr(sem), B, C, *dims, _ptr(ws), ws.numel(), _stream()))
    return loc, sem


# ---- backward of one conv + GroupNorm + ReLU block (include/vkn_fpn_train.h)
def gn_relu_apply(r, stats, gamma, beta):
    """y = relu(GN(r)) from a RAW conv output r [B, C, H, W] and the (mean, rstd) [B, groups, 2] that `conv_gn` returned with it
    (include/vkn_fpn_train.h: vkn_gn_relu_apply_f32)."""
    r, stats = _req(r, 'r'), _req(stats, 'stats')
    B, C, H, W = r.shape
    y = torch.empty_like(r)
    with torch.cuda.device(r.device):
        check(_lib.lib().vkn_gn_relu_apply_f32(_ptr(r), _ptr(stats), _ptr(_req(gamma, 'gamma')), _ptr(_req(beta, 'beta')), stats.shape[1],
                                               _ptr(y), B, C, H, W, _stream()))
    return y


def gn_relu_bwd(dy, r, stats, gamma, beta):
    """(dr, dgamma, dbeta) of y = relu(GN(r)) from the gradient dy of y (vkn_gn_relu_bwd_f32): the ReLU mask is recomputed from r,
    the sums are merged in a fixed order in fp64.  A non-finite dy is reported through `workspace_status`."""
    dy, r, stats = _req(dy, 'dy'), _req(r, 'r'), _req(stats, 'stats')
    if dy.shape != r.shape:
        raise ValueError(f'gn_relu_bwd: dy {tuple(dy.shape)} and r {tuple(r.shape)} differ')
    B, C, H, W = r.shape
    G, dev = stats.shape[1], r.device
    L = _lib.lib()
    nb = L.vkn_gn_relu_bwd_workspace_bytes(B, C, H, W, G)
    if not nb:
        raise ValueError('gn_relu_bwd: shape outside the envelope')
    dr = torch.empty_like(r)
    dgamma = torch.empty(C, dtype=torch.float32, device=dev)
    dbeta = torch.empty_like(dgamma)
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        check(L.vkn_gn_relu_bwd_f32(_ptr(dy), _ptr(r), _ptr(stats), _ptr(_req(gamma, 'gamma')), _ptr(_req(beta, 'beta')), G, _ptr(dr),
                                    _ptr(dgamma), _ptr(dbeta), B, C, H, W, _ptr(ws), ws.numel(), _stream()))
    return dr, dgamma, dbeta


def conv_wgrad(dr, x, ksize, stride=1):
    """dW [Cout, Cin, k, k] of a conv (padding k // 2, no bias) from the gradient dr [B, Cout, Ho, Wo] of its raw output and its input
    x [B, Cin, H, W] (vkn_conv_wgrad_f32): MFMA over B Ho Wo, both operands scaled by a power of two per tensor."""
    dr, x = _req(dr, 'dr'), _req(x, 'x')
    B, Cin, H, W = x.shape
    Cout, dev = dr.shape[1], x.device
    if tuple(dr.shape) != (B, Cout, _conv_out(H, stride), _conv_out(W, stride)):
        raise ValueError(f'conv_wgrad: dr {tuple(dr.shape)} is not the output of x {tuple(x.shape)} at stride {stride}')
    L = _lib.lib()
    nb = L.vkn_conv_wgrad_workspace_bytes(B, Cin, H, W, Cout, int(ksize), int(stride))
    if not nb:
        raise ValueError('conv_wgrad: shape outside the envelope')
    dw = torch.empty((Cout, Cin, ksize, ksize), dtype=torch.float32, device=dev)
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        check(L.vkn_conv_wgrad_f32(_ptr(dr), _ptr(x), _ptr(dw), B, Cin, H, W, Cout, int(ksize), int(stride), _ptr(ws), ws.numel(), _stream()))
    return dw


def conv_dgrad(dr, image_t, Cin, H, W, ksize, stride=1):
    """dx [B, Cin, H, W] of a conv from dr [B, Cout, Ho, Wo] (vkn_conv_dgrad_f32).  `image_t` is
    `conv_prepare(weight.flip(2, 3).transpose(0, 1))`: the flipped, channel-transposed weight as the forward engine's A operand."""
    dr = _req(dr, 'dr')
    B, Cout = dr.shape[:2]
    if tuple(dr.shape[2:]) != (_conv_out(H, stride), _conv_out(W, stride)):
        raise ValueError(f'conv_dgrad: dr {tuple(dr.shape)} is not the output of a {H} x {W} input at stride {stride}')
    L = _lib.lib()
    nb = L.vkn_conv_dgrad_workspace_bytes(B, Cout, H, W, int(stride))
    if not nb or image_t.numel() != L.vkn_conv_weight_bytes(int(Cin), Cout, int(ksize)):
        raise ValueError('conv_dgrad: shape outside the envelope, or an image of another weight')
    dev = dr.device
    dx = torch.empty((B, Cin, H, W), dtype=torch.float32, device=dev)
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        check(L.vkn_conv_dgrad_f32(_ptr(dr), _ptr(image_t), _ptr(dx), B, int(Cin), H, W, Cout, int(ksize), int(stride), _ptr(ws), ws.numel(),
                                   _stream()))
    return dx


def conv_gn_relu_fits(Cin, Cout, ksize, stride, groups):
    """The envelope of the block's forward and backward kernels (include/vkn_fpn_train.h; csrc/vkn_convtile.h: chan_ok, conv_ok)"""
    return (Cin % 32 == 0 and Cout % 32 == 0 and 0 < Cin <= 512 and 0 < Cout <= 512 and groups > 0 and Cout % groups == 0
            and (ksize, stride) in ((3, 1), (3, 2), (1, 1)))


# ------------------------------------------------------------------------------------------- deformable-attention neck
_MSDA = _lib.MSDA


def msda_fits(M, D, L, P):
    """The envelope of the sampling core (include/vkn_msda.h), sizes aside"""
    return (D in (16, 32, 64) and M > 0 and (M * D) % 32 == 0 and M * D <= _MSDA['VKN_MSDA_MAX_CHANNELS']
            and 1 <= L <= _MSDA['VKN_MSDA_MAX_LEVELS'] and 1 <= P <= _MSDA['VKN_MSDA_MAX_POINTS'])


def _req_rows(t, name, width):
    """A [rows, >= width] fp32 view whose rows may be strided (a column range of a GEMM output): (tensor, row stride in floats)"""
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _lib.VknLibraryError(f'{name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if t.dtype != torch.float32:
        raise TypeError(f'{name}: expected float32, got {t.dtype}')
    if t.dim() != 2 or t.shape[1] != width:
        raise ValueError(f'{name}: expected [rows, {width}], got {tuple(t.shape)}')
    if t.stride(1) != 1 or t.stride(0) < width:
        t = t.contiguous()
    if t.data_ptr() % 16:
        t = t.clone(memory_format=torch.contiguous_format)
    return t, t.stride(0)


def msda_sample(value, spatial_shapes, offsets, logits, ref, num_heads, num_points):
    """The sampling core of multi-scale deformable attention (include/vkn_msda.h: vkn_msda_sample_f32).  value [B, S, M D] with the
    levels of `spatial_shapes` = [(H_l, W_l)] concatenated; offsets [B Q, 2 M L P] and logits [B Q, M L P], the raw outputs of the
    `sampling_offsets` / `attention_weights` Linears (column ranges of one GEMM output are taken as they are, by row stride);
    ref [Q, L, 2] normalised (x, y).  -> [B, Q, M D]."""
    value, ref = _req(value, 'value'), _req(ref, 'ref')
    B, S, C = value.shape
    M, P, L = int(num_heads), int(num_points), len(spatial_shapes)
    Q = ref.shape[0]
    if C % M or tuple(ref.shape) != (Q, L, 2) or sum(int(h) * int(w) for h, w in spatial_shapes) != S:
        raise ValueError(f'msda_sample: value {tuple(value.shape)}, ref {tuple(ref.shape)}, levels {list(spatial_shapes)}, {M} heads do not fit')
    offsets, ld_off = _req_rows(offsets, 'offsets', 2 * M * L * P)
    logits, ld_logits = _req_rows(logits, 'logits', M * L * P)
    if offsets.shape[0] != B * Q or logits.shape[0] != B * Q:
        raise ValueError(f'msda_sample: {offsets.shape[0]} offset rows, {logits.shape[0]} logit rows for B Q = {B * Q}')
    out = torch.empty((B, Q, C), dtype=torch.float32, device=value.device)
    shapes = (ctypes.c_int * (2 * L))(*[int(v) for hw in spatial_shapes for v in hw])
    with torch.cuda.device(value.device):
        check(_lib.lib().vkn_msda_sample_f32(_ptr(value), _ptr(offsets), ld_off, _ptr(logits), ld_logits, _ptr(ref), shapes, _ptr(out),
                                             B, Q, M, C // M, L, P, _stream()))
    return out


def _msda_shapes(spatial_shapes):
    return (ctypes.c_int * (2 * len(spatial_shapes)))(*[int(v) for hw in spatial_shapes for v in hw])


def msda_bwd_workspace_bytes(spatial_shapes, B, Q, num_heads, head_dim, num_points):
    """vkn_msda_bwd_workspace_bytes (include/vkn_msda_train.h): the bytes `msda_sample_bwd` needs, 0 outside its envelope"""
    return int(_lib.lib().vkn_msda_bwd_workspace_bytes(_msda_shapes(spatial_shapes), int(B), int(Q), int(num_heads), int(head_dim),
                                                       len(spatial_shapes), int(num_points)))


def msda_sample_bwd(value, spatial_shapes, offsets, logits, ref, dout, num_heads, num_points, grad_rows=None):
    """The backward of `msda_sample` (include/vkn_msda_train.h: vkn_msda_sample_bwd_f32) from its own operands and the gradient
    dout [B, Q, M D] of its output -> (dvalue [B, S, M D], doff [B Q, 2 M L P], dlogits [B Q, M L P]).  No float atomics: two calls give
    the same bits.  `grad_rows`: an optional [B Q, 3 M L P] fp32 buffer that receives doff | dlogits side by side (the mirror of the
    forward's one GEMM output); the two gradients returned are then its column ranges.  A non-finite dout or contribution is reported
    through `workspace_status`."""
    value, ref, dout = _req(value, 'value'), _req(ref, 'ref'), _req(dout, 'dout')
    B, S, C = value.shape
    M, P, L = int(num_heads), int(num_points), len(spatial_shapes)
    Q = ref.shape[0]
    if C % M or tuple(ref.shape) != (Q, L, 2) or sum(int(h) * int(w) for h, w in spatial_shapes) != S or tuple(dout.shape) != (B, Q, C):
        raise ValueError(f'msda_sample_bwd: value {tuple(value.shape)}, ref {tuple(ref.shape)}, dout {tuple(dout.shape)}, levels '
                         f'{list(spatial_shapes)}, {M} heads do not fit')
    n_off, n_log = 2 * M * L * P, M * L * P
    offsets, ld_off = _req_rows(offsets, 'offsets', n_off)
    logits, ld_logits = _req_rows(logits, 'logits', n_log)
    if offsets.shape[0] != B * Q or logits.shape[0] != B * Q:
        raise ValueError(f'msda_sample_bwd: {offsets.shape[0]} offset rows, {logits.shape[0]} logit rows for B Q = {B * Q}')
    dev = value.device
    if grad_rows is None:
        doff = torch.empty((B * Q, n_off), dtype=torch.float32, device=dev)
        dlogits = torch.empty((B * Q, n_log), dtype=torch.float32, device=dev)
    else:
        if (not torch.is_tensor(grad_rows) or grad_rows.dtype != torch.float32 or grad_rows.device != dev or not grad_rows.is_contiguous()
                or tuple(grad_rows.shape) != (B * Q, n_off + n_log) or grad_rows.data_ptr() % 16):
            raise ValueError(f'msda_sample_bwd: grad_rows must be a contiguous, 16-byte aligned fp32 [{B * Q}, {n_off + n_log}] on {dev}')
        doff, dlogits = grad_rows[:, :n_off], grad_rows[:, n_off:]
    L_ = _lib.lib()
    shapes = _msda_shapes(spatial_shapes)
    nb = L_.vkn_msda_bwd_workspace_bytes(shapes, B, Q, M, C // M, L, P)
    if not nb:
        raise ValueError('msda_sample_bwd: shape outside the envelope')
    dvalue = torch.empty_like(value)
    ws = _workspace(nb, dev)
    with torch.cuda.device(dev):
        check(L_.vkn_msda_sample_bwd_f32(_ptr(value), _ptr(offsets), ld_off, _ptr(logits), ld_logits, _ptr(ref), shapes, _ptr(dout),
                                         _ptr(dvalue), _ptr(doff), doff.stride(0), _ptr(dlogits), dlogits.stride(0), B, Q, M, C // M, L, P,
                                         _ptr(ws), ws.numel(), _stream()))
    return dvalue, doff, dlogits


def layernorm_act(x, gamma, beta, resid=None, eps=1e-5, act=0):
    """act(LayerNorm(x + resid) gamma + beta) per row of [rows, C <= 256] (include/vkn.h: vkn_layernorm_act_fwd_f32), no gradient"""
    x = _req(x, 'x')
    M, C = x.shape
    resid = _req(resid, 'resid') if resid is not None else None
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        check(_lib.lib().vkn_layernorm_act_fwd_f32(_ptr(x), C, _ptr(resid), C, _ptr(_req(gamma, 'gamma')), _ptr(_req(beta, 'beta')),
                                                   float(eps), int(act), _ptr(out), C, None, M, C, _stream()))
    return out


def _four_maps(who, state, gt_sem, gt_ins, pred_sem, pred_ins):
    """(maps, B, HW) of a map meter's update: four int32 tensors [H,W] or [B,H,W] of one shape on the state's device."""
    maps = [_req_plain(m, name, torch.int32) for m, name in zip((gt_sem, gt_ins, pred_sem, pred_ins), ('gt_sem', 'gt_ins', 'pred_sem', 'pred_ins'))]
    shape = tuple(maps[0].shape)
    if len(shape) not in (2, 3) or any(tuple(m.shape) != shape or m.device != state.device for m in maps):
        raise ValueError(f'{who}: four int32 maps [H,W] or [B,H,W] of one shape on the state\'s device, got {[tuple(m.shape) for m in maps]}')
    return maps, (shape[0] if len(shape) == 3 else 1), shape[-2] * shape[-1]


# ---- the STQ meter (include/vkn_stq.h): one caller-owned state per sequence
def stq_cfg(num_classes, ignore_label, label_bit_shift, offset, drop_ignored_gt=True, cap_gt=2048, cap_pred=8192, cap_pair=32768):
    """The `VknStqCfg` of a meter; raises VknError (VKN_E_SHAPE) outside the envelope of include/vkn_stq.h."""
    cfg = _lib.VknStqCfg(int(offset), int(num_classes), int(ignore_label), int(label_bit_shift), int(bool(drop_ignored_gt)), int(cap_gt),
                         int(cap_pred), int(cap_pair))
    if not _lib.lib().vkn_stq_state_bytes(ctypes.byref(cfg)):
        raise _lib.VknError(-2, 'stq_cfg: outside the envelope of include/vkn_stq.h (classes 1..255, shift 1..30, offset >= classes << shift, '
                                '((classes + 1) << shift) * offset < 2^62, capacities powers of two in [16, 2^20])')
    return cfg


def stq_layout(cfg):
    """(state bytes, the eight byte offsets: header, confusion, gt keys, gt counts, pred keys, pred counts, pair keys, pair counts)"""
    off = (ctypes.c_size_t * 8)()
    check(_lib.lib().vkn_stq_state_layout(ctypes.byref(cfg), off))
    return int(_lib.lib().vkn_stq_state_bytes(ctypes.byref(cfg))), [int(o) for o in off]


def stq_state(cfg, device):
    """A freshly reset state of one sequence: uint8 [vkn_stq_state_bytes] on `device`."""
    state = torch.empty((stq_layout(cfg)[0],), dtype=torch.uint8, device=device)
    return stq_reset(cfg, state)


def stq_reset(cfg, state):
    """Empty the state (vkn_stq_reset, one fill launch); returns it."""
    with torch.cuda.device(state.device):
        check(_lib.lib().vkn_stq_reset(ctypes.byref(cfg), _ptr(state), state.numel(), _stream()))
    return state


def stq_update(cfg, state, is_thing, gt_sem, gt_ins, pred_sem, pred_ins):
    """Count B frames of one sequence into `state` (vkn_stq_update_i32, one launch, no synchronisation).  The four maps: int32 CUDA
    tensors [H,W] or [B,H,W] of one shape; is_thing uint8 [n]."""
    maps, B, HW = _four_maps('stq_update', state, gt_sem, gt_ins, pred_sem, pred_ins)
    thing = _req_plain(is_thing, 'is_thing', torch.uint8)
    if thing.numel() < cfg.num_classes or thing.device != state.device:
        raise ValueError(f'stq_update: is_thing must hold at least num_classes = {cfg.num_classes} bytes on the state\'s device')
    with torch.cuda.device(state.device):
        check(_lib.lib().vkn_stq_update_i32(ctypes.byref(cfg), _ptr(state), state.numel(), _ptr(thing), *[_ptr(m) for m in maps], int(B), int(HW),
                                            _stream()))


# ---- the VPQ meter (include/vkn_vpq.h): one caller-owned state per sequence
def vpq_cfg(num_cat, ks=(1,), ign_id=255, label_bit_shift=16, offset=2 ** 30, cap_gt=512, cap_pred=512, cap_pair=2048, cap_log=131072):
    """The `VknVpqCfg` of a meter; raises VknError (VKN_E_SHAPE) outside the envelope of include/vkn_vpq.h."""
    ks = tuple(int(k) for k in ks)
    if not 1 <= len(ks) <= _lib.VPQ['VKN_VPQ_MAX_KS']:
        raise _lib.VknError(-2, f'vpq_cfg: 1 to {_lib.VPQ["VKN_VPQ_MAX_KS"]} window lengths, got {ks}')
    cfg = _lib.VknVpqCfg(int(offset), int(num_cat), int(ign_id), int(label_bit_shift), len(ks),
                         (ctypes.c_int * _lib.VPQ['VKN_VPQ_MAX_KS'])(*ks), int(cap_gt), int(cap_pred), int(cap_pair), int(cap_log))
    if not _lib.lib().vkn_vpq_state_bytes(ctypes.byref(cfg)):
        raise _lib.VknError(-2, 'vpq_cfg: outside the envelope of include/vkn_vpq.h (num_cat 1..255 <= ign_id <= 255, shift 1..30, '
                                'offset >= num_cat << shift, ((ign_id + 1) << shift) * offset < 2^62, ks ascending in 1..8, '
                                'capacities powers of two in [16, 2^20])')
    return cfg


def vpq_layout(cfg):
    """(state bytes, the four byte offsets: header, acc, log, private)"""
    off = (ctypes.c_size_t * 4)()
    check(_lib.lib().vkn_vpq_state_layout(ctypes.byref(cfg), off))
    return int(_lib.lib().vkn_vpq_state_bytes(ctypes.byref(cfg))), [int(o) for o in off]


def vpq_state(cfg, device):
    """A freshly reset state of one sequence: uint8 [vkn_vpq_state_bytes] on `device`."""
    state = torch.empty((vpq_layout(cfg)[0],), dtype=torch.uint8, device=device)
    return vpq_reset(cfg, state)


def vpq_reset(cfg, state):
    """Empty the state (vkn_vpq_reset, one fill); returns it."""
    with torch.cuda.device(state.device):
        check(_lib.lib().vkn_vpq_reset(ctypes.byref(cfg), _ptr(state), state.numel(), _stream()))
    return state


def vpq_update(cfg, state, gt_sem, gt_ins, pred_sem, pred_ins):
    """Count B consecutive frames of one sequence into `state` and close every window that ends in them (vkn_vpq_update_i32, three
    launches per VKN_VPQ_GROUP frames, no synchronisation).  The four maps: int32 CUDA tensors [H,W] or [B,H,W] of one shape."""
    maps, B, HW = _four_maps('vpq_update', state, gt_sem, gt_ins, pred_sem, pred_ins)
    with torch.cuda.device(state.device):
        check(_lib.lib().vkn_vpq_update_i32(ctypes.byref(cfg), _ptr(state), state.numel(), *[_ptr(m) for m in maps], int(B), int(HW), _stream()))


# ---- COCO run-length encoding of instance masks (include/vkn_rle.h): caller-owned pools
def rle_workspace_bytes(K, H, W):
    """vkn_rle_workspace_bytes: bytes of one call's workspace, 0 outside the envelope of include/vkn_rle.h."""
    return int(_lib.lib().vkn_rle_workspace_bytes(int(K), int(H), int(W)))


def rle_encode(masks, records, runs, pool, status, ws, thr=None):
    """Encode K masks (vkn_rle_encode_u8 / vkn_rle_encode_f32, eight launches, no synchronisation).  masks: bool or uint8 [K,H,W]
    (nonzero = set), or float32 [K,H,W] with `thr` (set iff v > thr).  records int32 [K, VKN_RLE_RECORD_INTS], runs uint32-as-int32
    [cap_runs], pool uint8 [cap_bytes], status int32 [1] (sticky: cleared by the caller), ws uint8 [rle_workspace_bytes(K, H, W)]: CUDA
    tensors of the caller, written in place."""
    if torch.is_tensor(masks) and masks.is_cuda and masks.dtype == torch.float32:
        if thr is None:
            raise ValueError('rle_encode: float32 logits need `thr`')
        src = _req(masks, 'masks')
    else:
        if thr is not None:
            raise ValueError('rle_encode: `thr` goes with float32 logits only')
        src = _req_bytes(masks, 'masks')
        if src.data_ptr() % 16:
            src = src.clone()
    if src.dim() != 3:
        raise ValueError(f'rle_encode: masks [K,H,W], got {tuple(src.shape)}')
    K, H, W = src.shape
    records, runs, status = (_req_plain(t, n, torch.int32) for t, n in ((records, 'records'), (runs, 'runs'), (status, 'status')))
    pool, ws = _req_plain(pool, 'pool', torch.uint8), _req_plain(ws, 'ws', torch.uint8)
    if records.numel() != K * _lib.RLE['VKN_RLE_RECORD_INTS'] or status.numel() < 1 or any(t.device != src.device for t in (records, runs, pool, status, ws)):
        raise ValueError('rle_encode: records int32 [K, VKN_RLE_RECORD_INTS], status int32 [1], everything on the masks\' device')
    L = _lib.lib()
    tail = (K, H, W, _ptr(records), _ptr(runs), runs.numel(), _ptr(pool), pool.numel(), _ptr(status), _ptr(ws), ws.numel(), _stream())
    with torch.cuda.device(src.device):
        if thr is None:
            check(L.vkn_rle_encode_u8(_ptr(src), *tail))
        else:
            check(L.vkn_rle_encode_f32(_ptr(src), float(thr), *tail))


# ---- COCO mask AP (include/vkn_maskap.h): exact overlap tables, and the per-image matching into a caller-owned state
def mask_overlap_workspace_bytes(K, G, H, W):
    """vkn_mask_overlap_workspace_bytes: bytes of one call's workspace; 0 outside the envelope of include/vkn_maskap.h and for K = G = 0."""
    return int(_lib.lib().vkn_mask_overlap_workspace_bytes(int(K), int(G), int(H), int(W)))


def mask_overlap(dt, gt, thr=None, out=None):
    """Pairwise overlap of K detections and G ground truths (vkn_mask_overlap_u8 / _f32: two packs and one overlap launch, no
    synchronisation).  dt: bool or uint8 [K,H,W] (nonzero = set), or float32 [K,H,W] with `thr` (set iff v > thr); gt: bool or uint8
    [G,H,W].  K = 0 and G = 0 are valid.  -> (inter int64 [K,G], area_dt int64 [K], area_gt int64 [G]) on the masks' device; with
    `out` (such a triple) the call ADDS into it and returns it: per frame of a video, that yields tube overlaps."""
    for t, name in ((dt, 'dt'), (gt, 'gt')):
        if not torch.is_tensor(t) or not t.is_cuda:
            raise _lib.VknLibraryError(f'mask_overlap: {name}: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
    if dt.dtype == torch.float32:
        if thr is None:
            raise ValueError('mask_overlap: float32 logits need `thr`')
        d = _req(dt, 'dt')
    else:
        if thr is not None:
            raise ValueError('mask_overlap: `thr` goes with float32 logits only')
        d = _req_bytes(dt, 'dt')
    g = _req_bytes(gt, 'gt')
    if d.dim() != 3 or g.dim() != 3 or d.shape[1:] != g.shape[1:] or d.device != g.device:
        raise ValueError(f'mask_overlap: dt [K,H,W] and gt [G,H,W] of one size on one device, got {tuple(d.shape)} and {tuple(g.shape)}')
    d, g = (t.clone() if t.data_ptr() % 16 else t for t in (d, g))
    K, H, W = (int(s) for s in d.shape)
    G = int(g.shape[0])
    elem = 4 if thr is not None else 1
    need = mask_overlap_workspace_bytes(K, G, H, W)
    if (K + G and not need) or K * H * W * elem >= 2 ** 31:
        raise _lib.VknError(-2, f'mask_overlap: {K} x {G} masks of {H} x {W} are outside the envelope of include/vkn_maskap.h '
                                f'(K, G <= {_lib.MASKAP["VKN_MASKAP_MAX_MASKS"]}, H * W < 2^31, max(K, G) * H * W * element size < 2^31)')
    if out is None:
        flat = torch.zeros((K * G + K + G + 6,), dtype=torch.int64, device=d.device)        # one fill; each table on a 16-byte boundary
        a, b = (K * G + 1) // 2 * 2, (K * G + 1) // 2 * 2 + (K + 1) // 2 * 2
        out = flat[:K * G].view(K, G), flat[a:a + K], flat[b:b + G]
    inter, area_dt, area_gt = (_req_plain(t, n, torch.int64) for t, n in zip(out, ('inter', 'area_dt', 'area_gt')))
    if tuple(inter.shape) != (K, G) or tuple(area_dt.shape) != (K,) or tuple(area_gt.shape) != (G,) or any(t.device != d.device for t in (inter, area_dt, area_gt)):
        raise ValueError(f'mask_overlap: out = (int64 [{K},{G}], int64 [{K}], int64 [{G}]) on the masks\' device')
    if K + G == 0:
        return inter, area_dt, area_gt
    ws = _workspace(need, d.device, scratch=True)[:need]
    L = _lib.lib()
    opt = lambda t: _ptr(t if t.numel() else None)          # noqa: E731  (an empty side travels as NULL)
    tail = (opt(g), K, G, H, W, opt(inter), opt(area_dt), opt(area_gt), _ptr(ws), need, _stream())
    with torch.cuda.device(d.device):
        if thr is None:
            check(L.vkn_mask_overlap_u8(opt(d), *tail))
        else:
            check(L.vkn_mask_overlap_f32(opt(d), float(thr), *tail))
    return inter, area_dt, area_gt


def mask_ap_cfg(num_classes, iou_thrs, area_ranges, max_det, cap_records):
    """The `VknMaskApCfg` of a meter; raises VknError (VKN_E_SHAPE) outside the envelope of include/vkn_maskap.h."""
    C = _lib.MASKAP
    thrs, areas = [float(t) for t in iou_thrs], [(float(lo), float(hi)) for lo, hi in area_ranges]
    if not 1 <= len(thrs) <= C['VKN_MASKAP_MAX_THRS'] or not 1 <= len(areas) <= C['VKN_MASKAP_MAX_AREAS']:
        raise _lib.VknError(-2, f'mask_ap_cfg: 1 to {C["VKN_MASKAP_MAX_THRS"]} IoU thresholds and 1 to {C["VKN_MASKAP_MAX_AREAS"]} area ranges, '
                                f'got {len(thrs)} and {len(areas)}')
    cfg = _lib.VknMaskApCfg()
    cfg.iou_thrs[:len(thrs)] = thrs
    cfg.area_lo[:len(areas)], cfg.area_hi[:len(areas)] = [a[0] for a in areas], [a[1] for a in areas]
    cfg.num_classes, cfg.T, cfg.A, cfg.max_det, cfg.cap_records = int(num_classes), len(thrs), len(areas), int(max_det), int(cap_records)
    if not _lib.lib().vkn_mask_ap_state_bytes(ctypes.byref(cfg)):
        raise _lib.VknError(-2, f'mask_ap_cfg: outside the envelope of include/vkn_maskap.h (num_classes 1..{C["VKN_MASKAP_MAX_CLASSES"]}, '
                                f'max_det 1..{C["VKN_MASKAP_MAX_MASKS"]}, capacity 1..2^24, no NaN)')
    return cfg


def mask_ap_layout(cfg):
    """(state bytes, the three byte offsets: header, npig, log)"""
    off = (ctypes.c_size_t * 3)()
    check(_lib.lib().vkn_mask_ap_state_layout(ctypes.byref(cfg), off))
    return int(_lib.lib().vkn_mask_ap_state_bytes(ctypes.byref(cfg))), [int(o) for o in off]


def mask_ap_state(cfg, device):
    """A freshly reset state: uint8 [vkn_mask_ap_state_bytes] on `device`."""
    state = torch.empty((mask_ap_layout(cfg)[0],), dtype=torch.uint8, device=device)
    return mask_ap_reset(cfg, state)


def mask_ap_reset(cfg, state):
    """Empty the state (vkn_mask_ap_reset, one fill); returns it."""
    with torch.cuda.device(state.device):
        check(_lib.lib().vkn_mask_ap_reset(ctypes.byref(cfg), _ptr(state), state.numel(), _stream()))
    return state


def mask_ap_match(cfg, state, tables, scores, dt_labels, gt_labels, gt_crowd, gt_area=None, image_seq=0, match_gt=None):
    """Match one image into `state` (vkn_mask_ap_match, three launches, no synchronisation).  tables: `mask_overlap`'s triple; scores
    float32 [K], dt_labels int32 [K], gt_labels int32 [G], gt_crowd uint8 [G], gt_area float64 [G] or None (the pixel count),
    match_gt int32 [A,T,K] or None: CUDA tensors on the state's device."""
    inter, area_dt, area_gt = (_req_plain(t, n, torch.int64) for t, n in zip(tables, ('inter', 'area_dt', 'area_gt')))
    K, G = int(area_dt.numel()), int(area_gt.numel())
    scores = _req_plain(scores, 'scores', torch.float32)
    dt_labels, gt_labels = _req_plain(dt_labels, 'dt_labels', torch.int32), _req_plain(gt_labels, 'gt_labels', torch.int32)
    gt_crowd = _req_bytes(gt_crowd, 'gt_crowd')
    gt_area = _req_plain(gt_area, 'gt_area', torch.float64) if gt_area is not None else None
    match_gt = _req_plain(match_gt, 'match_gt', torch.int32) if match_gt is not None else None
    if (inter.numel() != K * G or scores.numel() != K or dt_labels.numel() != K or gt_labels.numel() != G or gt_crowd.numel() != G
            or (gt_area is not None and gt_area.numel() != G) or (match_gt is not None and match_gt.numel() != cfg.A * cfg.T * K)):
        raise ValueError(f'mask_ap_match: tables of {K} detections and {G} ground truths need scores, dt_labels [{K}], gt_labels, gt_crowd, '
                         f'gt_area [{G}] and match_gt [{cfg.A},{cfg.T},{K}]')
    if any(t is not None and t.device != state.device for t in (inter, area_dt, area_gt, scores, dt_labels, gt_labels, gt_crowd, gt_area, match_gt)):
        raise ValueError('mask_ap_match: everything on the state\'s device')
    opt = lambda t: _ptr(t if t is not None and t.numel() else None)          # noqa: E731
    with torch.cuda.device(state.device):
        check(_lib.lib().vkn_mask_ap_match(ctypes.byref(cfg), _ptr(state), state.numel(), opt(inter), opt(area_dt), opt(area_gt), opt(scores),
                                           opt(dt_labels), opt(gt_labels), opt(gt_crowd), opt(gt_area), K, G, int(image_seq), opt(match_gt), _stream()))


# ---- instance masks as bits straight from the head's mask logits (include/vkn_instmask.h): the fused rescale, and the two consumers of bits
def rescale_masks_torch(logits, img_meta, up=1):
    """The reference's chain in torch, on the logits' device: interp_up (up > 1 only) -> sigmoid -> bilinear to batch_input_shape -> crop
    to img_shape -> bilinear to ori_shape (knet/det/kernel_update_head.py:443-458).  -> float [K,Ho,Wo]."""
    import torch.nn.functional as F
    x = logits.unsqueeze(0)
    if up > 1:
        x = F.interpolate(x, scale_factor=up, mode='bilinear', align_corners=False)
    h, w = img_meta['img_shape'][:2]
    x = F.interpolate(x.sigmoid(), size=tuple(img_meta['batch_input_shape']), mode='bilinear', align_corners=False)[:, :, :h, :w]
    return F.interpolate(x, size=tuple(img_meta['ori_shape'][:2]), mode='bilinear', align_corners=False).squeeze(0)


def pack_mask_bits_torch(masks):
    """bool [K,H,W] -> int64 [K, ceil(W / 64), H] in the layout of csrc/vkn_maskbits.h, in torch on the masks' device (the torch path of
    `instance_mask_bits`: CPU tensors and geometries outside the envelope)."""
    K, H, W = (int(s) for s in masks.shape)
    NS = (W + 63) // 64
    pad = torch.zeros((K, H, NS * 64), dtype=torch.int64, device=masks.device)
    pad[:, :, :W] = masks.to(torch.int64)
    words = (pad.view(K, H, NS, 64) << torch.arange(64, dtype=torch.int64, device=masks.device)).sum(-1)      # disjoint bits: the sum is the OR (bit 63 wraps to the sign)
    return words.permute(0, 2, 1).contiguous()


def instance_mask_cfg(Hm, Wm, img_meta, up=1):
    """The `VknInstMaskCfg` of one image: logits [*, Hm, Wm], mmdet's img_meta (img_shape, batch_input_shape, ori_shape)."""
    cfg = _lib.VknInstMaskCfg()
    cfg.up, cfg.Hm, cfg.Wm = int(up), int(Hm), int(Wm)
    cfg.Hb, cfg.Wb = (int(v) for v in img_meta['batch_input_shape'])
    cfg.h, cfg.w = (int(v) for v in img_meta['img_shape'][:2])
    cfg.Ho, cfg.Wo = (int(v) for v in img_meta['ori_shape'][:2])
    return cfg


def instance_bits_workspace_bytes(cfg, K):
    """vkn_instance_bits_workspace_bytes: bytes of one call's workspace, 0 outside the envelope of include/vkn_instmask.h."""
    return int(_lib.lib().vkn_instance_bits_workspace_bytes(ctypes.byref(cfg), int(K)))


def instance_bits_fused(logits, img_meta, K, up=1):
    """Does `instance_mask_bits` run the kernel for these logits (a CUDA float32 [N,Hm,Wm] tensor, a geometry inside the envelope), or
    the torch path?"""
    if not (torch.is_tensor(logits) and logits.is_cuda and logits.dtype == torch.float32 and logits.dim() == 3 and up in (1, 2, 4)):
        return False
    if any(int(v) >= 1 << 24 for v in (*logits.shape, *img_meta['batch_input_shape'], *img_meta['img_shape'][:2], *img_meta['ori_shape'][:2])):
        return False
    return instance_bits_workspace_bytes(instance_mask_cfg(logits.shape[1], logits.shape[2], img_meta, up), K) > 0


def instance_mask_bits(logits, img_meta, thr, rows=None, up=1, status=None):
    """Instance masks as bits (vkn_instance_bits_f32: one fill, one launch, no synchronisation): for entry k,
    interp(interp(sigmoid(interp_up(logits[rows[k]])), batch_input_shape)[:h, :w], ori_shape) > thr.  logits float32 [N,Hm,Wm]: with
    up = 1 the head's scaled mask predictions, with up in (2, 4) its stride-8 logits; rows: int tensor / list [K] (any order, duplicates
    allowed) or None = every row; thr: one fp32 comparison, torch's `>`.  -> int64 [K, ceil(Wo / 64), Ho]: bit c of word [k, s, y] is
    pixel (y, 64 s + c), the bits behind Wo are zero — what `rle_encode_bits` and `mask_overlap_bits` read.  `status`: an int32 [4] CUDA
    tensor that takes the call's status word (VKN_INSTMASK_STATUS_*) instead of the stream's scratch buffer.
    CPU tensors and geometries outside the envelope take the torch path: `rescale_masks_torch(...) > thr`, packed in torch."""
    if not torch.is_tensor(logits) or logits.dim() != 3:
        raise ValueError(f'instance_mask_bits: logits [N,Hm,Wm], got {tuple(logits.shape) if torch.is_tensor(logits) else type(logits)}')
    N = int(logits.shape[0])
    if rows is not None:
        rows = torch.as_tensor(rows, device=logits.device).reshape(-1)
    K = N if rows is None else int(rows.numel())
    Ho, Wo = (int(v) for v in img_meta['ori_shape'][:2])
    if K == 0:
        return torch.zeros((0, (Wo + 63) // 64, Ho), dtype=torch.int64, device=logits.device)
    if not instance_bits_fused(logits, img_meta, K, up):
        sel = logits if rows is None else logits.index_select(0, rows.long())
        return pack_mask_bits_torch(rescale_masks_torch(sel.float(), img_meta, up) > thr)
    src = _req(logits, 'logits')
    cfg = instance_mask_cfg(src.shape[1], src.shape[2], img_meta, up)
    r = rows.to(torch.int32).contiguous() if rows is not None else None
    bits = torch.empty((K, (Wo + 63) // 64, Ho), dtype=torch.int64, device=src.device)
    need = _lib.INSTMASK['VKN_INSTMASK_WS_BYTES']
    ws = _req_plain(status, 'status', torch.int32).view(torch.uint8)[:need] if status is not None else _workspace(need, src.device, scratch=True)[:need]
    with torch.cuda.device(src.device):
        check(_lib.lib().vkn_instance_bits_f32(ctypes.byref(cfg), _ptr(src), N, _ptr(r), K, float(thr), _ptr(bits), _ptr(ws), need, _stream()))
    return bits


def rle_bits_workspace_bytes(K, H, W):
    """vkn_bits_rle_workspace_bytes: bytes of one `rle_encode_bits` call's workspace, 0 outside the envelope of include/vkn_rle.h."""
    return int(_lib.lib().vkn_bits_rle_workspace_bytes(int(K), int(H), int(W)))


def rle_encode_bits(bits, W, records, runs, pool, status, ws):
    """`rle_encode` on masks that are bits already (vkn_bits_rle_encode, seven launches, no synchronisation).  bits int64
    [K, ceil(W / 64), H] as `instance_mask_bits` returns them; the other tensors as in `rle_encode`, ws uint8
    [rle_bits_workspace_bytes(K, H, W)]."""
    b = _req_plain(bits, 'bits', torch.int64)
    if b.dim() != 3 or b.shape[1] != (int(W) + 63) // 64:
        raise ValueError(f'rle_encode_bits: bits [K, ceil(W / 64), H] for W = {W}, got {tuple(b.shape)}')
    K, _, H = (int(s) for s in b.shape)
    records, runs, status = (_req_plain(t, n, torch.int32) for t, n in ((records, 'records'), (runs, 'runs'), (status, 'status')))
    pool, ws = _req_plain(pool, 'pool', torch.uint8), _req_plain(ws, 'ws', torch.uint8)
    if records.numel() != K * _lib.RLE['VKN_RLE_RECORD_INTS'] or status.numel() < 1 or any(t.device != b.device for t in (records, runs, pool, status, ws)):
        raise ValueError('rle_encode_bits: records int32 [K, VKN_RLE_RECORD_INTS], status int32 [1], everything on the bits\' device')
    with torch.cuda.device(b.device):
        check(_lib.lib().vkn_bits_rle_encode(_ptr(b), K, H, int(W), _ptr(records), _ptr(runs), runs.numel(), _ptr(pool), pool.numel(), _ptr(status),
                                             _ptr(ws), ws.numel(), _stream()))


def mask_overlap_bits_workspace_bytes(K, G, H, W):
    """vkn_bits_mask_overlap_workspace_bytes: bytes of one `mask_overlap_bits` call's workspace (the ground truths as bits); 0 outside the
    envelope of include/vkn_maskap.h and for G = 0."""
    return int(_lib.lib().vkn_bits_mask_overlap_workspace_bytes(int(K), int(G), int(H), int(W)))


def mask_overlap_bits(bits, W, gt, out=None):
    """`mask_overlap` with the detections as bits (vkn_bits_mask_overlap: one pack and one overlap launch).  bits int64
    [K, ceil(W / 64), H] as `instance_mask_bits` returns them; gt bool / uint8 [G,H,W].  -> (inter int64 [K,G], area_dt int64 [K],
    area_gt int64 [G]); with `out` the call ADDS into that triple."""
    d = _req_plain(bits, 'bits', torch.int64)
    g = _req_bytes(gt, 'gt')
    if d.dim() != 3 or g.dim() != 3 or d.shape[1] != (int(W) + 63) // 64 or int(g.shape[2]) != int(W) or g.shape[1] != d.shape[2] or d.device != g.device:
        raise ValueError(f'mask_overlap_bits: bits [K, ceil(W / 64), H] and gt [G,H,W] of one size on one device, got {tuple(d.shape)} and {tuple(g.shape)}')
    if g.data_ptr() % 16:
        g = g.clone()
    K, _, H = (int(s) for s in d.shape)
    G, W = int(g.shape[0]), int(W)
    need = mask_overlap_bits_workspace_bytes(K, G, H, W)
    if (G and not need) or (K + G and not mask_overlap_workspace_bytes(K, G, H, W)):
        raise _lib.VknError(-2, f'mask_overlap_bits: {K} x {G} masks of {H} x {W} are outside the envelope of include/vkn_maskap.h')
    if out is None:
        flat = torch.zeros((K * G + K + G + 6,), dtype=torch.int64, device=d.device)        # one fill; each table on a 16-byte boundary
        a, b = (K * G + 1) // 2 * 2, (K * G + 1) // 2 * 2 + (K + 1) // 2 * 2
        out = flat[:K * G].view(K, G), flat[a:a + K], flat[b:b + G]
    inter, area_dt, area_gt = (_req_plain(t, n, torch.int64) for t, n in zip(out, ('inter', 'area_dt', 'area_gt')))
    if tuple(inter.shape) != (K, G) or tuple(area_dt.shape) != (K,) or tuple(area_gt.shape) != (G,) or any(t.device != d.device for t in (inter, area_dt, area_gt)):
        raise ValueError(f'mask_overlap_bits: out = (int64 [{K},{G}], int64 [{K}], int64 [{G}]) on the bits\' device')
    if K + G == 0:
        return inter, area_dt, area_gt
    ws = _workspace(need, d.device, scratch=True)[:need] if need else None
    opt = lambda t: _ptr(t if t is not None and t.numel() else None)          # noqa: E731  (an empty side travels as NULL)
    with torch.cuda.device(d.device):
        check(_lib.lib().vkn_bits_mask_overlap(opt(d), opt(g), K, G, H, W, opt(inter), opt(area_dt), opt(area_gt), opt(ws), need, _stream()))
    return inter, area_dt, area_gt


# ------------------------------------------------------------------------------------------- Swin backbone
_SWIN = _lib.SWIN


def swin_window_attention_supported(B, H, W, heads, window, shift, head_dim=_SWIN['VKN_SWIN_HEAD_DIM']):
    """The envelope of `swin_window_attention` (include/vkn_swin.h), sizes included.  Asks the device nothing."""
    return int(head_dim) == _SWIN['VKN_SWIN_HEAD_DIM'] and bool(
        _lib.lib().vkn_swin_window_attn_supported(int(B), int(H), int(W), int(heads), int(window), int(shift)))


def swin_window_attention(qkv, qkv_bias, bias_table, H, W, heads, window, shift, scale):
    """The (shifted-)window attention of one Swin block (include/vkn_swin.h: vkn_swin_window_attn_f32).  qkv [B, H W, 3 heads 32] (or
    [B, H, W, ...]): the rows of `attn.qkv(norm1(x))` on the tokens as they are; qkv_bias [3 heads 32] or None; bias_table
    [(2 window - 1)^2, heads].  -> [B, H W, heads 32], what `attn.proj` takes.  One launch."""
    qkv, bias_table = _req(qkv, 'qkv'), _req(bias_table, 'bias_table')
    H, W, heads, window, shift = int(H), int(W), int(heads), int(window), int(shift)
    C = heads * _SWIN['VKN_SWIN_HEAD_DIM']
    B, D = (int(qkv.shape[0]) if qkv.dim() else 0), _SWIN['VKN_SWIN_HEAD_DIM']
    if B < 1 or tuple(qkv.shape) not in ((B, H * W, 3 * C), (B, H, W, 3 * C), (B, H * W, 3, heads, D), (B, H, W, 3, heads, D)):
        raise ValueError(f'swin_window_attention: qkv {tuple(qkv.shape)} is neither [B, {H * W}, {3 * C}] nor [B, {H}, {W}, 3, {heads}, {D}]')
    if tuple(bias_table.shape) != ((2 * window - 1) ** 2, heads) or bias_table.device != qkv.device:
        raise ValueError(f'swin_window_attention: bias_table {tuple(bias_table.shape)} is not [{(2 * window - 1) ** 2}, {heads}] on the device of qkv')
    if qkv_bias is not None:
        qkv_bias = _req(qkv_bias, 'qkv_bias')
        if qkv_bias.numel() != 3 * C or qkv_bias.device != qkv.device:
            raise ValueError(f'swin_window_attention: qkv_bias {tuple(qkv_bias.shape)} is not [{3 * C}] on the device of qkv')
    out = torch.empty((B, H * W, C), dtype=torch.float32, device=qkv.device)
    with torch.cuda.device(qkv.device):
        check(_lib.lib().vkn_swin_window_attn_f32(_ptr(qkv), _ptr(qkv_bias), _ptr(bias_table), _ptr(out), B, H, W, heads, window, shift,
                                                  float(scale), _stream()))
    return out


def swin_window_attention_bwd_supported(B, H, W, heads, window, shift, head_dim=_SWIN['VKN_SWIN_HEAD_DIM']):
    """The envelope of `swin_window_attention_bwd` (include/vkn_wattn_train.h): the forward's and a workspace below 2^31 bytes.  Asks the
    device nothing."""
    return int(head_dim) == _SWIN['VKN_SWIN_HEAD_DIM'] and bool(
        _lib.lib().vkn_wattn_bwd_supported(int(B), int(H), int(W), int(heads), int(window), int(shift)))


def swin_window_attention_bwd(qkv, qkv_bias, bias_table, dout, H, W, heads, window, shift, scale):
    """The backward of `swin_window_attention` (include/vkn_wattn_train.h: vkn_wattn_bwd_f32) from its own operands and the gradient
    dout [B, H W, heads 32] of its output -> (dqkv in the shape of qkv, dqkv_bias [3 heads 32] or None, dbias_table in the shape of
    bias_table).  Nothing of the forward is needed: scores and softmax are recomputed.  `dqkv_bias` is ONLY the part of the bias gradient
    that flows through pad tokens (their k and v are the bias); the part through real tokens follows from dqkv in the `qkv` Linear.  No
    float atomics: two calls give the same bits.  Two launches."""
    qkv, bias_table, dout = _req(qkv, 'qkv'), _req(bias_table, 'bias_table'), _req(dout, 'dout')
    H, W, heads, window, shift = int(H), int(W), int(heads), int(window), int(shift)
    D = _SWIN['VKN_SWIN_HEAD_DIM']
    C = heads * D
    B = int(qkv.shape[0]) if qkv.dim() else 0
    if B < 1 or tuple(qkv.shape) not in ((B, H * W, 3 * C), (B, H, W, 3 * C), (B, H * W, 3, heads, D), (B, H, W, 3, heads, D)):
        raise ValueError(f'swin_window_attention_bwd: qkv {tuple(qkv.shape)} is neither [B, {H * W}, {3 * C}] nor [B, {H}, {W}, 3, {heads}, {D}]')
    if tuple(dout.shape) not in ((B, H * W, C), (B, H, W, C)) or dout.device != qkv.device:
        raise ValueError(f'swin_window_attention_bwd: dout {tuple(dout.shape)} is not [{B}, {H * W}, {C}] on the device of qkv')
    if tuple(bias_table.shape) != ((2 * window - 1) ** 2, heads) or bias_table.device != qkv.device:
        raise ValueError(f'swin_window_attention_bwd: bias_table {tuple(bias_table.shape)} is not [{(2 * window - 1) ** 2}, {heads}] on the device of qkv')
    if qkv_bias is not None:
        qkv_bias = _req(qkv_bias, 'qkv_bias')
        if qkv_bias.numel() != 3 * C or qkv_bias.device != qkv.device:
            raise ValueError(f'swin_window_attention_bwd: qkv_bias {tuple(qkv_bias.shape)} is not [{3 * C}] on the device of qkv')
    L_ = _lib.lib()
    nb = L_.vkn_wattn_bwd_workspace_bytes(B, H, W, heads, window)
    if not nb or not L_.vkn_wattn_bwd_supported(B, H, W, heads, window, shift):
        raise ValueError(f'swin_window_attention_bwd: B {B}, map {H} x {W}, {heads} heads, window {window}, shift {shift} is outside the envelope')
    dqkv = torch.empty_like(qkv)
    dqkv_bias = torch.empty_like(qkv_bias) if qkv_bias is not None else None
    dtable = torch.empty_like(bias_table)
    ws = _workspace(nb, qkv.device, scratch=True)
    with torch.cuda.device(qkv.device):
        check(L_.vkn_wattn_bwd_f32(_ptr(qkv), _ptr(qkv_bias), _ptr(bias_table), _ptr(dout), _ptr(dqkv), _ptr(dqkv_bias), _ptr(dtable), B, H, W,
                                   heads, window, shift, float(scale), _ptr(ws), ws.numel(), _stream()))
    return dqkv, dqkv_bias, dtable
