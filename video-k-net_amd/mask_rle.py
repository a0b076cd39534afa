"""`MaskRLE`: COCO run-length encoding of instance masks on the device (include/vkn_rle.h, csrc/vkn_rle.hip).

What the reference's test loops do with the instance masks — `encode_mask_results` (external/test.py:55-70, tools_vis/apis/test.py:36,80,
mmtrack/transform.py:outs2results) over K full-resolution boolean arrays copied to the host — happens here on the device: what crosses to
the host is the per-mask records (36 bytes each) and the strings (a few kilobytes per mask).  The format is the one pycocotools writes,
restated in include/vkn_rle.h; the results are plain integers and bytes, equal to tests/rle_ref.py bit for bit.
"""
import numpy as np
import torch

from . import _lib, ops

_C = _lib.RLE
_REC = _C['VKN_RLE_RECORD_INTS']


class MaskRLE:
    """One encoder per process or per consumer: it owns the workspace and the two pools per device, and grows them when a call reports
    that they were too small (at most one second call).  `cap_runs` / `cap_bytes`: the pools' first sizes.

        rles = enc(masks)                # bool / uint8 [K,H,W] CUDA tensor: nonzero = set
        rles = enc(logits, thr=0.5)      # float32 [K,H,W]: set iff logits > thr (one fp32 comparison, torch's `>`)

    -> [{'size': [H, W], 'counts': bytes}] * K, as pycocotools' `encode` returns them.  `areas()`, `bboxes()` and `counts()` speak of
    the last call; `device_calls` is the number of encode calls it took (1, or 2 after growing)."""

    def __init__(self, cap_runs=1 << 16, cap_bytes=1 << 18):
        self.cap_runs, self.cap_bytes = max(1, int(cap_runs)), max(1, int(cap_bytes))
        self._dev = {}
        self.device_calls = 0
        self._last = None

    def _buffers(self, device):
        b = self._dev.get(device)
        if b is None:
            b = self._dev[device] = dict(runs=torch.empty((self.cap_runs,), dtype=torch.int32, device=device),
                                         pool=torch.empty((self.cap_bytes,), dtype=torch.uint8, device=device),
                                         ws=torch.empty((0,), dtype=torch.uint8, device=device))
        return b

    def __call__(self, masks, thr=None):
        if not torch.is_tensor(masks) or masks.dim() != 3:
            raise ValueError(f'MaskRLE: a tensor of masks [K,H,W], got {tuple(masks.shape) if torch.is_tensor(masks) else type(masks)}')
        K, H, W = (int(s) for s in masks.shape)
        self.device_calls = 0
        if K == 0:                                                                         # nothing to encode: no launch, no library
            self._last = dict(K=0, H=H, W=W, rec=np.zeros((0, _REC), dtype=np.int32), raw=b'', buf=None)
            return []
        if not masks.is_cuda:
            raise _lib.VknLibraryError('MaskRLE: expected a CUDA/HIP tensor — the MI355X path has no CPU fallback')
        need = ops.rle_workspace_bytes(K, H, W)
        if not need or (thr is not None and K * H * W * 4 >= 2 ** 31):
            raise _lib.VknError(-2, f'MaskRLE: {K} masks of {H} x {W} are outside the envelope of include/vkn_rle.h '
                                    f'(1 <= K <= {_C["VKN_RLE_MAX_K"]}, H * W < 2^31, K * H * W * element size < 2^31)')
        return self._encode(K, H, W, masks.device, need, lambda head, b: ops.rle_encode(masks, head[:K * _REC], b['runs'], b['pool'], head[-1:], b['ws'][:need], thr=thr))

    def _encode(self, K, H, W, device, need, call):
        """The encode call (`call(head, buffers)`: head = the records, then the status word) with the one-retry rule: pools that were
        reported full grow to the reported sizes, once."""
        b = self._buffers(device)
        if b['ws'].numel() < need:
            b['ws'] = torch.empty((need,), dtype=torch.uint8, device=device)
        head = torch.empty((K * _REC + 1,), dtype=torch.int32, device=device)              # the records, then the status word
        for _ in range(2):
            head[-1:].zero_()
            call(head, b)
            self.device_calls += 1
            host = head.cpu().numpy()                                                      # one small device -> host copy
            rec, status = host[:-1].reshape(K, _REC), int(host[-1])
            runs_used = int(rec[-1, _C['VKN_RLE_REC_RUN_OFF']]) + int(rec[-1, _C['VKN_RLE_REC_NRUNS']])
            bytes_used = int(rec[-1, _C['VKN_RLE_REC_BYTE_OFF']]) + int(rec[-1, _C['VKN_RLE_REC_NBYTES']])
            if not status & _C['VKN_RLE_STATUS_FULL']:
                break
            if status & _C['VKN_RLE_STATUS_FULL_RUNS']:                                    # the records hold the true sizes: grow to them
                b['runs'] = torch.empty((runs_used,), dtype=torch.int32, device=device)
            if status & _C['VKN_RLE_STATUS_FULL_BYTES']:
                b['pool'] = torch.empty((bytes_used,), dtype=torch.uint8, device=device)
        else:
            raise _lib.VknError(-6, f'MaskRLE: pools of the reported sizes ({runs_used} runs, {bytes_used} bytes) were reported full again')
        raw = b['pool'][:bytes_used].cpu().numpy().tobytes()                               # the used prefix of the byte pool
        self._last = dict(K=K, H=H, W=W, rec=rec.copy(), raw=raw, buf=b, runs_used=runs_used)
        return self.counts()

    def encode_logits(self, logits, img_meta, thr, rows=None, up=1):
        """The RLEs of `rescale_masks(logits[rows]) > thr` without the K full-resolution maps: the masks come as bits straight from the
        logits (`ops.instance_mask_bits`, include/vkn_instmask.h) and are encoded as they are (vkn_bits_rle_encode).  logits float32
        [N,Hm,Wm]: with up = 1 the scaled mask predictions, with up in (2, 4) the head's stride-8 logits; rows: the entries to encode
        (None: every row).  The same accessors and the same one-retry rule as a call.  CPU tensors and geometries outside the kernel's
        envelope take the torch rescale and this encoder's call on its fp32 result."""
        if not torch.is_tensor(logits) or logits.dim() != 3:
            raise ValueError(f'MaskRLE.encode_logits: a tensor of logits [N,Hm,Wm], got {tuple(logits.shape) if torch.is_tensor(logits) else type(logits)}')
        if rows is not None:
            rows = torch.as_tensor(rows, device=logits.device).reshape(-1)
        K = int(logits.shape[0]) if rows is None else int(rows.numel())
        H, W = (int(v) for v in img_meta['ori_shape'][:2])
        if K == 0:
            return self(torch.zeros((0, H, W), dtype=torch.bool, device=logits.device))
        if not ops.instance_bits_fused(logits, img_meta, K, up) or not ops.rle_bits_workspace_bytes(K, H, W):
            sel = logits if rows is None else logits.index_select(0, rows.long())
            return self(ops.rescale_masks_torch(sel.float(), img_meta, up), thr=float(thr))
        self.device_calls = 0
        bits = ops.instance_mask_bits(logits, img_meta, thr, rows=rows, up=up)
        need = ops.rle_bits_workspace_bytes(K, H, W)
        return self._encode(K, H, W, logits.device, need, lambda head, b: ops.rle_encode_bits(bits, W, head[:K * _REC], b['runs'], b['pool'], head[-1:], b['ws'][:need]))

    # ---- the last call
    def _need_last(self):
        if self._last is None:
            raise RuntimeError('MaskRLE: nothing was encoded yet')
        return self._last

    def counts(self, uncompressed=False):
        """[{'size': [H, W], 'counts': bytes}] per mask; uncompressed=True: 'counts' is the list of run lengths instead (one more copy:
        the used prefix of the run pool, valid until the next call)."""
        last = self._need_last()
        rec, size = last['rec'], [last['H'], last['W']]
        if not uncompressed:
            off, n = rec[:, _C['VKN_RLE_REC_BYTE_OFF']], rec[:, _C['VKN_RLE_REC_NBYTES']]
            return [{'size': list(size), 'counts': last['raw'][int(o):int(o) + int(m)]} for o, m in zip(off, n)]
        if last['K'] == 0:
            return []
        if 'runs' not in last:
            last['runs'] = last['buf']['runs'][:last['runs_used']].cpu().numpy().view(np.uint32)
        off, n = rec[:, _C['VKN_RLE_REC_RUN_OFF']], rec[:, _C['VKN_RLE_REC_NRUNS']]
        return [{'size': list(size), 'counts': last['runs'][int(o):int(o) + int(m)].tolist()} for o, m in zip(off, n)]

    def areas(self):
        """int64 [K]: set pixels per mask"""
        return self._need_last()['rec'][:, _C['VKN_RLE_REC_AREA']].astype(np.int64)

    def bboxes(self):
        """int64 [K, 4]: x0, y0, width, height over the set pixels; zeros for an empty mask"""
        a = _C['VKN_RLE_REC_BBOX']
        return self._need_last()['rec'][:, a:a + 4].astype(np.int64)

    def records(self):
        """int32 [K, VKN_RLE_RECORD_INTS] as the device wrote them (include/vkn_rle.h)"""
        return self._need_last()['rec']


_DEFAULT = None


def default_encoder():
    """The process-wide `MaskRLE` behind `encode_mask_results` and the heads' `get_seg_masks_rle`."""
    global _DEFAULT
    if _DEFAULT is None:
        _DEFAULT = MaskRLE()
    return _DEFAULT


def encode_mask_results(mask_results, encoder=None):
    """mmdet's `encode_mask_results` for per-class lists of DEVICE masks (bool / uint8 [H,W] CUDA tensors of one image): the same
    per-class lists of RLE dicts, from ONE device call over all masks of the image.  A tuple (cls_segms, cls_mask_scores) keeps its
    second part, as in mmdet."""
    if isinstance(mask_results, tuple):
        cls_segms, cls_mask_scores = mask_results
    else:
        cls_segms, cls_mask_scores = mask_results, None
    flat = [m for cls in cls_segms for m in cls]
    if any(not torch.is_tensor(m) or not m.is_cuda for m in flat):
        raise _lib.VknLibraryError('encode_mask_results: expected CUDA/HIP masks — the MI355X path has no CPU fallback')
    rles = iter((encoder or default_encoder())(torch.stack([m.to(torch.uint8) for m in flat])) if flat else [])
    encoded = [[next(rles) for _ in cls] for cls in cls_segms]
    return (encoded, cls_mask_scores) if isinstance(mask_results, tuple) else encoded
