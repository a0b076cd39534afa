"""The fused instance-mask rescale of include/vkn_instmask.h against tests/instmask_ref.py: the bits equal the float64 chain's `>` on every
DECIDED pixel (all pixels of a partition case; all but at most instmask_ref.UNDECIDED_CAP of a noise case), the bits behind Wo are zero,
and the two consumers of bits (vkn_bits_rle_encode, vkn_bits_mask_overlap) equal their u8 entries on the unpacked masks, byte for byte.
Outputs are carved at exact size out of an `abi_arena.Arena`, the inputs are frozen, and `Arena.check` follows every call."""
import ctypes

import numpy as np
import pytest
import torch

import instmask_ref as R
import rle_ref
from abi_arena import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
REC = 9


def _bits(vkn, logits, meta, up, thr, rows=None, K=None):
    """one vkn_instance_bits_f32 call through the C ABI, the bits carved at exact size -> (uint64 [K, strips, Ho] on the host, status word)"""
    L = vkn._lib.lib()
    src = logits.to(DEV).contiguous()
    N, Hm, Wm = src.shape
    r = torch.as_tensor(np.asarray(rows), dtype=torch.int32).to(DEV) if rows is not None else None
    K = int(r.numel()) if r is not None else (K or N)
    cfg = vkn.ops.instance_mask_cfg(Hm, Wm, meta, up)
    Ho, Wo = meta['ori_shape'][:2]
    nbytes = L.vkn_instance_bits_workspace_bytes(ctypes.byref(cfg), K)
    assert nbytes == vkn._lib.INSTMASK['VKN_INSTMASK_WS_BYTES']
    A = Arena(DEV)
    out, ws = A.out((K, R.strips_of(Wo), Ho), torch.int64, 'bits'), A.out((4,), torch.int32, 'status')
    with frozen(src, r), torch.cuda.device(DEV):
        rc = L.vkn_instance_bits_f32(ctypes.byref(cfg), ctypes.c_void_p(src.data_ptr()), N, ctypes.c_void_p(r.data_ptr() if r is not None else None), K,
                                     ctypes.c_float(thr), out.ptr, ws.ptr, nbytes, vkn.ops._stream())
    assert rc == 0
    A.check(f'vkn_instance_bits_f32 {tuple(src.shape)} up {up} -> {Ho} x {Wo}')
    return out.t.cpu().numpy().view(np.uint64), int(ws.t.cpu()[0])


def _compare(bits, mask, decided, Wo, cap):
    got, tail = R.unpack_bits(bits, Wo)
    assert not tail, 'a bit behind Wo is set'
    assert got.shape == mask.shape
    left_out = 1.0 - decided.mean()
    wrong = (got != mask) & decided
    print(f'decided pixels that differ: {int(wrong.sum())} of {mask.size}; left out: {left_out:.2e} (cap {cap:.0e})')
    assert left_out <= cap
    assert not wrong.any(), np.argwhere(wrong)[:5]
    return got


@pytest.mark.parametrize('kind,name,thr', R.CASES, ids=[f'{k}-{n}-{t}' for k, n, t in R.CASES])
def test_bits_equal_the_reference_on_every_decided_pixel(vkn, kind, name, thr):
    c = R.get(kind, name, thr)
    bits, status = _bits(vkn, c['logits'], c['meta'], c['up'], thr)
    assert status == 0
    _compare(bits, c['mask'], c['decided'], c['geom'][5][1], 0.0 if kind == 'partition' else R.UNDECIDED_CAP)


def test_one_mask(vkn):
    c = R.partition('crop_down')
    bits, _ = _bits(vkn, c['logits'][2:3], c['meta'], c['up'], 0.5)
    _compare(bits, c['mask'][2:3], c['decided'][2:3], 65, 0.0)


@pytest.mark.parametrize('arm', ['none', 'permuted', 'duplicates', 'first_k'])
def test_a_hundred_rows_in_any_order(vkn, arm):
    c = R.rows_case(100)
    rng = np.random.default_rng(7)
    rows = {'none': None, 'permuted': rng.permutation(100), 'duplicates': rng.integers(0, 100, 100), 'first_k': None}[arm]
    K = 37 if arm == 'first_k' else None               # rows NULL, K < N: the first K rows
    bits, status = _bits(vkn, c['logits'], c['meta'], c['up'], 0.5, rows, K)
    idx = np.arange(K or 100) if rows is None else rows
    assert status == 0
    _compare(bits, c['mask'][idx], c['decided'][idx], 80, 0.0)


def test_row_out_of_range_is_reported_and_empty(vkn):
    c = R.partition('base')
    bits, status = _bits(vkn, c['logits'], c['meta'], c['up'], 0.5, rows=[1, 5, -1, 0])
    assert status == vkn._lib.INSTMASK['VKN_INSTMASK_STATUS_ROW_RANGE']
    got, tail = R.unpack_bits(bits, 80)
    assert not tail and not got[1].any() and not got[2].any() and np.array_equal(got[[0, 3]], c['mask'][[1, 0]])


def test_nonfinite_logits_follow_the_reference(vkn):
    """sigmoid(+inf) = 1, sigmoid(-inf) = 0, and a pixel that taps a NaN is NaN: the reference's `>` gives 0 there"""
    c = R.nonfinite_case()
    bits, status = _bits(vkn, c['logits'], c['meta'], c['up'], 0.5)
    got = _compare(bits, c['mask'], c['decided'], c['geom'][5][1], R.UNDECIDED_CAP)
    assert status == 0 and not got[np.isnan(c['p64'])].any()


def test_threshold_is_torchs_greater_than(vkn):
    """identity geometry, logits 0: p is exactly 0.5 at every pixel.  thr = 0.5: equal gives 0; the fp32 value below 0.5: set"""
    meta = R.meta_of(R.GEOMS['identity'])
    lg = torch.zeros((2, 16, 16))
    assert not R.unpack_bits(_bits(vkn, lg, meta, 1, 0.5)[0], 16)[0].any()
    assert R.unpack_bits(_bits(vkn, lg, meta, 1, float(np.nextafter(np.float32(0.5), np.float32(0))))[0], 16)[0].all()


def test_twice_and_under_graph_capture_the_same_bits(vkn):
    c = R.noise('vipseg', 0.5)
    lg = c['logits'].to(DEV)
    a = vkn.ops.instance_mask_bits(lg, c['meta'], 0.5, up=c['up'])
    b = vkn.ops.instance_mask_bits(lg, c['meta'], 0.5, up=c['up'])
    assert a.dtype == torch.int64 and tuple(a.shape) == (5, 5, 180) and torch.equal(a, b)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        vkn.ops.instance_mask_bits(lg, c['meta'], 0.5, up=c['up'])      # (the stream's scratch buffer exists before the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = vkn.ops.instance_mask_bits(lg, c['meta'], 0.5, up=c['up'])
    cap.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, a)


# ---- the consumers of bits
def _rle_call(vkn, entry, src, K, H, W, cap_runs, cap_bytes):
    L = vkn._lib.lib()
    nbytes = (L.vkn_bits_rle_workspace_bytes if entry == 'bits' else L.vkn_rle_workspace_bytes)(K, H, W)
    assert nbytes > 0
    A = Arena(DEV)
    rec, runs = A.out((K, REC), torch.int32, 'records'), A.out((cap_runs,), torch.int32, 'runs', full=False)
    pool, status, ws = A.out((cap_bytes,), torch.uint8, 'bytes', full=False), A.out((1,), torch.int32, 'status'), A.ws(nbytes, 'ws')
    A._materialise()
    runs.t.zero_(), pool.t.zero_(), status.t.zero_()
    fn = L.vkn_bits_rle_encode if entry == 'bits' else L.vkn_rle_encode_u8
    with frozen(src), torch.cuda.device(DEV):
        rc = fn(ctypes.c_void_p(src.data_ptr()), K, H, W, rec.ptr, runs.ptr, cap_runs, pool.ptr, cap_bytes, status.ptr, ws.ptr, nbytes, vkn.ops._stream())
    assert rc == 0
    A.check(f'vkn_rle_encode_{entry} {K} x {H} x {W}')
    return rec.t.cpu().numpy(), runs.t.cpu().numpy(), pool.t.cpu().numpy(), int(status.t.cpu()[0])


@pytest.mark.parametrize('name', ['crop_down', 'strip_128', 'strong_down'])
@pytest.mark.parametrize('pools', ['fit', 'full'])
def test_rle_on_bits_equals_rle_on_bytes(vkn, name, pools):
    """byte for byte: records, run pool, byte pool, status — with pools that fit exactly and with pools that are FULL"""
    c = R.noise(name, 0.5)
    mask = c['mask']
    K, H, W = mask.shape
    nruns = sum(len(rle_ref.counts(m)) for m in mask)
    nbytes = sum(len(rle_ref.to_string(rle_ref.counts(m))) for m in mask)
    caps = (nruns, nbytes) if pools == 'fit' else (nruns // 2, nbytes // 3)
    u8 = torch.from_numpy(mask.astype(np.uint8)).to(DEV)
    bits = torch.from_numpy(R.pack_bits(mask).view(np.int64)).to(DEV)
    a = _rle_call(vkn, 'u8', u8, K, H, W, *caps)
    b = _rle_call(vkn, 'bits', bits, K, H, W, *caps)
    assert a[3] == b[3] == (0 if pools == 'fit' else 3)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)


@pytest.mark.parametrize('name', list(R.GEOMS))
def test_rle_of_the_device_bits_equals_the_reference_encoder(vkn, name):
    c = R.partition(name)
    enc = vkn.MaskRLE(cap_runs=8, cap_bytes=8)                  # too small: the one-retry rule
    got = enc.encode_logits(c['logits'].to(DEV), c['meta'], 0.5, up=c['up'])
    assert enc.device_calls == 2
    want = [rle_ref.encode(m) for m in c['mask']]
    assert [g['counts'] for g in got] == [w['counts'] for w in want] and all(g['size'] == list(c['mask'].shape[1:]) for g in got)
    assert enc.areas().tolist() == [int(m.sum()) for m in c['mask']]


@pytest.mark.parametrize('G', [0, 3, 70])
def test_overlap_on_bits_equals_overlap_on_bytes(vkn, G):
    c = R.noise('vipseg', 0.3)
    mask = c['mask']
    K, H, W = mask.shape
    rng = np.random.default_rng(G)
    gt = torch.from_numpy((rng.random((G, H, W)) < 0.4).astype(np.uint8)).to(DEV)
    a = vkn.ops.mask_overlap(torch.from_numpy(mask.astype(np.uint8)).to(DEV), gt)
    b = vkn.ops.mask_overlap_bits(torch.from_numpy(R.pack_bits(mask).view(np.int64)).to(DEV), W, gt)
    for x, y in zip(a, b):
        assert torch.equal(x, y)
    assert b[1].tolist() == [int(m.sum()) for m in mask]


def test_overlap_on_bits_exact_workspace(vkn):
    c = R.partition('crop_down')
    mask = c['mask']
    K, H, W = mask.shape
    G = 4
    L = vkn._lib.lib()
    gt = torch.from_numpy(np.ascontiguousarray(mask[[0, 1, 1, 3]]).astype(np.uint8)).to(DEV)
    bits = torch.from_numpy(R.pack_bits(mask).view(np.int64)).to(DEV)
    nbytes = L.vkn_bits_mask_overlap_workspace_bytes(K, G, H, W)
    assert nbytes == (8 * G * R.strips_of(W) * H + 15) // 16 * 16
    A = Arena(DEV)
    inter, ad, ag, ws = A.out((K, G), torch.int64, 'inter'), A.out((K,), torch.int64, 'area_dt'), A.out((G,), torch.int64, 'area_gt'), A.ws(nbytes, 'ws')
    A._materialise()
    inter.t.zero_(), ad.t.zero_(), ag.t.zero_()
    with frozen(bits, gt), torch.cuda.device(DEV):
        rc = L.vkn_bits_mask_overlap(ctypes.c_void_p(bits.data_ptr()), ctypes.c_void_p(gt.data_ptr()), K, G, H, W, inter.ptr, ad.ptr, ag.ptr, ws.ptr,
                                     nbytes, vkn.ops._stream())
    assert rc == 0
    torch.cuda.synchronize()
    assert not [p for p in A.problems() if 'stray' in p]
    m = mask.reshape(K, -1).astype(np.int64)
    g = gt.cpu().numpy().reshape(G, -1).astype(np.int64)
    assert np.array_equal(inter.t.cpu().numpy(), m @ g.T) and ad.t.cpu().tolist() == m.sum(1).tolist() and ag.t.cpu().tolist() == g.sum(1).tolist()


def test_meter_from_logits_equals_meter_from_masks(vkn):
    c = R.partition('vipseg')
    mask = torch.from_numpy(c['mask']).to(DEV)
    K = mask.shape[0]
    scores = torch.linspace(0.9, 0.3, K, device=DEV)
    labels = torch.tensor([0, 1, 0, 1, 2], device=DEV)
    gt = torch.roll(mask, shifts=(3, 5), dims=(1, 2))[:4].contiguous()
    gl = torch.tensor([0, 1, 0, 2], device=DEV)
    a, b = vkn.MaskAPMeter(3, capacity=64), vkn.MaskAPMeter(3, capacity=64)
    ta = a.update(0, mask, scores, labels, gt, gl)
    tb = b.update_logits(0, c['logits'].to(DEV), c['meta'], 0.5, scores, labels, gt, gl, up=c['up'])
    for x, y in zip(ta, tb):
        assert torch.equal(x, y)
    ha, hb = a._host(), b._host()
    assert ha['count'] == hb['count'] == K and np.array_equal(ha['rec'], hb['rec']) and np.array_equal(ha['npig'], hb['npig'])


@pytest.mark.parametrize('video', [False, True])
def test_heads_fused_results_equal_the_default_path(vkn, video):
    """`get_seg_masks_rle_fused` and `get_seg_masks_tracking_rle` on a partition case (every pixel decided): the dicts of
    the default path, bit for bit"""
    c = R.partition('strong_down')                 # up = 1: the heads hand on the scaled mask predictions
    head = (vkn.KernelUpdateHeadVideo if video else vkn.KernelUpdateHead).__new__(vkn.KernelUpdateHeadVideo if video else vkn.KernelUpdateHead)
    head.num_classes = 3
    lg = c['logits'].to(DEV)
    labels, scores = torch.tensor([0, 2, 1, 0, 2], device=DEV), torch.linspace(0.9, 0.5, 5, device=DEV)
    ids = torch.tensor([4, -1, 0, 7, -1], device=DEV)
    cfg = dict(mask_thr=0.5)
    d = head.get_seg_masks_rle(lg, labels, scores, cfg, c['meta'])
    f = head.get_seg_masks_rle_fused(lg, labels, scores, cfg, c['meta'])
    assert d[1] == f[1] and all(np.array_equal(x, y) for x, y in zip(d[0], f[0]))
    want = [rle_ref.encode(m) for m in c['mask']]
    assert f[1] == [[want[0], want[3]], [want[2]], [want[1], want[4]]]
    d = head.get_seg_masks_tracking_rle(lg, labels, scores, ids, cfg, c['meta'])
    f = head.get_seg_masks_tracking_rle(lg, labels, scores, ids, cfg, c['meta'], fused_rescale=True)
    assert d[1] == f[1] == [[want[0], want[3]], [want[2]], []] and all(np.array_equal(x, y) for x, y in zip(d[0], f[0]))
    assert [r[:, 0].tolist() for r in f[0]] == [[4.0, 7.0], [0.0], []]
