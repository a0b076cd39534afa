"""The device encoder of include/vkn_rle.h against tests/rle_ref.py, bit for bit: counts, strings, offsets, area and bbox of every mask.
There is no float in the results, so every comparison is exact.  Outputs and the workspace are carved at exact size out of an
`abi_arena.Arena`, the inputs are frozen, and `Arena.check` follows every call: every output word written, nothing else touched.
S = VKN_RLE_STRIP_COLS is the strip of columns a workgroup owns; the shapes sit on its edges."""
import ctypes
import inspect

import numpy as np
import pytest
import torch

import rle_ref as R
from abi_arena import Arena, frozen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
S = 64
REC = 9
FULL_RUNS, FULL_BYTES = 1, 2


def _expect(masks):
    """per mask of bool [K,H,W]: counts, string; and the records the device must write"""
    cnts = [R.counts(m) for m in masks]
    strs = [R.to_string(c) for c in cnts]
    rec = np.zeros((len(cnts), REC), dtype=np.int64)
    ro = bo = 0
    for k, (m, c, s) in enumerate(zip(masks, cnts, strs)):
        rec[k] = [len(c), ro, len(s), bo, R.area(m), *R.bbox(m)]
        ro, bo = ro + len(c), bo + len(s)
    return cnts, strs, rec, ro, bo


def _call(vkn, src, thr, cap_runs, cap_bytes):
    """one call at exactly these capacities -> (records, runs, bytes, status) on the host"""
    L = vkn._lib.lib()
    K, H, W = src.shape
    assert vkn._lib.RLE['VKN_RLE_STRIP_COLS'] == S and vkn._lib.RLE['VKN_RLE_RECORD_INTS'] == REC and cap_runs >= 1 and cap_bytes >= 1
    nbytes = L.vkn_rle_workspace_bytes(K, H, W)
    assert nbytes > 0
    A = Arena(DEV)
    rec, runs = A.out((K, REC), torch.int32, 'records'), A.out((cap_runs,), torch.int32, 'runs')
    pool, status, ws = A.out((cap_bytes,), torch.uint8, 'bytes'), A.out((1,), torch.int32, 'status'), A.ws(nbytes, 'ws')
    status.t.zero_()
    tail = (K, H, W, rec.ptr, runs.ptr, cap_runs, pool.ptr, cap_bytes, status.ptr, ws.ptr, nbytes, vkn.ops._stream())
    with frozen(src), torch.cuda.device(DEV):
        if thr is None:
            rc = L.vkn_rle_encode_u8(ctypes.c_void_p(src.data_ptr()), *tail)
        else:
            rc = L.vkn_rle_encode_f32(ctypes.c_void_p(src.data_ptr()), ctypes.c_float(thr), *tail)
    assert rc == 0
    A.check(f'vkn_rle_encode {tuple(src.shape)} caps {cap_runs}, {cap_bytes}')
    return rec.t.cpu().numpy().astype(np.int64), runs.t.cpu().numpy().view(np.uint32), pool.t.cpu().numpy().tobytes(), int(status.t.cpu()[0])


def _check(vkn, masks, src=None, thr=None):
    """masks: bool numpy [K,H,W], what `src` (default: the masks as uint8) means; encodes at exactly the needed capacities"""
    masks = np.asarray(masks, dtype=bool)
    cnts, strs, want, nruns, nbytes = _expect(masks)
    if src is None:
        src = torch.from_numpy(masks.astype(np.uint8)).to(DEV)
    assert tuple(src.shape) == masks.shape and src.data_ptr() % 16 == 0
    rec, runs, pool, status = _call(vkn, src, thr, nruns, nbytes)
    assert status == 0
    assert np.array_equal(rec, want), (rec[:4], want[:4])
    for k, (c, s) in enumerate(zip(cnts, strs)):
        assert runs[want[k, 1]:want[k, 1] + want[k, 0]].tolist() == c, k
        assert pool[want[k, 3]:want[k, 3] + want[k, 2]] == s, k
    assert runs.size == nruns and len(pool) == nbytes
    return rec, runs, pool


def _rand(rng, K, H, W, p=0.5):
    return rng.random((K, H, W)) < p


def _blobs(rng, K, H, W, r=3):
    n = rng.random((K, H, W))
    acc = np.zeros_like(n)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            acc += np.roll(np.roll(n, dy, axis=1), dx, axis=2)
    return acc / (2 * r + 1) ** 2 > 0.5


@pytest.mark.parametrize('arm', ['u8', 'f32'])
def test_degenerate_shapes_and_uniform_masks(vkn, arm):
    rng = np.random.default_rng(1)
    cases = [np.zeros((1, 1, 1), bool), np.ones((1, 1, 1), bool), _rand(rng, 1, 1, 2 * S + 3), _rand(rng, 1, 4099, 1, 0.3),
             np.zeros((1, 37, S + 1), bool), np.ones((1, 37, S + 1), bool), np.ones((2, 3, 2 * S), bool)]
    for m in cases:
        if arm == 'u8':
            _check(vkn, m)
        else:
            _check(vkn, m, torch.from_numpy(np.where(m, 0.75, 0.25).astype(np.float32)).to(DEV), thr=0.5)


@pytest.mark.parametrize('arm', ['u8', 'f32'])
@pytest.mark.parametrize('W', [S - 1, S, S + 1, S + 2, 2 * S + 3])
def test_strip_and_alignment_edges(vkn, arm, W):
    """H = 37 and three masks: with W % 4 in {1, 2, 3} (S + 1, S + 2, S - 1 / 2 S + 3) rows and masks start at every byte alignment"""
    rng = np.random.default_rng(100 + W)
    m = np.concatenate([_rand(rng, 1, 37, W, 0.5), _blobs(rng, 1, 37, W), _rand(rng, 1, 37, W, 0.05)])
    if arm == 'u8':
        src = torch.from_numpy(np.where(m, rng.integers(1, 256, m.shape), 0).astype(np.uint8)).to(DEV)      # nonzero means set
        _check(vkn, m, src)
    else:
        _check(vkn, m, torch.from_numpy(np.where(m, 1.0 + rng.random(m.shape), -rng.random(m.shape)).astype(np.float32)).to(DEV), thr=0.5)


def test_column_seams(vkn):
    """the last pixel of a column against the first of the next, at a strip seam (columns S - 1 | S) and inside a strip (10 | 11): both
    set (no transition), set then clear, clear then set"""
    H, W = 9, S + 3
    masks = []
    for last, first in ((1, 1), (1, 0), (0, 1)):
        for extra in (False, True):
            m = np.zeros((H, W), bool)
            for x in (S - 1, 10):
                m[H - 1, x], m[0, x + 1] = last, first
            if extra:                                       # the same seams inside longer runs
                m[H - 3:, S - 1] |= bool(last)
                m[:2, 11] |= bool(first)
                m[4, :] = True
            masks.append(m)
    m = np.stack(masks)
    rec, _, _ = _check(vkn, m)
    assert rec[0, 0] == 1 + 4 and rec[2, 0] == 1 + 4 and rec[4, 0] == 1 + 4        # two pixels in one run; one pixel; one pixel: two runs of ones each
    assert R.counts(m[0])[1] == 2 and R.counts(m[2])[1] == 1


def test_checkerboard_every_pixel_is_a_transition(vkn):
    y, x = np.mgrid[0:64, 0:67]
    m = np.stack([(x + y) % 2 == 0, (x + y) % 2 == 1])
    rec, _, _ = _check(vkn, m)
    # H is even: a column's last pixel and the next column's first have the same value, so 63 pixels per column change the value
    assert rec[0, 0] == 1 + 1 + 63 * 67 and rec[1, 0] == 1 + 63 * 67 and rec[1, 1] == rec[0, 0]


def test_one_column_hits_every_delta_edge(vkn):
    cnts, hits = R.delta_edge_counts()
    m = R.decode(cnts, sum(cnts), 1)[None]
    rec, runs, pool = _check(vkn, m)
    assert runs.tolist() == cnts and R.from_string(pool) == cnts
    for i, d, n in hits:
        assert len(R.to_string(cnts[:i + 1])) - len(R.to_string(cnts[:i])) == n and cnts[i] - cnts[i - 2] == d


def test_full_hd_single_pixels_take_five_byte_counts(vkn):
    m = np.zeros((2, 1, 1080, 1920), bool)
    m[:, 0, 1079, 1919] = True
    m[1, 0, 0, 0] = True
    for k in range(2):
        rec, runs, pool = _check(vkn, m[k])
        assert runs.tolist() == ([1080 * 1920 - 1, 1] if k == 0 else [0, 1, 1080 * 1920 - 2, 1])
        assert len(R.to_string([1080 * 1920 - 2])) == 5 and len(pool) == (6 if k == 0 else 8)
        assert rec[0, 4:].tolist() == ([1, 1919, 1079, 1, 1] if k == 0 else [2, 0, 0, 1920, 1080])


def _five(rng):
    H, W = 41, 2 * S + 9
    m = np.zeros((5, H, W), bool)
    m[0] = _rand(rng, 1, H, W, 0.5)[0]                     # thousands of runs
    m[1, 7:30, 60:70] = True                               # ten columns of one run, over a strip seam
    m[3] = _blobs(rng, 1, H, W)[0]                         # (mask 2 stays empty)
    m[4, H - 1, W - 1] = True
    return m


def test_five_masks_with_an_empty_one_pin_the_offsets(vkn):
    m = _five(np.random.default_rng(5))
    rec, _, _ = _check(vkn, m)
    assert rec[2].tolist()[:1] == [1] and rec[2, 4:].tolist() == [0, 0, 0, 0, 0] and rec[0, 0] > 1000 and rec[1, 0] == 21 and rec[4, 0] == 2
    assert rec[3, 1] == rec[2, 1] + 1 and rec[3, 3] == rec[2, 3] + rec[2, 2]


def test_random_blobs(vkn):
    m = _blobs(np.random.default_rng(7), 7, 45, 80)
    assert 0.2 < m.mean() < 0.8
    _check(vkn, m)


def test_capacities_exact_and_one_short(vkn):
    m = _five(np.random.default_rng(5))
    cnts, strs, want, nruns, nbytes = _expect(m)
    src = torch.from_numpy(m.astype(np.uint8)).to(DEV)
    all_runs, all_bytes = np.concatenate(cnts), b''.join(strs)
    for cap_runs, cap_bytes, bits in ((nruns, nbytes, 0), (nruns - 1, nbytes, FULL_RUNS), (nruns, nbytes - 1, FULL_BYTES), (nruns - 1, nbytes - 1, 3),
                                      (7, 5, 3)):
        # (`_call` checks the guards behind both pools and that every word below the capacity was written)
        rec, runs, pool, status = _call(vkn, src, None, cap_runs, cap_bytes)
        assert status == bits and np.array_equal(rec, want)                      # the records: the TRUE sizes, whatever the capacity
        n, b = min(cap_runs, nruns), min(cap_bytes, nbytes)
        assert np.array_equal(runs[:n], all_runs[:n]) and pool[:b] == all_bytes[:b]


def test_mask_rle_grows_tiny_pools_with_one_retry(vkn):
    m = _five(np.random.default_rng(5))
    cnts, strs, want, _, _ = _expect(m)
    src = torch.from_numpy(m).to(DEV)                                              # bool
    enc = vkn.MaskRLE(cap_runs=4, cap_bytes=4)
    for calls in (2, 1):                                                           # the second time the pools fit
        out = enc(src)
        assert enc.device_calls == calls
        assert out == [{'size': [41, 2 * S + 9], 'counts': s} for s in strs] == [R.encode(x) for x in m]
        assert [d['counts'] for d in enc.counts(uncompressed=True)] == cnts
        assert enc.areas().tolist() == want[:, 4].tolist() and enc.bboxes().tolist() == want[:, 5:].tolist()
    assert enc(src[:0]) == [] and enc.device_calls == 0
    # mmdet's encode_mask_results over per-class lists of device masks: the class structure is kept, one device call
    per_class = [[src[3]], [], [src[0], src[2]], [src[4].to(torch.uint8)]]
    got = vkn.encode_mask_results(per_class, encoder=enc)
    assert got == [[R.encode(m[3])], [], [R.encode(m[0]), R.encode(m[2])], [R.encode(m[4])]] and enc.device_calls == 1
    assert vkn.encode_mask_results((per_class, 'scores'), encoder=enc) == (got, 'scores')
    assert vkn.encode_mask_results([[], []]) == [[], []]


def test_f32_arm_at_the_threshold(vkn):
    """a pixel is set iff v > thr in fp32: equal is 0, the next float above is 1, NaN is 0, +inf is 1, -inf is 0; the result equals the
    u8 arm's on `logits > thr`"""
    rng = np.random.default_rng(9)
    thr = np.float32(0.3)
    pool = np.array([thr, np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(-1)), np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0], dtype=np.float32)
    v = pool[rng.integers(0, pool.size, (3, 23, S + 5))]
    logits = torch.from_numpy(v).to(DEV)
    bits = logits > float(thr)
    want = v > thr
    assert np.array_equal(bits.cpu().numpy(), want) and want[v == thr].sum() == 0 and want[np.isnan(v)].sum() == 0 and want[v == np.inf].all()
    a = _check(vkn, want, logits, thr=float(thr))
    b = _check(vkn, want, bits.to(torch.uint8))
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]
    # thr itself is rounded to fp32 once, as torch's comparison does
    _check(vkn, v > np.float32(0.1), logits, thr=0.1)
    zero = torch.from_numpy(np.where(rng.random((1, 5, 7)) < 0.5, 0.0, -0.0).astype(np.float32)).to(DEV)
    _check(vkn, np.zeros((1, 5, 7), bool), zero, thr=0.0)


def test_two_calls_give_the_same_bytes(vkn):
    m = _blobs(np.random.default_rng(11), 4, 50, 3 * S + 1)
    a, b = _check(vkn, m), _check(vkn, m)
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2]


def test_one_capture_replayed_on_two_inputs_equals_eager(vkn):
    rng = np.random.default_rng(13)
    K, H, W = 3, 33, S + 7
    inputs = [_blobs(rng, K, H, W), _rand(rng, K, H, W, 0.4)]
    nb = vkn.ops.rle_workspace_bytes(K, H, W)
    src = torch.zeros((K, H, W), dtype=torch.uint8, device=DEV)
    rec, status = torch.zeros((K, REC), dtype=torch.int32, device=DEV), torch.zeros((1,), dtype=torch.int32, device=DEV)
    runs, pool = torch.zeros((K * H * W + K,), dtype=torch.int32, device=DEV), torch.zeros((2 * K * H * W,), dtype=torch.uint8, device=DEV)
    ws = torch.empty((nb,), dtype=torch.uint8, device=DEV)
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        vkn.ops.rle_encode(src, rec, runs, pool, status, ws)                        # warm-up: the code object is loaded before the capture
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        vkn.ops.rle_encode(src, rec, runs, pool, status, ws)
    for m in inputs + inputs[:1]:
        cnts, strs, want, nruns, nbytes = _expect(m)
        src.copy_(torch.from_numpy(m.astype(np.uint8)))
        for t in (rec, runs, pool):
            t.fill_(0x55)
        graph.replay()
        torch.cuda.synchronize()
        eager = _check(vkn, m)
        assert int(status[0]) == 0 and np.array_equal(rec.cpu().numpy(), eager[0]) and np.array_equal(rec.cpu().numpy(), want)
        assert np.array_equal(runs[:nruns].cpu().numpy().view(np.uint32), eager[1]) and pool[:nbytes].cpu().numpy().tobytes() == eager[2] == b''.join(strs)


@pytest.mark.parametrize('typ', ['KernelUpdateHead', 'KernelUpdateHeadVideo'])
def test_get_seg_masks_rle_equals_the_reference_on_get_seg_masks(vkn, typ):
    """the new head method against `rle_ref` applied to the boolean masks `get_seg_masks` returns for the same arguments"""
    extra = dict(num_proposals=5, query_merge_method='mean') if typ.endswith('Video') else {}
    head = vkn.build_head(vkn.configs.mask_head_cfg(False, C=32, heads=8, ffn=64, ncls=4, n_thing=4, n_stuff=0, up=1, head_type=typ, loss_rank=None,
                                                    **extra)).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    K = 5
    low = (torch.randn((K, 12, 20), generator=g) * 3).to(DEV)
    low[2] = -5.0                                                                   # an empty mask
    labels, scores = torch.tensor([2, 0, 2, 3, 0], device=DEV), torch.rand((K,), generator=g).to(DEV)
    meta = dict(img_shape=(45, 77, 3), batch_input_shape=(48, 80), ori_shape=(71, 123, 3))
    test_cfg = dict(mask_thr=0.5, max_per_img=K)
    with frozen(low, labels, scores):
        bbox_ref, segm_ref = head.get_seg_masks(low, labels, scores, test_cfg, meta)
        bbox, segm = head.get_seg_masks_rle(low, labels, scores, test_cfg, meta)
    assert len(segm) == len(segm_ref) == 4 and [len(c) for c in segm] == [2, 0, 2, 1]
    assert all(m.shape == (71, 123) and m.dtype == bool for c in segm_ref for m in c)
    assert segm == [[R.encode(m) for m in c] for c in segm_ref]
    assert all(np.array_equal(a, b) for a, b in zip(bbox, bbox_ref))
    assert any(R.area(m) == 0 for c in segm_ref for m in c) and any(0 < R.area(m) < 71 * 123 for c in segm_ref for m in c)
    assert list(inspect.signature(head.get_seg_masks_rle).parameters) == list(inspect.signature(head.get_seg_masks).parameters)
