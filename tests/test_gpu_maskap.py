"""The device mask-AP meter of include/vkn_maskap.h against tests/maskap_ref.py, at zero tolerance: the overlap tables are integers, the
records are bit words, and precision / recall / stats are float64 arrays produced by the same stated operations.  Tables, states and
workspaces of the raw calls are carved at exact size out of an `abi_arena.Arena`, the inputs are frozen, and `Arena.check` follows every
call.  RUN, DT, GT, GC are the overlap kernel's row run, detection tile, register tile and LDS chunk: the shapes sit on their edges."""
import ctypes

import numpy as np
import pytest
import torch

import maskap_ref as R
from abi_arena import Arena, frozen
from mask_ap_cases import img, match_cases

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
RUN, DT, GT, GC = 32, 64, 8, 64
REC = 12
FULL, LABEL_RANGE, SCORE_NAN = 1, 2, 4
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def _rand(rng, K, H, W, p=0.5):
    return rng.random((K, H, W)) < p


def _overlap(vkn, masks_dt, masks_gt, src=None, thr=None):
    """masks: bool numpy [K,H,W] / [G,H,W]; src: the device tensor that means masks_dt (default: as uint8).  One call through the C ABI in
    an arena -> the three tables on the host, compared with the restatement"""
    L = vkn._lib.lib()
    masks_dt, masks_gt = np.asarray(masks_dt, dtype=bool), np.asarray(masks_gt, dtype=bool)
    K, G, (H, W) = masks_dt.shape[0], masks_gt.shape[0], masks_dt.shape[1:]
    assert masks_gt.shape[1:] == (H, W)
    if src is None:
        src = torch.from_numpy(masks_dt.astype(np.uint8)).to(DEV)
    gt = torch.from_numpy(masks_gt.astype(np.uint8)).to(DEV)
    nbytes = L.vkn_mask_overlap_workspace_bytes(K, G, H, W)
    assert nbytes == 16 * ((K * ((W + 63) // 64) * H + 1) // 2) + 16 * ((G * ((W + 63) // 64) * H + 1) // 2)
    A = Arena(DEV)
    inter, adt, agt, ws = A.out((K, G), torch.int64, 'inter'), A.out((K,), torch.int64, 'area_dt'), A.out((G,), torch.int64, 'area_gt'), A.ws(nbytes, 'ws')
    for r in (inter, adt, agt):
        if r.nbytes:
            r.t.zero_()                                                    # the call ADDS: the caller zeroes
    tail = (ctypes.c_void_p(gt.data_ptr() if G else None), K, G, H, W, inter.ptr, adt.ptr, agt.ptr, ws.ptr, nbytes, vkn.ops._stream())
    with frozen(src if K else None, gt if G else None), torch.cuda.device(DEV):
        if thr is None:
            rc = L.vkn_mask_overlap_u8(ctypes.c_void_p(src.data_ptr() if K else None), *tail)
        else:
            rc = L.vkn_mask_overlap_f32(ctypes.c_void_p(src.data_ptr() if K else None), ctypes.c_float(thr), *tail)
    assert rc == 0
    A.check(f'vkn_mask_overlap {K} x {G} of {H} x {W}')
    got = tuple(r.t.cpu().numpy() if r.nbytes else np.zeros(r.shape, np.int64) for r in (inter, adt, agt))
    want = R.overlaps(masks_dt, masks_gt)
    for g, w, name in zip(got, want, ('inter', 'area_dt', 'area_gt')):
        assert np.array_equal(g, w), (name, (K, G, H, W), g.reshape(-1)[:8], w.reshape(-1)[:8])
    return got


def _as_f32(rng, m):
    return torch.from_numpy(np.where(m, 0.5 + rng.random(m.shape) + 1e-3, 0.5 - rng.random(m.shape)).astype(np.float32)).to(DEV)


@pytest.mark.parametrize('arm', ['u8', 'f32'])
def test_overlap_shapes_on_every_edge(vkn, arm):
    rng = np.random.default_rng(1)
    shapes = [(1, 1, 1, 1)] + [(3, 2, 5, W) for W in (63, 64, 65, 66, 131)] + [(3, 2, H, 70) for H in (RUN - 1, RUN, RUN + 1, 2 * RUN + 3)]
    shapes += [(K, 3, 5, 9) for K in (DT - 1, DT, DT + 1, 2 * DT + 1)] + [(3, G, 5, 9) for G in (GT - 1, GT, GT + 1, GC - 1, GC, GC + 1)]
    for K, G, H, W in shapes:
        dt, gt = _rand(rng, K, H, W), _rand(rng, G, H, W, 0.4)
        if arm == 'u8':
            _overlap(vkn, dt, gt, torch.from_numpy(np.where(dt, rng.integers(1, 256, dt.shape), 0).astype(np.uint8)).to(DEV))      # nonzero means set
        else:
            _overlap(vkn, dt, gt, _as_f32(rng, dt), thr=0.5)


@pytest.mark.parametrize('arm', ['u8', 'f32'])
def test_overlap_of_the_largest_shape_and_of_empty_sides(vkn, arm):
    rng = np.random.default_rng(2)
    K, G, H, W = 100, 37, 192, 320
    dt, gt = np.zeros((K, H, W), bool), np.zeros((G, H, W), bool)
    for m in (dt, gt):                                                     # boxes: instance masks are local
        for i in range(m.shape[0]):
            y, x, h, w = rng.integers(0, H - 8), rng.integers(0, W - 8), rng.integers(1, 80), rng.integers(1, 120)
            m[i, y:y + h, x:x + w] = True
    inter, _, _ = _overlap(vkn, dt, gt, None if arm == 'u8' else _as_f32(rng, dt), None if arm == 'u8' else 0.5)
    assert 0 < np.count_nonzero(inter) < inter.size
    small = _rand(rng, 3, 37, 131)
    none = np.zeros((0, 37, 131), bool)
    src = (lambda m: None) if arm == 'u8' else (lambda m: _as_f32(rng, m))
    thr = None if arm == 'u8' else 0.5
    _overlap(vkn, small, none, src(small), thr)                            # G = 0: the detections' areas, NULL for the other side
    _overlap(vkn, none, small, src(none), thr)                             # K = 0
    _overlap(vkn, none, none, src(none), thr)                              # nothing at all: no workspace, nothing launched


def test_overlap_of_uniform_disjoint_and_seam_masks(vkn):
    H, W = 2 * RUN + 3, 131
    ones = np.ones((2, H, W), bool)
    inter, adt, agt = _overlap(vkn, ones, ones[:1])
    assert inter.tolist() == [[H * W]] * 2 and adt.tolist() == [H * W] * 2 and agt.tolist() == [H * W]
    left, right = np.zeros((1, H, W), bool), np.zeros((1, H, W), bool)
    left[:, :, :64], right[:, :, 64:] = True, True                         # disjoint at the strip seam
    inter, _, _ = _overlap(vkn, np.concatenate([left, right]), np.concatenate([right, left, left | right]))
    assert inter.tolist() == [[0, 64 * H, 64 * H], [(W - 64) * H, 0, (W - 64) * H]]
    seam = np.zeros((3, H, W), bool)
    seam[0, :, 63], seam[1, :, 64], seam[2, :, 63:65] = True, True, True   # confined to the seam's two columns
    rows = np.zeros((2, H, W), bool)
    rows[0, RUN - 1], rows[1, RUN] = True, True                            # ... and to the two rows at a run's seam
    inter, _, _ = _overlap(vkn, seam, np.concatenate([seam, rows]))
    assert inter.tolist() == [[H, 0, H, 1, 1], [0, H, H, 1, 1], [H, H, 2 * H, 2, 2]]
    _overlap(vkn, np.zeros((2, H, W), bool), ones)


def test_overlap_f32_at_the_threshold(vkn):
    thr = np.float32(0.5)
    up, down = np.nextafter(thr, np.float32(1)), np.nextafter(thr, np.float32(0))
    vals = np.array([thr, up, down, np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0], dtype=np.float32)
    K, H, W = 2, 5, 67
    logits = np.resize(vals, (K, H, W)).astype(np.float32)
    want = logits > thr
    assert np.array_equal(want, np.isin(np.resize(np.arange(9), (K, H, W)), (1, 4, 8)))      # nextafter above, +inf and 1.0: nothing else
    gt = np.ones((1, H, W), bool)
    inter, adt, _ = _overlap(vkn, want, gt, torch.from_numpy(logits).to(DEV), thr=float(thr))
    assert adt.tolist() == want.reshape(K, -1).sum(1).tolist() == inter[:, 0].tolist()


def test_two_calls_add_and_the_same_input_gives_the_same_bits(vkn):
    rng = np.random.default_rng(5)
    K, G, H, W = 5, 4, RUN + 5, 70
    frames = [(_rand(rng, K, H, W), _rand(rng, G, H, W)) for _ in range(2)]
    out = None
    for dt, gt in frames:                                                  # the tube tables of two frames
        out = vkn.ops.mask_overlap(torch.from_numpy(dt).to(DEV), torch.from_numpy(gt).to(DEV), out=out)
    want = [a + b for a, b in zip(R.overlaps(*frames[0]), R.overlaps(*frames[1]))]
    assert all(np.array_equal(o.cpu().numpy(), w) for o, w in zip(out, want))
    a = vkn.ops.mask_overlap(torch.from_numpy(frames[0][0]).to(DEV), torch.from_numpy(frames[0][1]).to(DEV))
    b = vkn.ops.mask_overlap(torch.from_numpy(frames[0][0]).to(DEV), torch.from_numpy(frames[0][1]).to(DEV))
    assert all(torch.equal(x, y) for x, y in zip(a, b)) and all(np.array_equal(x.cpu().numpy(), w) for x, w in zip(a, R.overlaps(*frames[0])))
    assert a[0].data_ptr() % 16 == a[1].data_ptr() % 16 == a[2].data_ptr() % 16 == 0
    f = vkn.ops.mask_overlap(_as_f32(rng, frames[0][0]), torch.from_numpy(frames[0][1]).to(DEV), thr=0.5)
    assert all(torch.equal(x, y) for x, y in zip(a, f))


def test_overlap_refusals_with_device_memory(vkn):
    L = vkn._lib.lib()
    K, G, H, W = 2, 2, 5, 7
    nb = L.vkn_mask_overlap_workspace_bytes(K, G, H, W)
    dt, gt = torch.ones((K, H, W), dtype=torch.uint8, device=DEV), torch.ones((G, H, W), dtype=torch.uint8, device=DEV)
    outs = {k: torch.full((n,), 0x5A, dtype=torch.uint8, device=DEV) for k, n in (('inter', 8 * K * G + 16), ('area_dt', 8 * K), ('area_gt', 8 * G), ('ws', nb + 16))}

    def call(ws_bytes=nb, K=K, H=H, **kw):
        a = dict(dt=dt.data_ptr(), gt=gt.data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})
        a.update(kw)
        return L.vkn_mask_overlap_u8(a['dt'], a['gt'], K, G, H, W, a['inter'], a['area_dt'], a['area_gt'], a['ws'], ws_bytes, None)
    with torch.cuda.device(DEV):
        assert call(dt=None) == call(K=-1) == E_ARG and call(K=1025) == call(H=0, ws_bytes=0) == E_SHAPE
        assert call(ws_bytes=nb + 16) == call(ws_bytes=nb - 16, inter=outs['inter'].data_ptr() + 8) == E_WORKSPACE
        assert call(inter=outs['inter'].data_ptr() + 8) == call(ws=outs['ws'].data_ptr() + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in outs.values())


def test_one_overlap_capture_replayed_on_two_inputs_equals_eager(vkn):
    rng = np.random.default_rng(13)
    K, G, H, W = 3, 4, RUN + 1, 71
    inputs = [(_rand(rng, K, H, W), _rand(rng, G, H, W)), (_rand(rng, K, H, W, 0.2), _rand(rng, G, H, W, 0.8))]
    dt, gt = torch.zeros((K, H, W), dtype=torch.uint8, device=DEV), torch.zeros((G, H, W), dtype=torch.uint8, device=DEV)
    out = tuple(torch.zeros(s, dtype=torch.int64, device=DEV) for s in ((K, G), (K,), (G,)))
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        vkn.ops.mask_overlap(dt, gt, out=out)                              # warm-up: the code object and the workspace exist before the capture
    stream.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        vkn.ops.mask_overlap(dt, gt, out=out)
    for a, b in inputs + inputs[:1]:
        dt.copy_(torch.from_numpy(a.astype(np.uint8)))
        gt.copy_(torch.from_numpy(b.astype(np.uint8)))
        for t in out:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
        eager = _overlap(vkn, a, b)
        assert all(np.array_equal(t.cpu().numpy(), e) for t, e in zip(out, eager))


# ------------------------------------------------------------------------------------------------------------------------ match
def _cfg(vkn, num_classes, thrs, areas, max_det, cap):
    return vkn.ops.mask_ap_cfg(num_classes, thrs, areas, max_det, cap)


def _expect_records(images, num_classes, thrs, areas, max_det):
    """the log the device must hold after `images` (in this order), npig, and match_gt of the last image: from maskap_ref.evaluate_img"""
    T, A = len(thrs), len(areas)
    recs, npig, match_gt = [], np.zeros((num_classes, A), np.int64), None
    for im in images:
        K = len(im['dt_scores'])
        rec = np.zeros((K, REC), np.int64)
        rec[:, 0], rec[:, 1], rec[:, 2], rec[:, 3] = im['image_id'], im['dt_labels'], im['dt_scores'].view(np.int32), -1
        match_gt = -np.ones((A, T, K), np.int64)
        for c in range(num_classes):
            for a, rng in enumerate(areas):
                e = R.evaluate_img(im['tables'], im['dt_scores'], im['dt_labels'], im['gt_labels'], im['gt_iscrowd'], im['gt_area'], c, rng, thrs, max_det)
                npig[c, a] += e['npig']
                for di, k in enumerate(e['dt']):
                    rec[k, 3] = di
                    rec[k, 4 + 2 * a] = sum(1 << t for t in range(T) if e['matched'][t][di])
                    rec[k, 5 + 2 * a] = sum(1 << t for t in range(T) if e['ignored'][t][di])
                    for t in range(T):
                        match_gt[a, t, k] = e['gt_of'][t][di]
        recs.append(rec)
    return (np.concatenate(recs) if recs else np.zeros((0, REC), np.int64)), npig, match_gt


def _match(vkn, images, num_classes, thrs, areas, max_det, cap, want_status=0):
    """the images through vkn_mask_ap_match, state and match_gt in a guarded arena; compared with the restatement bit for bit"""
    L = vkn._lib.lib()
    cfg = _cfg(vkn, num_classes, thrs, areas, max_det, cap)
    nbytes, off = vkn.ops.mask_ap_layout(cfg)
    T, A = len(thrs), len(areas)
    A_ = Arena(DEV)
    state = A_.out((nbytes,), torch.uint8, 'state')
    mgs = [A_.out((A, T, len(im['dt_scores'])), torch.int32, f'match_gt{i}') for i, im in enumerate(images)]
    with torch.cuda.device(DEV):
        assert L.vkn_mask_ap_reset(ctypes.byref(cfg), state.ptr, nbytes, vkn.ops._stream()) == 0
        for im, mg in zip(images, mgs):
            dev = [torch.from_numpy(np.ascontiguousarray(x)).to(DEV) if x is not None else None
                   for x in (*im['tables'], im['dt_scores'], im['dt_labels'], im['gt_labels'], im['gt_iscrowd'], im['gt_area'])]
            K, G = len(im['dt_scores']), len(im['gt_labels'])
            ptrs = [ctypes.c_void_p(t.data_ptr() if t is not None and t.numel() else None) for t in dev]
            with frozen(*[t for t in dev if t is not None and t.numel()]):
                rc = L.vkn_mask_ap_match(ctypes.byref(cfg), state.ptr, nbytes, *ptrs, K, G, int(im['image_id']), mg.ptr, vkn.ops._stream())
            assert rc == 0
    A_.check(f'vkn_mask_ap_match {len(images)} images')
    raw = state.t.cpu().numpy()
    status, count = (int(v) for v in raw[:8].view(np.uint32))
    assert not raw[8:256].any()
    want_rec, want_npig, want_mg = _expect_records(images, num_classes, thrs, areas, max_det)
    assert status == want_status and count == len(want_rec)
    npig = raw[off[1]:off[1] + 8 * num_classes * A].view(np.int64).reshape(num_classes, A)
    assert np.array_equal(npig, want_npig), (npig, want_npig)
    n = min(count, cap)
    rec = raw[off[2]:off[2] + 48 * n].view(np.int32).reshape(n, REC)
    assert np.array_equal(rec.astype(np.int64), want_rec[:n].astype(np.int32).astype(np.int64)), (rec[:6], want_rec[:6])
    assert not raw[off[2] + 48 * n:].any()                                  # nothing at or beyond the capacity (the reset's zeros)
    if images and mgs[-1].nbytes:
        assert np.array_equal(mgs[-1].t.cpu().numpy(), want_mg)
    return rec, npig


def test_every_matching_rule_through_the_c_abi(vkn):
    for name, case in match_cases().items():
        im, want = case['image'], case['want']
        T = len(case['thrs'])
        rec, npig = _match(vkn, [im], 2, case['thrs'], [case['area']], case.get('max_det', 100), 16)
        assert npig[0, 0] == want['npig'], name
        for di, k in enumerate(want['dt']):                                # ... and against the answers worked by hand
            assert rec[k, 3] == di and rec[k, 4] == sum(1 << t for t in range(T) if want['matched'][t][di]), (name, k)
            assert rec[k, 5] == sum(1 << t for t in range(T) if want['ignored'][t][di]), (name, k)


def _random_image(rng, image_id, K, G, num_classes, crowd=True, area=True):
    """hand-built integer tables: areas and intersections drawn so that IoUs spread over (0, 1] with many exact ties"""
    adt, agt = rng.integers(1, 40, K) * 100, rng.integers(1, 40, G) * 100
    inter = np.minimum(adt[:, None], agt[None, :]) * rng.integers(0, 5, (K, G)) // 4
    inter[rng.random((K, G)) < 0.5] = 0
    scores = np.round(rng.random(K), 1).astype(np.float32)                 # tied scores
    return img(image_id, inter, adt, agt, scores, rng.integers(0, num_classes, K), rng.integers(0, num_classes, G),
               crowd=(rng.random(G) < 0.2) if crowd else None, area=(agt * rng.choice([0.5, 1.0, 3.0], G)) if area else None)


@pytest.mark.parametrize('T,A', [(1, 1), (16, 4), (10, 4)])
def test_random_tables_several_images(vkn, T, A):
    rng = np.random.default_rng(100 + T)
    thrs = np.linspace(0.05, 0.95, T) if T > 1 else [0.5]
    areas = R.COCO_AREAS[:A]
    C = 4                                                                   # category 3 gets no detections, category 2 no ground truths
    ims = []
    for i, (K, G) in enumerate(((7, 5), (0, 3), (4, 0), (70, 66), (1, 1))):
        im = _random_image(rng, 10 - i, K, G, C, crowd=i != 4, area=i % 2 == 0)
        im['dt_labels'][im['dt_labels'] == 3] = 0
        im['gt_labels'][im['gt_labels'] == 2] = 1
        ims.append(im)
    _match(vkn, ims, C, thrs, areas, 100, 128)


def test_more_detections_than_max_det(vkn):
    rng = np.random.default_rng(7)
    max_det = 5
    im = _random_image(rng, 1, max_det + 1, 4, 1)
    rec, _ = _match(vkn, [im], 1, [0.3, 0.6], R.COCO_AREAS, max_det, 8)
    assert sorted(rec[:, 3].tolist()) == [-1, 0, 1, 2, 3, 4]
    big = _random_image(rng, 2, 300, 40, 2)                                 # more than one wave of detections per category, cut at 100
    _match(vkn, [big], 2, [0.5], R.COCO_AREAS[:1], 100, 300)
    wide = _random_image(rng, 3, 5, 130, 1)                                 # ... and of ground truths
    _match(vkn, [wide], 1, [0.5, 0.9], R.COCO_AREAS[:2], 100, 8)


def test_capacity_exact_and_one_short(vkn):
    rng = np.random.default_rng(8)
    ims = [_random_image(rng, i, K, 3, 2) for i, K in enumerate((4, 3))]
    _match(vkn, ims, 2, [0.5, 0.75], R.COCO_AREAS, 100, 7)                      # exact: no FULL
    _match(vkn, ims, 2, [0.5, 0.75], R.COCO_AREAS, 100, 6, want_status=FULL)    # one short: count stays 7, nothing behind record 5
    _match(vkn, ims, 2, [0.5, 0.75], R.COCO_AREAS, 100, 3, want_status=FULL)    # the first call already overflows


def test_label_range_and_nan_scores_are_flagged(vkn):
    im = img(1, [[100, 0], [0, 100], [100, 0]], [100] * 3, [100, 100], [0.9, 0.8, 0.7], [0, 5, -1], [0, 7])
    rec, npig = _match(vkn, [im], 2, [0.5], R.COCO_AREAS[:1], 100, 8, want_status=LABEL_RANGE)
    assert rec[:, 3].tolist() == [0, -1, -1] and npig.sum() == 1
    nan = img(1, [[100], [100], [100]], [100] * 3, [100], [np.nan, 0.2, np.nan], [0, 0, 0], [0])
    rec, _ = _match(vkn, [nan], 1, [0.5], R.COCO_AREAS[:1], 100, 8, want_status=SCORE_NAN)
    assert rec[:, 3].tolist() == [1, 0, 2] and rec[:, 4].tolist() == [0, 1, 0]          # NaN behind every number, in input order


# ------------------------------------------------------------------------------------------------------------------------ meter
def _blob_images(rng):
    """eight images of 48 x 80 and 37 x 131, three classes: box ground truths, jittered detections, one crowd, one image without ground
    truth and one without detections"""
    ims = []
    for i in range(8):
        H, W = ((48, 80), (37, 131))[i % 2]
        G = 0 if i == 3 else int(rng.integers(1, 5))
        gt = np.zeros((G, H, W), bool)
        boxes = []
        for g in range(G):
            h, w = int(rng.integers(4, H // 2)), int(rng.integers(4, W // 2))
            y, x = int(rng.integers(0, H - h)), int(rng.integers(0, W - w))
            gt[g, y:y + h, x:x + w] = True
            boxes.append((y, x, h, w))
        gl = rng.integers(0, 3, G)
        crowd = np.zeros(G, np.uint8)
        if i == 1 and G:
            crowd[0] = 1
        dts, dl = [], []
        if i != 5:
            for g, (y, x, h, w) in enumerate(boxes):
                for _ in range(int(rng.integers(1, 3))):                    # jittered copies of a ground truth, sometimes of another class
                    m = np.zeros((H, W), bool)
                    dy, dx = rng.integers(-3, 4, 2)
                    m[max(0, y + dy):y + dy + h, max(0, x + dx):x + dx + w] = True
                    dts.append(m)
                    dl.append(gl[g] if rng.random() < 0.8 else (gl[g] + 1) % 3)
            for _ in range(2):                                              # and false positives
                m = np.zeros((H, W), bool)
                y, x = int(rng.integers(0, H - 6)), int(rng.integers(0, W - 6))
                m[y:y + 6, x:x + 6] = True
                dts.append(m)
                dl.append(int(rng.integers(0, 3)))
        K = len(dts)
        ims.append(dict(image_id=100 - 7 * i if i % 3 else 7 * i, dt_masks=np.stack(dts) if K else np.zeros((0, H, W), bool),
                        dt_scores=np.round(rng.random(K), 2).astype(np.float32), dt_labels=np.asarray(dl, np.int32).reshape(K), gt_masks=gt,
                        gt_labels=gl.astype(np.int32), gt_iscrowd=crowd, gt_area=(gt.sum(axis=(1, 2)) * 1.5) if i % 2 else None))
    return ims


def _feed(vkn, meter, ims, f32=False):
    for im in ims:
        t = lambda a, dt=None: torch.from_numpy(np.ascontiguousarray(a)).to(DEV) if dt is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV).to(dt)      # noqa: E731
        dtm = t(np.where(im['dt_masks'], 0.75, 0.25).astype(np.float32)) if f32 else t(im['dt_masks'])
        meter.update(im['image_id'], dtm, t(im['dt_scores']), t(im['dt_labels'], torch.int64), t(im['gt_masks']), t(im['gt_labels'], torch.int64),
                     t(im['gt_iscrowd']), t(im['gt_area']) if im['gt_area'] is not None else None, thr=0.5 if f32 else None)


def test_meter_equals_the_restatement_bit_for_bit(vkn):
    ims = _blob_images(np.random.default_rng(21))
    assert [im['image_id'] for im in ims] != sorted(im['image_id'] for im in ims) and len({im['image_id'] for im in ims}) == 8      # out of id order
    want = R.evaluate(ims, 3)
    meter, twin = vkn.MaskAPMeter(3, capacity=256, device=DEV), vkn.MaskAPMeter(3, capacity=256)
    _feed(vkn, meter, ims)
    _feed(vkn, twin, ims, f32=True)
    out = meter.result()
    assert np.array_equal(out['precision'], want['precision']) and np.array_equal(out['recall'], want['recall'])
    assert list(out['stats'].values()) == want['stats'] and np.array_equal(out['classwise'], want['classwise'], equal_nan=True)
    assert np.array_equal(meter.counts()['npig'], want['npig']) and meter.counts()['records'] == sum(len(im['dt_scores']) for im in ims)
    assert 0 < out['stats']['mAP'] <= 1 and (out['precision'] > 0).any() and want['npig'][:, 0].sum() > 0
    r = meter.records()
    assert r['image'].tolist() == [im['image_id'] for im in ims for _ in im['dt_scores']] and r['matched'].shape == (len(r['image']), 4)
    # a second meter fed the same updates (the fp32 arm of the overlap) holds the same state bytes
    assert np.array_equal(meter.state_bytes(), twin.state_bytes()) and meter.state_bytes().size == vkn.ops.mask_ap_layout(meter._cfg)[0]
    meter.reset()
    assert meter.counts()['records'] == 0 and not meter.state_bytes().any()


def test_full_log_makes_result_raise(vkn):
    ims = _blob_images(np.random.default_rng(21))[:3]
    meter = vkn.MaskAPMeter(3, capacity=2)
    _feed(vkn, meter, ims)
    with pytest.raises(vkn.VknError):
        meter.result()
    with pytest.raises(vkn.VknError):
        meter.check_status()
    assert meter.counts()['records'] == sum(len(im['dt_scores']) for im in ims) and len(meter.records()['image']) == 2


@pytest.mark.parametrize('typ', ['KernelUpdateHead', 'KernelUpdateHeadVideo'])
def test_get_seg_masks_device_feeds_the_meter_as_get_seg_masks_does(vkn, typ):
    extra = dict(num_proposals=5, query_merge_method='mean') if typ.endswith('Video') else {}
    head = vkn.build_head(vkn.configs.mask_head_cfg(False, C=32, heads=8, ffn=64, ncls=4, n_thing=4, n_stuff=0, up=1, head_type=typ, loss_rank=None,
                                                    **extra)).to(DEV).eval()
    g = torch.Generator().manual_seed(3)
    K = 5
    low = (torch.randn((K, 12, 20), generator=g) * 3).to(DEV)
    low[2] = -5.0                                                           # an empty mask
    labels, scores = torch.tensor([2, 0, 2, 3, 0], device=DEV), torch.rand((K,), generator=g).to(DEV)
    meta = dict(img_shape=(45, 77, 3), batch_input_shape=(48, 80), ori_shape=(71, 123, 3))
    test_cfg = dict(mask_thr=0.5, max_per_img=K)
    with frozen(low, labels, scores):
        _, segm_ref = head.get_seg_masks(low, labels, scores, test_cfg, meta)
        masks, lab, sc = head.get_seg_masks_device(low, labels, scores, test_cfg, meta)
    assert masks.is_cuda and masks.dtype == torch.bool and tuple(masks.shape) == (K, 71, 123) and lab is labels and sc is scores
    per_class = [list(c) for c in segm_ref]
    host = np.stack([per_class[int(l)].pop(0) for l in labels.cpu()])      # get_seg_masks' boolean masks back in detection order
    assert np.array_equal(masks.cpu().numpy(), host)
    gt = np.zeros((2, 71, 123), bool)
    gt[0], gt[1, 10:40, 20:90] = host[0], True
    a, b = vkn.MaskAPMeter(4, capacity=16), vkn.MaskAPMeter(4, capacity=16)
    gtt, gl = torch.from_numpy(gt).to(DEV), torch.tensor([2, 0], device=DEV)
    a.update(1, masks, sc, lab, gtt, gl)
    b.update(1, torch.from_numpy(host).to(DEV), sc, lab, gtt, gl)
    assert np.array_equal(a.state_bytes(), b.state_bytes())
    want = R.evaluate([dict(image_id=1, dt_masks=host, dt_scores=scores.cpu().numpy(), dt_labels=labels.cpu().numpy(), gt_masks=gt, gt_labels=[2, 0])], 4)
    out = a.result()
    assert np.array_equal(out['precision'], want['precision']) and list(out['stats'].values()) == want['stats'] and want['npig'][2, 0] == 1
