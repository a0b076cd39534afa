"""The references of the ground-truth preparation (tests/gt_prep_ref.py) checked on their own, without a GPU: the NumPy restatement
and `GtPrep`'s torch composition against the reference's fixtures, bit for bit; the 2 x 2-centre identity the kernels build on; the
three label tables; and what the fourth part of the C ABI (include/vkn_gt.h) promises before any launch."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import gt_prep_ref as R

E_ARG, E_SHAPE, E_ALIGN = -1, -2, -5


def _check_against_fixture(c, masks, sem_cls, sem_seg):
    """what a preparation returned (arrays) against what the reference returned; for an image without stuff the reference gives G_b
    rows of zeros, the preparation an empty [0, aH, aW] (the documented deviation)"""
    for b in range(c.B):
        assert masks[b].dtype == np.float32 and np.array_equal(masks[b], c.out_masks[b]), b
    if c.sem is None:
        assert sem_cls is None and sem_seg is None
        return
    for b in range(c.B):
        assert sem_cls[b].dtype == np.int64 and np.array_equal(sem_cls[b], c.out_sem_cls[b]), b
        if len(c.out_sem_cls[b]):
            assert sem_seg[b].dtype == np.float32 and np.array_equal(sem_seg[b], c.out_sem_seg[b]), b
        else:
            assert sem_seg[b].shape == (0,) + c.out_masks[b].shape[1:] and not c.out_sem_seg[b].any()


@pytest.mark.parametrize('name', R.FIXTURES)
def test_restatement_equals_the_fixtures(name):
    c = R.load(name)
    want = R.reference(c)
    G = [m.shape[0] for m in c.masks]
    masks = [want.bank[r:r + g] for r, g in zip(want.thing_row0, G)]
    seg = [want.bank[r:r + n] for r, n in zip(want.sem_row0, want.n_sem)]
    _check_against_fixture(c, masks, None if c.sem is None else want.labels, None if c.sem is None else seg)
    assert want.status == 0 and want.bank.shape[0] == sum(G) + sum(want.n_sem)
    for listed in want.classes:
        assert listed == sorted(listed)


def test_fixtures_hit_their_edges():
    k = R.reference(R.load('kitti_s2'))
    assert k.n_sem[2] == 0 and k.n_sem[0] > 0 and R.load('kitti_s2').masks[1].shape[0] == 0
    assert 10 in k.classes[0] and 12 in k.classes[0] and 14 in k.classes[0] and 11 not in k.classes[0] and 13 not in k.classes[0]
    assert R.load('generic_s8').masks[0].max() == 255
    e = R.reference(R.EDGE_CASES['class_edges_uint8']())
    assert e.classes == [[0, 7, 20, 21, 254]] and e.labels[0].tolist() == [3, 10, 23, 24, 257]
    rows = e.bank[e.sem_row0[0]:]
    assert not rows[2].any() and rows[3].sum() == 0.25 and (rows[3] > 0).sum() == 1 and rows[3][1, 1] == 0.25
    assert R.reference(R.EDGE_CASES['out_of_range']()).status == R.STATUS_RANGE
    r = R.reference(R.EDGE_CASES['ragged_s4']())
    assert r.n_sem[3] == 0 and r.thing_row0[2] == r.sem_row0[1] + r.n_sem[1]


@pytest.mark.parametrize('name', R.FIXTURES)
def test_torch_composition_equals_the_fixtures(vkn, name):
    """CPU tensors decline the fused path; the composition gives the reference's bits, leaves the caller's map alone, and needs no
    library"""
    c = R.load(name)
    sem_before = None if c.sem is None else c.sem.copy()
    prep, masks, sem_cls, sem_seg = R.run(vkn, c, 'cpu')
    assert prep.fused is False and prep.bank is None
    arr = lambda ts: None if ts is None else [t.numpy() for t in ts]  # noqa: E731
    _check_against_fixture(c, arr(masks), arr(sem_cls), arr(sem_seg))
    want = R.reference(c)
    assert prep.n_sem == want.n_sem and prep.classes == want.classes and prep.status_word == 0
    if c.sem is not None:
        assert np.array_equal(c.sem, sem_before)


def test_torch_composition_outside_the_envelope(vkn):
    """an odd stride and sizes the stride does not divide stay on the composition: the reference's op sequence"""
    rng = np.random.default_rng(5)
    m = R.blobs(rng, 2, 31, 50)
    sem = torch.from_numpy(R.sem_map(rng, 1, 33, 51, [0, 1, 2, 255]))[:, None]
    prep = vkn.GtPrep(3, 4, 9, dataset='cityscapes')
    masks, cls, seg = prep.preprocess_gt_masks([dict(batch_input_shape=(33, 51), img_shape=(31, 50, 3))], [R.Bitmap(m)],
                                               [torch.zeros(2, dtype=torch.int64)], sem)
    t = F.pad(torch.from_numpy(m).float(), (0, 1, 0, 2))
    assert prep.fused is False and torch.equal(masks[0], F.interpolate(t[None], (11, 17), mode='bilinear', align_corners=False)[0])
    s2 = sem[0].clone()
    s2[:, 31:, :] = 255
    s2[:, :, 50:] = 255
    want = torch.cat([s2 == c for c in (0, 1, 2)]).float()
    assert cls[0].tolist() == [4, 5, 6] and torch.equal(seg[0], F.interpolate(want[None], (11, 17), mode='bilinear', align_corners=False)[0])
    fl = vkn.GtPrep(2, 4, 9).preprocess_gt_masks([dict(batch_input_shape=(4, 4), img_shape=(4, 4, 3))], [torch.rand(1, 4, 4)],
                                                 [torch.zeros(1, dtype=torch.int64)], None)
    assert fl[1] is None and fl[2] is None and fl[0][0].shape == (1, 2, 2)


@pytest.mark.parametrize('s', [2, 4, 8])
@pytest.mark.parametrize('shape', [(34, 70), (32, 72), (48, 80)])
def test_two_by_two_centre_identity(s, shape):
    """`F.interpolate(bilinear, align_corners=False)` at an even integer factor IS the mean of the 2 x 2 centre pixels, bit for bit,
    for byte-valued inputs (0 / 1 and 0..255)"""
    H, W = (v // s * s for v in shape)
    rng = np.random.default_rng(s)
    for hi in (2, 256):
        x = rng.integers(0, hi, (3, H, W)).astype(np.float64)
        got = F.interpolate(torch.from_numpy(x).float()[None], (H // s, W // s), mode='bilinear', align_corners=False)[0].numpy()
        assert np.array_equal(got, R.down(x, s).astype(np.float32))
    x = rng.integers(0, 256, (2, 9, 13)).astype(np.float64)
    assert np.array_equal(F.interpolate(torch.from_numpy(x).float()[None], (9, 13), mode='bilinear', align_corners=False)[0].numpy(), x)


def test_label_tables_equal_the_reference_functions(vkn):
    """for every class 0..255: the table `GtPrep` hands the kernel, the restatement's, and the labels the three reference functions
    returned for a map holding every value (-1: not listed)"""
    g = np.load(R.GOLDEN + '/gt_prep_tables.npz')
    from video_k_net_amd.gt_prep import label_of_class
    for key, args in (('generic_t80_thing0', ('generic', 80, 53, 255, 0)), ('generic_t4_thing3', ('generic', 4, 9, 255, 3)),
                      ('cityscapes_t8_s11', ('cityscapes', 8, 11, 255, None)), ('vipseg_t58_s66', ('vipseg', 58, 66, 255, None)),
                      ('kitti_step', ('kitti_step', 2, 17, 255, None))):
        assert label_of_class(*args) == g[key].tolist(), key
        assert np.array_equal(R.table(*args), g[key]), key
    assert vkn.GtPrep(2, 2, 17, dataset='kitti_step').label_of_class[10:15] == [12, -1, 13, -1, 14]
    assert label_of_class('generic', 80, 53, 255, None) == label_of_class('generic', 80, 53, 255, 0)
    with pytest.raises(ValueError):
        label_of_class('coco', 80, 53)


def test_match_indices_restatement_and_composition(vkn):
    keys, refs, pids = R.load_match()
    assert len(keys[-1]) == len(refs[-1]) == 1024 and (pids[-1] >= 0).any() and (pids[-1] < 0).any()
    assert pids[0].tolist() == [1, -1, 0, 1]                    # a duplicate reference id: the first index; an absent id: -1
    for got, want in zip(R.match(keys, refs), pids):
        assert np.array_equal(got, want)
    prep = vkn.GtPrep(2, 2, 17)
    out = prep.match_indices([torch.from_numpy(k) for k in keys], [torch.from_numpy(r) for r in refs])
    assert prep.fused is False and prep.match_off.tolist() == [0] + np.cumsum([len(k) for k in keys]).tolist()
    for got, want in zip(out, pids):
        assert got.dtype == torch.int64 and np.array_equal(got.numpy(), want)
        assert got.numel() == 0 or got.untyped_storage().data_ptr() == prep.match.untyped_storage().data_ptr()


# ---------------------------------------------------------------------------------------------------- the ABI, before any launch
def test_gt_entries_refuse_before_any_launch(vkn):
    """NULL pointers, shapes outside the envelope and misaligned pointers are refused by the host-side checks, in this order, before a
    pointer is looked at (the fake pointers below are never dereferenced)"""
    lib = vkn._lib
    L = lib.lib()
    p = 0x10000
    table = (ctypes.c_int * 256)(*range(256))

    def imgs(B=2, **kw):
        a = (lib.VknGtImage * max(B, 1))()
        for b in range(max(B, 1)):
            f = dict(masks=p, sem=p, classes=p, G=2, Hm=30, Wm=61, valid_h=29, valid_w=59, n_sem=3, row0=5 * b, sem_row0=5 * b + 2)
            f.update(kw)
            a[b] = lib.VknGtImage(**f)
        return a

    def classes(B=2, Hp=32, Wp=72, i64=0, im=None, tab=table, flags=p, n_sem=p, cls=p, labels=p, status=p, **kw):
        return L.vkn_gt_classes(imgs(B, **kw) if im is None else im, B, Hp, Wp, i64, tab, flags, n_sem, cls, labels, status, None)

    def fill(B=2, Hp=32, Wp=72, s=4, i64=0, im=None, bank=p, G_total=10, **kw):
        return L.vkn_gt_bank_fill_f32(imgs(B, **kw) if im is None else im, B, Hp, Wp, s, i64, bank, G_total, None)

    def match(key=p, klen=(3, 4), ref=p, rlen=(2, 0), B=2, out=p, off=p):
        kl = (ctypes.c_int * len(klen))(*klen) if klen is not None else None
        rl = (ctypes.c_int * len(rlen))(*rlen) if rlen is not None else None
        return L.vkn_gt_match_indices(key, kl, ref, rl, B, out, off, None)

    # VKN_E_ARG
    for name in ('tab', 'flags', 'n_sem', 'cls', 'labels', 'status'):
        assert classes(**{name: None}) == E_ARG, name
    assert classes(sem=None) == E_ARG and classes(B=-1) == E_ARG
    assert L.vkn_gt_classes(None, 2, 32, 72, 0, table, p, p, p, p, p, None) == E_ARG
    assert fill(bank=None) == E_ARG and fill(B=-1) == E_ARG and L.vkn_gt_bank_fill_f32(None, 2, 32, 72, 4, 0, p, 10, None) == E_ARG
    assert fill(masks=None) == E_ARG and fill(sem=None) == E_ARG and fill(classes=None) == E_ARG and fill(G=-1) == E_ARG
    for name in ('klen', 'rlen', 'off', 'key', 'ref', 'out'):
        assert match(**{name: None}) == E_ARG, name
    assert match(klen=(3, -1)) == E_ARG
    # VKN_E_SHAPE
    assert classes(B=0) == E_SHAPE and classes(B=65) == E_SHAPE and classes(Hp=0) == E_SHAPE and classes(Hp=1 << 16, Wp=1 << 15) == E_SHAPE
    assert classes(valid_h=33) == E_SHAPE and classes(valid_w=-1) == E_SHAPE
    assert fill(B=0) == E_SHAPE and fill(B=65) == E_SHAPE
    for s in (0, 3, 5, 6, 16):
        assert fill(s=s, Hp=240, Wp=480) == E_SHAPE, s
    assert fill(Hp=34) == E_SHAPE and fill(Wp=70) == E_SHAPE and fill(s=8, Hp=32, Wp=76) == E_SHAPE
    assert fill(Hm=33) == E_SHAPE and fill(Wm=73) == E_SHAPE and fill(Hm=0) == E_SHAPE
    assert fill(G_total=0) == E_SHAPE and fill(G_total=9) == E_SHAPE and fill(row0=-1) == E_SHAPE and fill(n_sem=257) == E_SHAPE
    assert fill(Hp=2048, Wp=4096, s=1, G_total=64) == E_SHAPE            # 64 * 2048 * 4096 * 4 = 2^31
    assert fill(valid_h=33) == E_SHAPE
    assert fill(Hp=262144, Wp=4, s=1, Hm=30, Wm=4, valid_w=4, G_total=10) == E_SHAPE          # aH beyond the fill's grid
    assert classes(Hp=524288, Wp=4, valid_w=4) == E_SHAPE                                     # Hp beyond the presence pass's grid
    assert match(B=0) == E_SHAPE and match(B=65, klen=(1,) * 65, rlen=(1,) * 65) == E_SHAPE
    assert match(klen=(3, 1025)) == E_SHAPE and match(rlen=(1025, 0)) == E_SHAPE
    # VKN_E_ALIGN
    assert fill(bank=p + 4) == E_ALIGN and fill(bank=p + 8) == E_ALIGN
    assert fill(i64=1, sem=p + 4) == E_ALIGN
    for name in ('flags', 'n_sem', 'status'):
        assert classes(**{name: p + 2}) == E_ALIGN, name
    assert classes(labels=p + 4) == E_ALIGN and classes(i64=1, sem=p + 4) == E_ALIGN
    for name in ('key', 'ref', 'out', 'off'):
        assert match(**{name: p + 4}) == E_ALIGN, name
    # the order: ARG before SHAPE before ALIGN; then the fake pointers turn out not to be device memory
    assert fill(bank=None, s=3) == E_ARG and fill(s=3, bank=p + 4) == E_SHAPE
    assert classes(flags=None, B=0) == E_ARG and classes(B=0, flags=p + 2) == E_SHAPE
    assert match(off=None, B=0) == E_ARG and match(B=0, off=p + 4) == E_SHAPE
    assert fill() == E_ARG and classes() == E_ARG and match() == E_ARG


def test_envelope_by_shapes(vkn):
    """`gt_prep_supported` is what `GtPrep` asks before it takes the fused path"""
    ok = vkn.ops.gt_prep_supported
    assert ok(2, 384, 1248, 2) and ok(1, 1024, 2048, 4) and ok(64, 32, 72, 8) and ok(1, 9, 13, 1)
    assert not ok(65, 32, 72, 4) and not ok(0, 32, 72, 4) and not ok(1, 34, 70, 4) and not ok(1, 33, 51, 3) and not ok(1, 32, 64, 16)
    assert ok(1, 262140, 4, 1) and not ok(1, 262144, 4, 1) and ok(1, 524280, 8, 8) and not ok(1, 524288, 8, 8)
