"""The ground-truth preparation on the device (`vkn.GtPrep`, csrc/vkn_gtprep.hip) against tests/gt_prep_ref.py and the reference's
fixtures: zero tolerance throughout — every value is a count of at most four pixels, or a sum of at most four bytes, times 1/4."""
import numpy as np
import pytest
import torch

import gt_prep_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _cases():
    return [(n, 'fixture') for n in R.FIXTURES] + [(n, 'edge') for n in R.EDGE_CASES]


def _case(name, kind):
    return R.load(name) if kind == 'fixture' else R.EDGE_CASES[name]()


def _check(c, prep, masks, sem_cls, sem_seg):
    """everything the call returned and kept against the restatement: bank, views, labels, counts, class lists, status"""
    want = R.reference(c)
    assert prep.fused is True
    assert prep.bank.dtype == torch.float32 and prep.bank.is_contiguous() and torch.equal(prep.bank.cpu(), torch.from_numpy(want.bank))
    assert prep.thing_row0 == want.thing_row0
    assert prep.status_word == want.status
    size = want.bank[0].size * 4 if want.bank.shape[0] else 0
    for b in range(c.B):
        G = c.masks[b].shape[0]
        assert masks[b].shape[0] == G and (G == 0 or masks[b].data_ptr() == prep.bank.data_ptr() + want.thing_row0[b] * size)
    if c.sem is None:
        assert sem_cls is None and sem_seg is None and prep.n_sem == [0] * c.B
        return want
    assert prep.n_sem == want.n_sem and prep.classes == want.classes and prep.sem_row0 == want.sem_row0
    for b in range(c.B):
        assert sem_cls[b].dtype == torch.int64 and sem_cls[b].is_cuda and torch.equal(sem_cls[b].cpu(), torch.from_numpy(want.labels[b]))
        n = want.n_sem[b]
        assert tuple(sem_seg[b].shape) == (n,) + want.bank.shape[1:]
        assert n == 0 or sem_seg[b].data_ptr() == prep.bank.data_ptr() + want.sem_row0[b] * size
    return want


@pytest.mark.parametrize('name,kind', _cases())
def test_fused_preparation_equals_the_restatement(vkn, name, kind):
    """strides 1 / 2 / 4 / 8 with store tails (aW = 18, 35), ragged masks inside the pad, img_shape cutting 2 x 2 centres, B = 3 / 4 with
    an image without things and one all ignore, the class edges, the three dataset modes, uint8 and int64 maps, byte masks holding 255,
    vector and byte-wise loads, more than one column block; fixtures also against the reference's own outputs; two calls, same bits;
    the caller's map is not written"""
    c = _case(name, kind)
    sem_before = None if c.sem is None else c.sem.copy()
    prep, masks, sem_cls, sem_seg = R.run(vkn, c, DEV)
    _check(c, prep, masks, sem_cls, sem_seg)
    if kind == 'fixture':
        for b in range(c.B):
            assert torch.equal(masks[b].cpu(), torch.from_numpy(c.out_masks[b]))
            if c.sem is not None:
                assert torch.equal(sem_cls[b].cpu(), torch.from_numpy(c.out_sem_cls[b]))
                if len(c.out_sem_cls[b]):
                    assert torch.equal(sem_seg[b].cpu(), torch.from_numpy(c.out_sem_seg[b]))
    first = prep.bank.clone()
    again, *_ = R.run(vkn, c, DEV)
    assert torch.equal(first, again.bank) and again.n_sem == prep.n_sem and again.classes == prep.classes
    if c.sem is not None:
        assert np.array_equal(c.sem, sem_before)


def test_device_maps_and_tensor_masks_are_not_written(vkn):
    """uint8 / bool mask tensors already on the device and a device map: same bits, and the inputs keep theirs"""
    c = R.load('city_s4')
    want = R.reference(c)
    sem = torch.from_numpy(c.sem)[:, None].to(DEV)
    keep = sem.clone()
    for conv in (lambda m: torch.from_numpy(m).to(DEV), lambda m: torch.from_numpy(m).to(DEV).bool(), lambda m: torch.from_numpy(m)):
        prep = R.make_prep(vkn, c)
        prep.preprocess_gt_masks(R.metas(c), [conv(m) for m in c.masks], [torch.zeros(1, dtype=torch.int64, device=DEV)] * c.B, sem)
        assert prep.fused and torch.equal(prep.bank.cpu(), torch.from_numpy(want.bank)) and torch.equal(sem, keep)


def test_class_edges_on_the_device(vkn):
    """a class only inside the ignore region is not listed; one only at non-centre pixels is listed with an all-zero row; one at exactly
    one centre pixel gives a single 0.25; classes 0 and 254 are present — for both map types"""
    for name in ('class_edges_uint8', 'class_edges_int64'):
        c = R.EDGE_CASES[name]()
        prep, masks, sem_cls, sem_seg = R.run(vkn, c, DEV)
        assert prep.classes == [[0, 7, 20, 21, 254]] and sem_cls[0].tolist() == [3, 10, 23, 24, 257]
        rows = sem_seg[0].cpu()
        assert not rows[2].any() and float(rows[3].sum()) == 0.25 and float(rows[3][1, 1]) == 0.25
        assert float(masks[0].max()) == 255.0


def test_out_of_range_map_values_set_the_status_bit_and_count_as_ignore(vkn):
    c = R.EDGE_CASES['out_of_range']()
    prep, *_ = R.run(vkn, c, DEV)
    assert prep.status_word & R.STATUS_RANGE and prep.classes == R.reference(c).classes
    ok = R.load('kitti_s2')
    assert R.run(vkn, ok, DEV)[0].status_word == 0


def test_guard_rows_are_not_touched(vkn):
    """the bank with extra rows before and after, filled with a sentinel: the fill writes its rows and nothing else"""
    for name in ('ragged_s4', 'aligned_s2_uint8', 'kitti_s2'):
        c = R.EDGE_CASES[name]() if name in R.EDGE_CASES else R.load(name)
        want = R.reference(c)
        prep, *_ = R.run(vkn, c, DEV)
        sem = torch.from_numpy(c.sem).to(DEV)
        _, classes, _, _, _ = vkn.ops.gt_classes(sem, c.img_shape, prep.label_of_class)
        rows, (aH, aW) = want.bank.shape[0], want.bank.shape[1:]
        pad = 4                                           # guard rows on each side (4 keep the bank 16-byte aligned at odd aH * aW)
        guarded = torch.full((rows + 2 * pad, aH, aW), -7.0, dtype=torch.float32, device=DEV)
        masks = [torch.from_numpy(m).to(DEV) for m in c.masks]
        bank, row0, sem_row0 = vkn.ops.gt_bank_fill(masks, sem, c.img_shape, want.n_sem, classes, c.stride, c.pad, bank=guarded[pad:-pad])
        assert bank.data_ptr() == guarded[pad].data_ptr() and row0 == want.thing_row0 and sem_row0 == want.sem_row0
        assert torch.equal(guarded[pad:-pad].cpu(), torch.from_numpy(want.bank))
        assert bool((guarded[:pad] == -7.0).all()) and bool((guarded[-pad:] == -7.0).all())


def test_match_indices_on_the_device(vkn):
    """a duplicate reference id returns the first index, an absent id -1, empty key / reference lists work, 1024 ids work; the result
    is one tensor with its offsets, and the per-image tensors are views of it"""
    keys, refs, pids = R.load_match()
    prep = vkn.GtPrep(2, 2, 17)
    out = prep.match_indices([torch.from_numpy(k).to(DEV) for k in keys], [torch.from_numpy(r).to(DEV) for r in refs])
    assert prep.fused is True and prep.match.is_cuda and prep.match.dtype == torch.int64
    assert prep.match_off.tolist() == [0] + np.cumsum([len(k) for k in keys]).tolist()
    assert torch.equal(prep.match.cpu(), torch.from_numpy(np.concatenate(pids)))
    for got, want, a in zip(out, pids, prep.match_off.tolist()):
        assert torch.equal(got.cpu(), torch.from_numpy(want))
        assert got.numel() == 0 or got.data_ptr() == prep.match.data_ptr() + 8 * a
    again = vkn.GtPrep(2, 2, 17)
    again.match_indices([torch.from_numpy(k).to(DEV) for k in keys], [torch.from_numpy(r).to(DEV) for r in refs])
    assert torch.equal(again.match, prep.match)
    one = vkn.GtPrep(2, 2, 17).match_indices([torch.zeros(0, dtype=torch.int64, device=DEV)], [torch.zeros(0, dtype=torch.int64, device=DEV)])
    assert one[0].numel() == 0
    big = vkn.GtPrep(2, 2, 17)
    big.match_indices([torch.arange(1025, device=DEV)], [torch.arange(1025, device=DEV)])           # beyond the kernel: the composition
    assert big.fused is False and torch.equal(big.match.cpu(), torch.arange(1025))
    with pytest.raises(vkn.VknError):
        vkn.ops.gt_match_indices([torch.arange(1025, device=DEV)], [torch.arange(4, device=DEV)])


def test_outside_the_envelope_the_composition_runs_on_the_device(vkn):
    """an odd stride on CUDA tensors: `fused` is False and the values are the composition's; inside the envelope both agree bit for bit"""
    c = R.load('city_s4')
    prep, masks, sem_cls, sem_seg = R.run(vkn, c, DEV)
    comp = R.make_prep(vkn, c)
    m2, c2, s2 = comp._compose(torch.device(DEV), [torch.from_numpy(m) for m in c.masks], torch.from_numpy(c.sem)[:, None].to(DEV),
                               c.img_shape, *c.pad)
    for b in range(c.B):
        assert torch.equal(masks[b], m2[b]) and torch.equal(sem_cls[b], c2[b]) and torch.equal(sem_seg[b], s2[b])
    odd = vkn.GtPrep(3, 8, 11, dataset='cityscapes')
    out = odd.preprocess_gt_masks([dict(batch_input_shape=(33, 72), img_shape=(30, 61, 3))], [R.Bitmap(c.masks[0])],
                                  [torch.zeros(3, dtype=torch.int64, device=DEV)], None)
    assert odd.fused is False and out[0][0].is_cuda and tuple(out[0][0].shape) == (3, 11, 24)


# ------------------------------------------------------------------------------------------------------------------ integration
def _train_inputs(case, tg, stride):
    """raw ground truth for a training case of tests/test_gpu_train.py: byte masks and a Cityscapes-form map at `stride` times the
    assignment resolution; the thing labels are the case's"""
    rng = np.random.default_rng(3)
    Ht, Wt = case['H'] * case['up'] * stride, case['W'] * case['up'] * stride
    masks = [R.blobs(rng, len(e['gt_labels']), Ht - 3, Wt - 5) for e in tg]
    sem = R.sem_map(rng, case['B'], Ht, Wt, list(range(case['n_stuff'])) + [255])
    metas = [dict(batch_input_shape=(Ht, Wt), img_shape=(Ht - 3, Wt - 5, 3)) for _ in tg]
    return masks, sem, metas


def test_tail_step_adopts_the_bank_and_the_losses_are_the_compositions(vkn):
    """`TailStep.begin` on `GtPrep`'s tensors uses its bank (no copy); one `forward_train` on them gives bit for bit the losses it gives
    on the torch composition's tensors"""
    from oracle import synth
    from test_gpu_train import _train_case
    from video_k_net_amd.train_tail import TailStep
    g, case, head, (x, pf, mp, prev), (_, gt_labels, _, _) = _train_case(vkn, 'train_tiny')
    tg = synth.train_targets(case['B'], case['n_thing'], case['n_stuff'], case['H'] * case['up'], case['W'] * case['up'], case['seed'])
    masks, sem, metas = _train_inputs(case, tg, 2)

    def prepare(device):
        prep = vkn.GtPrep(2, case['n_thing'], case['n_stuff'], dataset='cityscapes')
        labels = [l.to(device) for l in gt_labels]
        out = prep.preprocess_gt_masks(metas, [R.Bitmap(m) for m in masks], labels, torch.from_numpy(sem)[:, None].to(device))
        return prep, out

    fused, (fm, fc, fs) = prepare(DEV)
    comp, (cm, cc, cs) = prepare('cpu')
    assert fused.fused is True and comp.fused is False and max(fused.n_sem) > 0
    cm, cc, cs = ([t.to(DEV) for t in ts] for ts in (cm, cc, cs))
    step = TailStep.begin(head, torch.device(DEV), fm, gt_labels, fs, fc)
    assert step is not None and step.bank.data_ptr() == fused.bank.data_ptr() and tuple(step.bank.shape) == tuple(fused.bank.shape)
    other = TailStep.begin(head, torch.device(DEV), cm, gt_labels, cs, cc)
    assert other.bank.data_ptr() not in [t.data_ptr() for t in cm] and torch.equal(other.bank, step.bank)
    assert step.gt_row0 == other.gt_row0 and step.sem_row0 == other.sem_row0 and step.n_sem == other.n_sem

    def losses(gm, gs, gc):
        head.zero_grad(set_to_none=True)
        out = head.forward_train(x.to(DEV), pf.to(DEV), mp.to(DEV), None, [dict() for _ in range(case['B'])], gm, gt_labels, gt_sem_seg=gs,
                                 gt_sem_cls=gc)
        return {k: v.detach().clone() for k, v in out.items()}
    la, lb = losses(fm, fs, fc), losses(cm, cs, cc)
    assert sorted(la) == sorted(lb) and any('loss' in k for k in la)
    for k in lb:
        assert torch.equal(la[k], lb[k]), (k, la[k], lb[k])


def test_match_indices_feed_the_tracking_loss(vkn):
    """`match_indices` handed to `match_loss_rows` reproduces the loss of the host-built list"""
    import track_loss_ref as T
    case = T.CASES['emb_cfg_full']()
    head = T.build_head(vkn, case.head).to(DEV)
    keys, refs = [], []
    for m in case.matches:
        n_ref = int(m.max()) + 2
        refs.append(torch.arange(n_ref, dtype=torch.int64) + 100)
        keys.append(torch.where(m >= 0, m + 100, torch.arange(len(m)) + 5000))
    prep = vkn.GtPrep(2, 2, 17)
    got = prep.match_indices([k.to(DEV) for k in keys], [r.to(DEV) for r in refs])
    for a, b in zip(got, case.matches):
        assert torch.equal(a.cpu(), b)
    args = [t.to(DEV) for t in (case.key, case.ref, case.key_gt, case.ref_gt)]
    la = head.match_loss_rows(*args, got)
    lb = head.match_loss_rows(*args, [m.to(DEV) for m in case.matches])
    assert sorted(la) == sorted(lb)
    for k in lb:
        assert torch.equal(la[k], lb[k])
