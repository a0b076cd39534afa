"""GPU: the joint panoptic merge (`vkn_panoptic_joint_f32`, csrc/vkn_panoptic.hip) pinned EXACTLY.

The other panoptic tests (test_gpu_parity.py, test_gpu_real_shapes.py, helpers.assert_pan_matches_oracle) feed blob-like masks with
continuous random scores and exempt near ties.  Here every input is built so that the float64 evaluation decides every pixel with a
margin of at least 1e-4 (pan_joint_ref.py; asserted on the CPU by test_pan_joint_refs.py), or ties exactly by duplication, and every
integer the library returns — the map, the six info columns (the score as bits), nseg, the boxes — is compared with `array_equal`
against pan_joint_ref.joint_ref: no near-tie rule, no slack on the counts.  What each group walks:
  geometry   pan_region / cap_of / the coefficient tables at two and three levels, up- and down-scaling, anisotropic, ragged last tiles,
             outputs under one tile, one-row and one-column logits (a capacity mistake is nseg = -1);
  dense      more than 32 and more than 64 live kernels in one tile: k_pan_argmax's survivor chunk loop and its short last batch;
  K = 300    the second trip of the `k += 256` loops;
  ties       (score descending, index ascending) in the selection and the merge order, first maximum in the arg-max (include/vkn.h);
  edges      the accept / reject tests of k_pan_merge at their thresholds."""
import ctypes

import numpy as np
import pytest
import torch

import pan_joint_ref as P

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _run(vkn, cases):
    """the frames `cases` (one geometry, one configuration) in one call -> numpy (seg [B,Ho,Wo], info [B,K,6], nseg [B], bbox [B,K,4])"""
    c = cases[0]
    m = c['meta']
    cls = torch.stack([x['cls'] for x in cases]).to(DEV)
    logits = torch.stack([x['logits'] for x in cases]).to(DEV)
    out = vkn.ops.panoptic_joint(cls, logits, c['Np'], c['T'], c['Kt'], c['inst_thr'], c['overlap_thr'], m['img_shape'][:2],
                                 m['batch_input_shape'], m['ori_shape'][:2], upsample_stride=c['up'], want_bbox=True)
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy() for t in out)


def _assert_frame(out, b, r):
    seg, info, nseg, bbox = (a[b] for a in out)
    assert int(nseg) >= 0, 'nseg = -1: the capacity alarm of k_pan_argmax'
    for col, name in enumerate(('sel_row', 'sel_label', 'seg_of', 'area', 'orig')):
        assert np.array_equal(info[:, col], r[name]), name
    assert np.array_equal(info[:, 5], r['sel_score'].view(np.int32)), 'score bits'
    assert int(nseg) == r['nseg']
    assert np.array_equal(seg, r['panoptic_seg'])
    assert np.array_equal(bbox, r['bbox'])


def _pin(vkn, name):
    case, r = P.get(name)
    out = _run(vkn, [case])
    _assert_frame(out, 0, r)
    return out, r


# ----------------------------------------------------------------------------------------------------------------------- a. geometry
@pytest.mark.parametrize('name', [n for n in P.SWEEP if not n.endswith('_b')])
def test_geometry_sweep(vkn, name):
    _pin(vkn, name)


@pytest.mark.parametrize('a,b', P.PAIRS)
def test_two_frames_in_one_call(vkn, a, b):
    """B = 2 with two different frames: frame b is the reference's frame b and, bit for bit, its own B = 1 run"""
    (ca, ra), (cb, rb) = P.get(a), P.get(b)
    both = _run(vkn, [ca, cb])
    _assert_frame(both, 0, ra)
    _assert_frame(both, 1, rb)
    for i, c in enumerate((ca, cb)):
        alone = _run(vkn, [c])
        assert all(np.array_equal(x[i], y[0]) for x, y in zip(both, alone))


# ------------------------------------------------------------------------------------------------- b. survivor chunks, f. determinism
@pytest.mark.parametrize('name', list(P.DENSE))
def test_survivor_chunks(vkn, name):
    """>= 33 (K = 60) and >= 65 (K = 117) kernels are live in one tile (test_pan_joint_refs.py::test_dense_cases_fill_more_than_one_chunk),
    and the run twice gives the same bits"""
    out, _ = _pin(vkn, name)
    again = _run(vkn, [P.get(name)[0]])
    assert all(np.array_equal(x, y) for x, y in zip(out, again))


# ------------------------------------------------------------------------------------------------------------------------ c. K > 256
def test_more_than_256_kernels(vkn):
    out, r = _pin(vkn, 'k300')
    info = out[1][0]
    late = info[256:]
    assert int(((late[:, 2] > 0) & (late[:, 3] > 0) & (late[:, 1] < 3)).sum()) >= 1      # accepted thing winners behind entry 256
    assert int(((late[:, 2] > 0) & (late[:, 3] > 0) & (late[:, 1] >= 3)).sum()) >= 1     # and stuff ones


# --------------------------------------------------------------------------------------------------------------------------- d. ties
def test_tie_same_mask_row_in_two_classes(vkn):
    """bit-equal scores of proposal 1 in classes 0 and 1: class 0 is listed first and wins every pixel of the shared mask; the second
    entry has area 0, orig 80 and is rejected without a segment id"""
    out, _ = _pin(vkn, 'tie_same_row')
    info = out[1][0]
    assert info[1:3, :5].tolist() == [[1, 0, 2, 80, 80], [1, 1, 0, 0, 80]] and info[1, 5] == info[2, 5]
    assert out[3][0][2].tolist() == list(P.EMPTY_BOX)


def test_tie_identical_stuff_planes(vkn):
    """stuff rows with bit-identical planes and bit-equal scores: the lower row comes first in the selection and wins"""
    out, _ = _pin(vkn, 'tie_stuff_planes')
    info = out[1][0]
    assert info[2:4, :5].tolist() == [[3, 3, 2, 256, 256], [4, 4, 0, 0, 256]]


def test_tie_equal_scores_on_different_planes(vkn):
    """only the order is at stake: selection by flat index, segment ids in (score, entry) order across things and stuff"""
    out, _ = _pin(vkn, 'tie_scores')
    info = out[1][0]
    assert info[:, 0].tolist() == [2, 0, 1, 4, 3, 5, 6] and info[:, 2].tolist() == [1, 3, 4, 2, 5, 6, 7]


def test_tie_all_scores_zero(vkn):
    """every product is 0.0: entry 0 wins every pixel; it is a thing below the threshold, so the map is empty"""
    out, _ = _pin(vkn, 'zero_scores')
    seg, info, nseg, bbox = (a[0] for a in out)
    assert info[:, 3].tolist() == [16 * 64, 0, 0, 0, 0] and int(nseg) == 0 and not seg.any() and not info[:, 2].any()


# ---------------------------------------------------------------------------------------------------------------- e. threshold edges
def test_threshold_edges(vkn):
    """pan_joint_ref.EDGE_THINGS / EDGE_STUFF, entries in selection order (I X A E C D H F G | S background):
      score    F at exactly 0.25f is kept, G one fp32 step below is rejected; the background stuff at 0.01 is kept (things only);
      overlap  C keeps 6 of its 10 pixels: kept at overlap_thr = 0.6; D keeps 5 of 10: rejected, its 5 pixels are 0 in the map;
      orig 0   X wins 36 pixels at prob 0.27 where everything else is at -30: rejected, pixels 0, empty box;
      area 0   H lies under I: rejected, no segment id consumed;
      ids      1..7 over the accepted entries in score order, things and stuff interleaved."""
    out, _ = _pin(vkn, 'edges')
    seg, info, nseg, bbox = (a[0] for a in out)
    assert info[:, 3].tolist() == P.EDGE_AREA == [27, 36, 19, 10, 6, 5, 0, 8, 5, 160, 1644]
    assert info[:, 4].tolist() == P.EDGE_ORIG == [27, 0, 19, 10, 10, 10, 5, 8, 5, 160, 1884]
    assert info[:, 2].tolist() == [1, 0, 2, 4, 5, 0, 0, 6, 0, 3, 7] and int(nseg) == 7
    assert not seg[20:23, 66:78].any() and not seg[5, 2:7].any() and not seg[8, 70:75].any() and int((seg == 0).sum()) == 46
    assert (seg[8, 60:68] == 6).all() and (seg[2, 21:27] == 5).all() and (seg[18, 2:7] == 1).all()
    assert bbox[1].tolist() == bbox[5].tolist() == bbox[6].tolist() == bbox[8].tolist() == list(P.EMPTY_BOX)
    assert bbox[7].tolist() == [60, 8, 67, 8] and bbox[10].tolist() == [0, 0, 79, 23]


def test_overlap_threshold_is_compared_in_fp64(vkn):
    """the same frame with overlap_thr = float(float32(0.6)) = 0.60000002...: 6 / 10 is now below it, C goes and the ids close up —
    the compare is the fp64 one, on the value passed"""
    out, _ = _pin(vkn, 'edges_f32_thr')
    assert out[1][0][:, 2].tolist() == [1, 0, 2, 4, 0, 0, 0, 5, 0, 3, 6] and int(out[2][0]) == 6
    assert int((out[0][0] == 0).sum()) == 46 + 6


# ------------------------------------------------------------------------------------------------------------- fewer than four kernels
@pytest.mark.parametrize('K', [1, 2, 3])
def test_fewer_than_four_kernels(vkn, K):
    """K below one batch of four: the survivor chunk is still one batch long (it was 0 — K / 4 * 4 — and the chunk loop never advanced)"""
    out, _ = _pin(vkn, f'few_{K}')
    assert out[1][0][:, 2].tolist() == list(range(1, K + 1))


# ------------------------------------------------------------------------------------------------------------------ f. capacity gate
def test_footprint_past_lds_is_refused_before_any_output(vkn):
    """512 x 512 logits resized to a 16 x 64 output: one tile's footprint cannot fit LDS.  VKN_E_SHAPE, raised by ops, and — through the
    raw entry point with prefilled outputs — nothing written."""
    Np, T, nstuff, H = 2, 2, 2, 512
    cls = torch.rand(1, Np + nstuff, T + nstuff, generator=torch.Generator().manual_seed(0)).to(DEV)
    logits = torch.zeros(1, Np + nstuff, H, H, device=DEV)
    with pytest.raises(vkn._lib.VknError) as e:
        vkn.ops.panoptic_joint(cls, logits, Np, T, Np, 0.25, 0.6, (H, H), (H, H), (16, 64), want_bbox=True)
    assert e.value.code == -2
    L = vkn._lib.lib()
    K = Np + nstuff
    cfg = vkn._lib.VknPanopticCfg(Np, T, Np, 0.25, 0.6, 1, H, H, H, H, H, H, 16, 64)
    outs = [torch.full(s, 0x5a5a5a5a, dtype=torch.int32, device=DEV) for s in ((1, 16, 64), (1, K, 6), (1,), (1, K, 4))]
    nb = int(L.vkn_panoptic_workspace_bytes(ctypes.byref(cfg), 1, Np + nstuff))
    ws = torch.zeros(max(nb, 256), dtype=torch.uint8, device=DEV)
    p = lambda t: ctypes.c_void_p(t.data_ptr())          # noqa: E731
    code = L.vkn_panoptic_joint_f32(ctypes.byref(cfg), p(cls), p(logits), 1, Np + nstuff, T + nstuff, *(p(o) for o in outs), p(ws), nb,
                                    ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert code == -2
    assert all(bool((o == 0x5a5a5a5a).all()) for o in outs)
