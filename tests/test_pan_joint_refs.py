"""CPU: the premises of tests/test_gpu_pan_joint_pins.py.  The GPU tests compare the joint panoptic merge with pan_joint_ref.joint_ref
by `array_equal`, which is only fair if (1) joint_ref IS the oracle that tests/golden pins to the reference, with the tie rules written
out, and (2) the float64 evaluation decides every pixel of every case with room to spare (FLOOR = 1e-4 on the arg-max margin and on
|prob - 0.5|: a condition on the INPUTS, asserted here, not a tolerance on the kernel).  Also here: the survivor counts that make the
dense cases walk k_pan_argmax's chunk loop, and the pixel counts the crisp cases are built to have."""
import numpy as np
import pytest
import torch

import pan_joint_ref as P
from oracle.knet_oracle import panoptic_joint as oracle_panoptic_joint


def _oracle_agrees(case, r, dtype):
    with torch.no_grad():
        o = oracle_panoptic_joint(case['cls'].to(dtype), case['logits'].to(dtype), case['Np'], case['T'], case['Kt'], case['inst_thr'],
                                  case['overlap_thr'], case['meta'], upsample_stride=case['up'])
    assert np.array_equal(o['panoptic_seg'].numpy(), r['panoptic_seg'])
    assert np.array_equal(o['rows'].numpy(), r['sel_row']) and np.array_equal(o['total_labels'].numpy(), r['sel_label'])
    assert np.array_equal(o['total_scores'].float().numpy(), r['sel_score'])
    assert np.array_equal(o['seg_of'].numpy(), r['seg_of'])
    assert np.array_equal(o['area'].numpy(), r['area']) and np.array_equal(o['orig'].numpy(), r['orig'])
    assert len(o['segments_info']) == r['nseg']


@pytest.mark.parametrize('name', list(P.SWEEP))
def test_joint_ref_is_the_oracle_in_float64(name):
    """tie-free inputs, both in float64: every integer the two produce is the same"""
    case, r = P.get(name)
    _oracle_agrees(case, r, torch.float64)


@pytest.mark.parametrize('name', P.FLOORED)
def test_cases_are_decided(name):
    """both float64 minima reach FLOOR, and the fp32 oracle arrives at the float64 integers"""
    case, r = P.get(name)
    print(f'[pan_joint_ref] {name}: K = {r["sel_row"].size}, margin = {r["margin"]:.3e}, half_margin = {r["half_margin"]:.3e}')
    assert r['margin'] >= P.FLOOR and r['half_margin'] >= P.FLOOR
    _oracle_agrees(case, r, torch.float32)


@pytest.mark.parametrize('name', ['tie_same_row', 'tie_stuff_planes', 'tie_scores', 'few_1', 'few_2', 'few_3'])
def test_tie_cases_are_decided_outside_their_duplicates(name):
    """constructed duplicates (bit-equal score and plane) are bitwise equal in any arithmetic; everything else keeps the floor"""
    _, r = P.get(name)
    assert r['margin'] >= P.FLOOR and r['half_margin'] >= P.FLOOR


@pytest.mark.parametrize('name', list(P.SWEEP))
def test_sweep_cases_accept_and_reject(name):
    _, r = P.get(name)
    assert int((r['seg_of'] > 0).sum()) >= 1
    assert int(((r['seg_of'] == 0) & (r['area'] > 0)).sum()) >= 1          # a rejected winner: its pixels become 0 in the map
    assert int(r['area'].sum()) == r['ids'].size


def test_sweep_geometries_take_the_arms_they_are_named_for():
    for geom, (Hm, Wm, up, bis, img, ori) in P.GEOMS.items():
        assert img[0] <= bis[0] and img[1] <= bis[1], geom
    three = {g for g, (Hm, Wm, up, bis, img, ori) in P.GEOMS.items() if tuple(img) != tuple(ori)}
    assert three == {'three_levels_up', 'down_under_a_tile', 'anisotropic', 'ragged_1', 'ragged_63_15'}
    Hm, Wm, up, bis, _, _ = P.GEOMS['level1_down']
    assert up * Hm == 2 * bis[0] and up * Wm == 2 * bis[1]
    assert {g: (o[0] % P.TILE_H, o[1] % P.TILE_W) for g, (_, _, _, _, _, o) in P.GEOMS.items() if g.startswith('ragged')} == \
        {'ragged_1': (1, 1), 'ragged_63_15': (15, 63)}
    for a, b in P.PAIRS:
        assert P.SWEEP[a][:2] == P.SWEEP[b][:2] and P.SWEEP[a][2] != P.SWEEP[b][2]
        assert not np.array_equal(P.get(a)[1]['panoptic_seg'], P.get(b)[1]['panoptic_seg'])


def test_dense_cases_fill_more_than_one_chunk():
    """k_pan_argmax stages at most 32 survivors per chunk, four per batch: >= 33 live kernels in a tile walk a second chunk, >= 65 a
    third, and a count that is no multiple of 4 ends on a short batch"""
    best = {}
    for name, spec in P.DENSE.items():
        live = P.live_lower_bound(P.get(name)[0])
        print(f'[pan_joint_ref] {name}: live kernels per tile (lower bound) = {live.tolist()}')
        assert int(live.max()) >= spec[-1]
        best[name] = live
    assert best['dense_k60'].max() >= 33 and best['dense_k117'].max() >= 65
    assert any(int(v) % 4 != 0 and int(v) >= 33 for live in best.values() for v in live.reshape(-1))


def test_k300_case_has_late_winners():
    case, r = P.get('k300')
    assert r['sel_row'].size == 300
    assert int(np.bincount(r['sel_row']).max()) == 3                                     # a row selected in all three classes
    late = (np.arange(300) >= 256) & (r['seg_of'] > 0) & (r['area'] > 0)
    assert int((late & (r['sel_label'] < case['T'])).sum()) >= 1 and int((late & (r['sel_label'] >= case['T'])).sum()) >= 1
    assert np.unique(r['sel_score']).size == 300                                         # no ties


def test_edge_case_counts():
    """the pixel counts tests/test_gpu_pan_joint_pins.py::test_threshold_edges states, from the rectangles alone"""
    _, r = P.get('edges')
    assert r['area'].tolist() == P.EDGE_AREA and r['orig'].tolist() == P.EDGE_ORIG and r['seg_of'].tolist() == P.EDGE_SEG
    assert r['sel_row'].tolist() == [7, 8, 0, 3, 1, 2, 6, 4, 5, 10, 9]
    assert r['sel_score'][7] == np.float32(0.25) and r['sel_score'][8] < np.float32(0.25)
    assert r['sel_score'][8] == np.nextafter(np.float32(0.25), np.float32(0))
    assert 6 / 10 >= 0.6 and 6 / 10 < float(np.float32(0.6))
    _, r32 = P.get('edges_f32_thr')
    assert r32['seg_of'].tolist() == P.EDGE_SEG_F32_THR and r32['area'].tolist() == P.EDGE_AREA
    assert r['bbox'][1].tolist() == list(P.EMPTY_BOX) and r['bbox'][7].tolist() == [60, 8, 67, 8]
    assert int((r['panoptic_seg'] == 0).sum()) == 36 + 5 + 5                             # X's hole, D's and G's own pixels


def test_tie_case_answers():
    _, r = P.get('tie_same_row')             # entries: 0 = (row 0, class 1) .9; 1, 2 = (row 1, class 0), (row 1, class 1) .7; 3 = row 2; 4 = stuff
    assert r['sel_row'].tolist() == [0, 1, 1, 2, 3] and r['sel_label'].tolist() == [1, 0, 1, 0, 2]
    assert r['area'].tolist()[1:3] == [80, 0] and r['orig'].tolist()[1:3] == [80, 80] and r['seg_of'].tolist() == [1, 2, 0, 3, 4]
    _, r = P.get('tie_stuff_planes')         # entries 2, 3 = mask rows 3, 4 (.6, the same plane), 4 = background
    assert r['sel_row'].tolist() == [0, 1, 3, 4, 2] and r['area'].tolist()[2:4] == [256, 0] and r['orig'].tolist()[2:4] == [256, 256]
    assert r['seg_of'].tolist() == [1, 3, 2, 0, 4]
    _, r = P.get('tie_scores')               # things .8 (row 2), .6 (row 0, class 1), .6 (row 1, class 0); stuff .8 (row 4), .6 (rows 3, 5)
    assert r['sel_row'].tolist() == [2, 0, 1, 4, 3, 5, 6] and r['sel_label'].tolist() == [0, 1, 0, 3, 2, 4, 5]   # (entry 6: the background)
    assert r['seg_of'].tolist() == [1, 3, 4, 2, 5, 6, 7] and (r['area'][:6] == r['orig'][:6]).all()
    _, r = P.get('zero_scores')
    assert r['sel_row'].tolist() == [0, 0, 1, 2, 3] and r['sel_label'].tolist() == [0, 1, 0, 2, 3]
    assert r['area'].tolist() == [16 * 64, 0, 0, 0, 0] and r['nseg'] == 0 and not r['panoptic_seg'].any()
    assert (r['bbox'] == np.array(P.EMPTY_BOX)).all()
