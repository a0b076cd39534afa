"""The references of the fused tracking loss (tests/track_loss_ref.py) checked on their own, without a GPU: the float64 restatement
against the reference's goldens and against the package's host path, the premises the GPU tests build on (mining active, an
unambiguous cut), and what the third part of the C ABI (include/vkn_track_train.h) promises before any launch."""
import ctypes

import numpy as np
import pytest
import torch

import track_loss_ref as R

E_ARG, E_SHAPE, E_WS, E_ALIGN = -1, -2, -3, -5


@pytest.mark.parametrize('name', ['emb_cfg', 'emb_one', 'emb_temp'])
def test_reference_reproduces_the_goldens(vkn, name):
    """Losses 1e-5 relative (the bound of tests/test_track_heads.py), targets and weights bit-exact, the kept mask equal to the host
    path's `topk` selection; the full-row form is the same computation."""
    g = np.load(R.GOLDEN)
    case = R.CASES[name + '_compact']()
    want = R.reference(case)
    for j, key in enumerate(('loss_track', 'loss_track_aux')):
        if f'{name}_{key}' in g.files:
            ref = float(g[f'{name}_{key}'])
            assert abs(want['losses'][j] - ref) < 1e-5 * max(1.0, abs(ref)), (key, want['losses'][j], ref)
        else:
            assert key == 'loss_track_aux' and want['losses'][j] == 0.0
    for i in range(2):
        assert np.array_equal(want['targets'][i], g[f'{name}_targets{i}']) and np.array_equal(want['weights'][i], g[f'{name}_weights{i}'])
    host = R.host_path(vkn, case)
    assert np.array_equal(want['kept'], host['kept'])
    full = R.reference(R.CASES[name + '_full']())
    assert np.allclose(full['losses'], want['losses'], rtol=1e-12, atol=0) and np.array_equal(full['stats'], want['stats'])


def test_premises_of_the_gpu_tests():
    """Mining is active in emb_cfg and emb_one; wherever a kept mask will be compared the cost gap at the cut is at least 1e-4 (the
    kernel's fp32 cosine differs from the float64 one by ~1e-7) and the cost at the cut is positive (ties among zero costs are arbitrary
    in the reference too, and carry zero loss and zero gradient)."""
    mined = {}
    for name in R.MASK_CASES:
        if name == 'capacity':
            continue                                   # its cut lies among zero costs: losses, stats and gradients are compared, not the mask
        want = R.reference(R.CASES[name]())
        mined[name] = [gap is not None for gap in want['cut_gap']]
        for gap, cut in zip(want['cut_gap'], want['cut_cost']):
            if gap is not None:
                assert gap >= R.MIN_GAP and cut > 0, (name, gap, cut)
    assert all(mined['emb_cfg_compact']) and all(mined['emb_one_compact']) and all(mined['emb_cfg_full'])
    assert mined['edge_above'] == [True] and mined['edge_at'] == [False] and mined['edge_below'] == [False]
    assert mined['no_mining'] == [False] and mined['ub_off'] == [False]


def test_edge_cases_hit_their_edges():
    s = {n: R.reference(R.CASES[n]())['stats'] for n in R.EDGE_CASES if n != 'capacity'}
    assert s['edge_at'].tolist() == [[1, 7, 1, 6]]                 # 6 / (1 + 1) == 3: not above the ratio, everything stays
    assert s['edge_above'].tolist() == [[2, 4, 1, 3]]              # 7 / 2 > 3: 1 * 3 negatives stay
    assert s['edge_below'].tolist() == [[3, 3, 2, 7]]
    assert s['no_partner'].tolist() == [[4, 3, 3, 9], [3, 4, 0, 0]]
    assert s['degenerate'][1].tolist() == [3, 1, 1, 2]
    assert s['one_by_one'].tolist() == [[1, 1, 1, 0]]
    assert s['ub_off'][0, 3] == 8 * 9 - s['ub_off'][0, 2] and s['ub_off'][0, 2] > 8      # more positives than rows: multi-positive rows


@pytest.mark.parametrize('name', [n for n in R.EDGE_CASES if n != 'capacity'])
def test_reference_agrees_with_the_host_path(vkn, name):
    """The float64 restatement and the package's fp32 host path: losses 1e-5, gradients 1e-4 of the largest magnitude, kept masks equal,
    NaN in the same places (the image without a partner)."""
    case = R.CASES[name]()
    for gout in R.GOUTS[:2]:
        want, host = R.reference(case, gout), R.host_path(vkn, case, gout)
        assert np.array_equal(np.isnan(want['losses']), np.isnan(host['losses']))
        ok = ~np.isnan(want['losses'])
        assert np.all(np.abs(host['losses'][ok] - want['losses'][ok]) < 1e-5 * np.maximum(1.0, np.abs(want['losses'][ok])))
        assert np.array_equal(want['kept'], host['kept'])
        for k in ('d_key', 'd_ref'):
            nan = np.isnan(want[k])
            assert np.array_equal(nan, np.isnan(host[k])), k
            assert R.rel_err(np.where(nan, 0, host[k]), np.where(nan, 0, want[k])) < 1e-4, k
    if name == 'no_partner':
        assert np.isnan(want['losses']).all() and np.isnan(want['d_key'][1]).any() and not np.isnan(want['d_key'][0]).any()


def test_clamp_passes_gradient_on_its_closed_interval():
    """What the backward restates: ATen's clamp_backward passes the gradient where min <= x <= max."""
    x = torch.tensor([-0.5, 0.0, 0.5, 1.0, 1.5], requires_grad=True)
    x.clamp(0, 1).sum().backward()
    assert x.grad.tolist() == [0.0, 1.0, 1.0, 1.0, 0.0]


def test_match_loss_without_a_device_is_the_host_path(vkn):
    """CPU tensors decline the fused path: `match_loss` is `loss(*match(...), *get_track_targets(...))`, value for value; a head whose
    mining draws from NumPy's RNG has no fused form at all."""
    case = R.CASES['emb_one_compact']()
    head = R.build_head(vkn, case.head)
    kidx, ridx, kres, rres, matches = R.sampling(case)
    ke = torch.cat([case.key[b, kidx[b]] for b in range(2)])
    re_ = torch.cat([case.ref[b, ridx[b]] for b in range(2)])
    got = head.match_loss(ke, re_, kres, rres, matches)
    want = head.loss(*head.match(ke, re_, kres, rres), *head.get_track_targets(matches, kres, rres))
    assert sorted(got) == sorted(want) == ['loss_track', 'loss_track_aux']
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert head.fused_loss_cfg() is not None and head.fused_loss_cfg().neg_pos_ub == 3
    aux = dict(case.head['loss_track_aux'], hard_mining=False)
    assert R.build_head(vkn, dict(case.head, loss_track_aux=aux)).fused_loss_cfg() is None
    assert R.build_head(vkn, dict(case.head, loss_track_aux=dict(aux, neg_pos_ub=-1))).fused_loss_cfg() is not None
    assert R.build_head(vkn, dict(case.head, loss_track_aux=None)).fused_loss_cfg().has_aux == 0
    with pytest.raises(vkn.VknLibraryError):
        vkn.TrackTrainTail(100, head)(torch.zeros(2, 100, 64), torch.zeros(2, 100, 64), [], [], [])


# ---------------------------------------------------------------------------------------------------- the ABI, before any launch
def test_track_loss_entries_refuse_before_any_launch(vkn):
    """NULL pointers, shapes outside the envelope, misaligned pointers and a short workspace are refused by the host-side checks, in this
    order, before a pointer is looked at (the fake pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    cap = vkn._lib.TRACK_LOSS_MAX_ROWS
    assert L.vkn_track_loss_workspace_bytes(2, cap) > 0 and L.vkn_track_loss_workspace_bytes(2, cap + 1) == 0
    assert L.vkn_track_loss_workspace_bytes(0, 8) == 0 and L.vkn_track_loss_workspace_bytes(65536, 8) == 0
    cfg = vkn.ops.track_loss_cfg(-1, True, 0.25, 1.0, 3, 0, 0.1)
    p = 0x10000
    big = 1 << 24

    def fwd(cfg_=cfg, key=p, ref=p, kgt=p, rgt=p, match=p, off=p, n_match=4, B=2, N=8, E=16, losses=p, stats=p, kept=None, status=p, ws=p,
            nws=big):
        return L.vkn_track_loss_fwd_f32(ctypes.byref(cfg_) if cfg_ is not None else None, key, ref, kgt, rgt, match, off, n_match, B, N, E,
                                        losses, stats, kept, status, ws, nws, None)

    def bwd(cfg_=cfg, key=p, ref=p, gout=p, B=2, N=8, E=16, dk=p, dr=p, ws=p, nws=big):
        return L.vkn_track_loss_bwd_f32(ctypes.byref(cfg_) if cfg_ is not None else None, key, ref, gout, B, N, E, dk, dr, ws, nws, None)

    for name in ('cfg_', 'key', 'ref', 'kgt', 'rgt', 'match', 'off', 'losses', 'stats', 'status'):
        assert fwd(**{name: None}) == E_ARG, name
    assert fwd(n_match=-1) == E_ARG
    for name in ('cfg_', 'key', 'ref', 'gout', 'dk', 'dr'):
        assert bwd(**{name: None}) == E_ARG, name
    for call in (fwd, bwd):
        assert call(N=cap + 1) == E_SHAPE and call(N=0) == E_SHAPE
        assert call(E=18) == E_SHAPE and call(E=1028) == E_SHAPE and call(E=0) == E_SHAPE
        assert call(B=65536) == E_SHAPE and call(B=0) == E_SHAPE
        assert call(ws=None) == E_WS and call(ws=p + 8) == E_WS and call(nws=L.vkn_track_loss_workspace_bytes(2, 8) - 1) == E_WS
    for name in ('key', 'ref', 'kgt', 'rgt', 'match', 'off', 'losses', 'stats'):
        assert fwd(**{name: p + 4}) == E_ALIGN, name
    assert fwd(status=p + 2) == E_ALIGN
    for name in ('key', 'ref', 'gout', 'dk', 'dr'):
        assert bwd(**{name: p + 4}) == E_ALIGN, name
