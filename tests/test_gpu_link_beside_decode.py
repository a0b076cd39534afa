"""GPU (-m gpu): the last decode on a workgroup budget and the head step that leaves CUs to the side-stream tracking link beside it
(VKN_FLAG_LINK_RESERVE / VKN_FLAG_LINK_NO_RESERVE).  Everything here is bit for bit: the split of a frame's pixels over workgroups
does not change the MFMA sequence an accumulator sees, and the reservation changes no kernel's operands."""
import pytest
import torch

from helpers import load_golden
from oracle import synth

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'


def _rand(shape, salt, std=1.0):
    return torch.from_numpy(synth.normalish(shape, salt, std))


@pytest.mark.parametrize('N,C', [(117, 256), (33, 256), (117, 64), (33, 64)], ids=lambda v: str(v))
def test_budgeted_decode_equals_default_decode_bit_for_bit(vkn, N, C):
    """B = 2; P = 2048 splits evenly, P = 2560 leaves a ragged last workgroup; 2, 3 and 5 workgroups in all (default: 8 and 10, spread
    over blockIdx.z on top); x stored as fp32 and as fp16."""
    B = 2
    k = _rand((B, N, C), 7102, 0.7).to(DEV)
    kb = _rand((B, N), 7103).to(DEV)
    hi, lo = vkn.ops.split_planes(k)
    for H, W in ((32, 64), (40, 64)):
        P = H * W
        x32 = _rand((B, C, H, W), 7101 + H).to(DEV)
        for x in (x32, x32.half()):
            ref = vkn.ops.mask_decode_planes(x, hi, lo, N, bias=kb)
            assert torch.equal(vkn.ops.mask_decode_planes_wg(x, hi, lo, N, 0, bias=kb), ref)
            for budget in (2, 3, 5):
                px = vkn.ops.decode_px_per_wg(B, P, budget)
                assert px > vkn.ops.decode_px_per_wg(B, P, 0) and B * -(-P // px) <= budget      # the budget does change the launch
                out = vkn.ops.mask_decode_planes_wg(x, hi, lo, N, budget, bias=kb)
                assert torch.equal(out, ref), (H, W, x.dtype, budget)


def _forced_budget(vkn, B, P):
    """VKN_FLAG_LINK_RESERVE: 3/4 of the default grid, at most 192 workgroups, at least one per frame (csrc/vkn_api.hip: link_reserve_wg)"""
    grid = B * -(-P // vkn.ops.decode_px_per_wg(B, P, 0))
    return max(B, min(192, grid * 3 // 4))


_HEAD = {}


def _head(vkn):
    """the config-width video head (N = 117, C = 256, x4) with the golden's weights, built once"""
    if not _HEAD:
        from helpers import make_case
        from test_host_logic import _cfg
        _, case = load_golden('video_cfg')
        assert (case['N'], case['C'], case['up']) == (117, 256, 4)
        head = vkn.build_head(_cfg(True, C=case['C'], heads=case['heads'], ffn=case['ffn'], ncls=case['ncls'], n_thing=case['n_thing'],
                                   n_stuff=case['n_stuff'], S=case['S'], up=case['up'], nprop=case['nprop']))
        head.load_state_dict(make_case(case)[1], strict=True)
        head = head.to(DEV).eval()
        _HEAD.update(head=head, packs=[h.stage_pack(torch.device(DEV)) for h in head.mask_head], N=case['N'], C=case['C'], up=case['up'])
    return _HEAD


def _inputs(vkn, B, H, W, salt):
    h = _head(vkn)
    N, C = h['N'], h['C']
    return dict(x=_rand((B, C, H, W), salt + 1).to(DEV), pf=_rand((B, N, C), salt + 2).to(DEV), mp=_rand((B, N, H, W), salt + 3, 4.0).to(DEV),
                first=_rand((1, N, C), salt + 4).to(DEV), prevs=_rand((B, N, C), salt + 5).to(DEV))


def _call(vkn, ins, clip, flags):
    h = _head(vkn)
    B, _, H, W = ins['x'].shape
    dims = h['head'].mask_head[0].make_dims(B, h['N'], H, W)
    return vkn.ops.head_forward(dims, h['packs'], ins['x'], ins['pf'], ins['mp'], None if clip else ins['prevs'], h['up'],
                                clip_first_prev=ins['first'] if clip else None, want_track=True, flags=flags), dims


def _decode_row_blocks(names):
    """NB (32-row blocks per workgroup) of the LOGITS decode kernels (template <NB, ABL, RING, BITS = 0, ...>) among the launched kernel
    names, mangled or not"""
    import re
    pat = re.compile(r'k_decode_mfma(?:ILi(\d+)ELi\d+ELi\d+ELi0E|<(\d+), *\d+, *\d+, *0,)')
    return {int(m.group(1) or m.group(2)) for n in names for m in pat.finditer(n)}


@pytest.mark.parametrize('B,H,W', [(2, 16, 32), (5, 16, 32), (6, 16, 32), (2, 32, 64)], ids=lambda v: str(v))
def test_head_step_with_reservation_equals_without_bit_for_bit(vkn, B, H, W):
    """16x32 features, N = 117, C = 256, x4: B = 2 few-row chain and link, B = 5 (19 row tiles) launch-per-GEMM chain and link, B = 6
    (22 row tiles) persistent chain; clip-link mode and an explicit previous-kernel tensor; with and without VKN_FLAG_JOIN_EARLY.
    The forced reservation must CHANGE the last decode's launch, or the comparison is of a launch sequence with itself: at 16x32 a
    frame is one 512-px workgroup, so the budget (one workgroup per frame) takes the row split over blockIdx.z away — the decode runs
    as 4-row-block workgroups instead of 1-row-block ones; at 32x64 (added for it) the pixel split itself changes, 512 -> 1024 px."""
    from helpers import run_and_kernels
    ops = vkn.ops
    P = H * W
    ins = _inputs(vkn, B, H, W, 7200 + B + H)
    budget = _forced_budget(vkn, B, P)
    if P == 512:
        assert budget == B and ops.decode_px_per_wg(B, P, budget) == ops.decode_px_per_wg(B, P, 0) == 512
    else:
        assert ops.decode_px_per_wg(B, P, budget) > ops.decode_px_per_wg(B, P, 0)
    (_, _), k_ref = run_and_kernels(lambda: _call(vkn, ins, True, ops.FLAG_LINK_NO_RESERVE))
    (_, _), k_out = run_and_kernels(lambda: _call(vkn, ins, True, ops.FLAG_LINK_RESERVE))
    assert _decode_row_blocks(k_ref) == {1} and _decode_row_blocks(k_out) == {4}, (k_ref, k_out)     # row split on / off
    for clip in (True, False):
        for early in (0, ops.FLAG_JOIN_EARLY):
            ref, _ = _call(vkn, ins, clip, ops.FLAG_LINK_NO_RESERVE | early)
            out, _ = _call(vkn, ins, clip, ops.FLAG_LINK_RESERVE | early)
            dflt, _ = _call(vkn, ins, clip, early)
            torch.cuda.synchronize()
            assert len(out) == 5 and all(t is not None for t in out)
            for name, u, v, w in zip(('object_feats', 'cls_score', 'mask_preds', 'scaled_mask_preds', 'track'), out, ref, dflt):
                assert torch.equal(u, v), (name, clip, early)
                assert torch.equal(w, v), (name, clip, early, 'default policy')


def test_reserved_head_step_is_ordered_on_the_callers_stream(vkn):
    """With the reservation forced (a budget that bites, see above): copies of `track` and `scaled_mask_preds` enqueued on the caller's
    stream right behind the call (no synchronisation) hold the final values; `track` is what track_link returns alone; a second call on
    the same workspace right behind the first gives what it gives with a synchronise in between."""
    ops = vkn.ops
    B, H, W = 5, 16, 32
    ins, ins2 = _inputs(vkn, B, H, W, 7300), _inputs(vkn, B, H, W, 7400)
    fl = ops.FLAG_LINK_RESERVE
    torch.cuda.synchronize()
    out, dims = _call(vkn, ins, True, fl)
    track_copy, scaled_copy = out[4].clone(), out[3].clone()      # enqueued behind the call, nothing waits in between
    second, _ = _call(vkn, ins2, True, fl)                        # same workspace, directly behind
    second_copy = [t.clone() for t in second]
    torch.cuda.synchronize()
    assert torch.equal(track_copy, out[4]) and torch.equal(scaled_copy, out[3])
    prevs = torch.cat([ins['first'], out[0][:-1]], 0)
    assert torch.equal(out[4], ops.track_link(dims, _head(vkn)['packs'][-1], out[0], prevs))
    first_sync, _ = _call(vkn, ins, True, fl)
    torch.cuda.synchronize()
    second_sync, _ = _call(vkn, ins2, True, fl)
    torch.cuda.synchronize()
    for u, v in zip(first_sync, out):
        assert torch.equal(u, v)
    for u, v, w in zip(second, second_sync, second_copy):
        assert torch.equal(u, v) and torch.equal(w, v)
