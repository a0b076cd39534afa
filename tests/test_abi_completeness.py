"""CPU: every entry point of the six headers that WRITES through a pointer has a named place where its outputs are guarded — the table
that drives tests/test_gpu_abi_contract.py (`ENTRIES`) or `GUARDED_ELSEWHERE` below.  A new entry point cannot be added without
deciding where its guards are.  The two entries that write HOST memory are guarded here, in a CPU arena."""
import ctypes
import os
import re

import numpy as np
import torch

from abi_arena import Arena

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# entry point -> the test module that calls it (through the C ABI or its one-to-one binding) with sentinel-filled memory around its outputs
GUARDED_ELSEWHERE = {
    **{e: 'tests/test_gpu_chain_blocks.py' for e in (
        'vkn_linear_dw_f32', 'vkn_linear_dw_batch_f32', 'vkn_layernorm_act_fwd_f32', 'vkn_layernorm_act_bwd_f32', 'vkn_updator_gate_product_f32',
        'vkn_updator_gate_product_bwd_f32', 'vkn_updator_mix_fwd_f32', 'vkn_updator_mix_bwd_f32', 'vkn_attention_f32', 'vkn_attention_bwd_f32')},
    **{e: 'tests/test_gpu_track_tail.py' for e in ('vkn_track_boxes_f32', 'vkn_track_maps_i32', 'vkn_qd_tracker_match_dev_f32')},
    **{e: 'tests/test_gpu_track_loss.py' for e in ('vkn_track_loss_fwd_f32', 'vkn_track_loss_bwd_f32')},
    **{e: 'tests/test_gpu_seg_tail.py' for e in ('vkn_seg_targets_u8', 'vkn_seg_loss_fwd_f32', 'vkn_seg_loss_bwd_f32')},
    'vkn_gt_bank_fill_f32': 'tests/test_gpu_gt_prep.py',
    'vkn_lsap_f32': 'tests/test_abi_completeness.py',
    'vkn_qd_tracker_state_layout': 'tests/test_abi_completeness.py',
}


def _writing_entries(vkn):
    """{entry point: its non-`const` pointer parameters, and the non-`const` pointer members of the structs it takes} over `ABI_HEADERS` + `EXTENSION_HEADERS`: the functions are the ones `_lib`
    parsed out of the headers; `const` is read from the header text (the binding does not keep it).  `stream` (a hipStream_t passed as
    void*) is no output."""
    lib = vkn._lib
    out = {}
    texts = {h: re.sub(r'/\*.*?\*/', ' ', open(hdr.path).read(), flags=re.S) for table in (lib.ABI, lib.ABI_EXT) for h, hdr in table.items()}
    # structs with a member the library may write through (`float* dW` of VknDwItem ...): an entry that takes one, even as a `const` array,
    # writes through a pointer as well
    carriers = {}
    for text in texts.values():
        for body, name in re.findall(r'typedef\s+struct\s+\w*\s*\{([^{}]*)\}\s*(\w+)\s*;', text):
            members = [m.strip().lstrip('*').strip() for d in body.split(';') if '*' in d and not re.search(r'\bconst\b', d)
                       for m in re.sub(r'^[\w\s]*?(?=\*)', '', d.strip()).split(',')]
            if members:
                carriers[name] = members
    assert {'VknDwItem', 'VknSplitItem', 'VknAssignProblem', 'VknLsapProblem', 'VknAdamwItem', 'VknUpdatorNormGrads'} <= set(carriers), carriers
    assert 'VknStageWeights' not in carriers and 'VknGtImage' not in carriers and carriers['VknDwItem'] == ['dW', 'db']
    for table in (lib.ABI, lib.ABI_EXT):
        for h, hdr in table.items():
            text = texts[h]
            declared = dict(re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text))
            assert set(declared) == set(hdr.symbols), h
            for name in hdr.symbols:
                params = [q.strip() for q in declared[name].split(',')]
                writes = [q.split()[-1].lstrip('*') for q in params if '*' in q and not re.search(r'\bconst\b', q.split('*')[0])]
                writes = [w for w in writes if w != 'stream']
                writes += [f'{q.split()[-1].lstrip("*")}->{m}' for q in params for c, ms in carriers.items() if re.search(rf'\b{c}\b', q) for m in ms]
                if writes:
                    out[name] = writes
    return out


def test_every_writing_entry_point_has_its_guards_somewhere(vkn):
    from test_gpu_abi_contract import ENTRIES
    writing = _writing_entries(vkn)
    assert len(writing) > 85 and {'vkn_linear_dw_batch_f32', 'vkn_split_weights_batch_f32', 'vkn_assign_costs_batch_f32'} <= set(writing) and writing['vkn_mask_gather_f32'] == ['xraw_out', 'cnt_out', 'ws'] and 'vkn_gather_workspace_bytes' not in writing
    assert tuple(vkn._lib.ABI) + tuple(vkn._lib.ABI_EXT) == ('vkn.h', 'vkn_track.h', 'vkn_track_train.h', 'vkn_gt.h', 'vkn_decode.h', 'vkn_seg_loss.h')
    absent = sorted(set(writing) - set(ENTRIES) - set(GUARDED_ELSEWHERE))
    assert not absent, f'entry points that write through a pointer and are guarded nowhere: {absent}'
    twice = sorted(set(ENTRIES) & set(GUARDED_ELSEWHERE))
    assert not twice, twice
    declared = {s for t in (vkn._lib.ABI, vkn._lib.ABI_EXT) for h in t.values() for s in h.symbols}
    assert set(ENTRIES) <= declared and set(GUARDED_ELSEWHERE) <= declared       # (no stale names)
    contract = open(os.path.join(ROOT, 'tests', 'test_gpu_abi_contract.py')).read()
    for entry, test in ENTRIES.items():
        assert re.search(rf'^def {test}\(', contract, flags=re.M), (entry, test)
        assert re.search(rf'\bL\.{entry}\(', contract), f'{entry}: never called through the raw library in tests/test_gpu_abi_contract.py'
    for entry, path in GUARDED_ELSEWHERE.items():
        full = os.path.join(ROOT, path)
        assert os.path.isfile(full), (entry, path)
        text = open(full).read()
        binding = entry[4:].rsplit('_', 1)[0]                # vkn_gt_bank_fill_f32 -> gt_bank_fill: the one-to-one binding in ops.py
        assert re.search(rf'\b{entry}\b', text) or re.search(rf'\bops\.{binding}\b', text), f'{path} does not mention {entry}'


def test_host_outputs_of_exactly_their_size(vkn):
    """vkn_lsap_f32 writes min(nr, nc) pairs into HOST arrays, vkn_qd_tracker_state_layout twelve offsets: both in a CPU arena"""
    from scipy.optimize import linear_sum_assignment
    L = vkn._lib.lib()
    rng = np.random.default_rng(3)
    for nr, nc in ((1, 1), (5, 3), (3, 5), (64, 65), (65, 64)):
        cost = np.ascontiguousarray(rng.integers(0, 4, (nr, nc)).astype(np.float32))
        before = cost.copy()
        A = Arena('cpu')
        k = min(nr, nc)
        r, c = A.out((k,), torch.int32, name='row_ind'), A.out((k,), torch.int32, name='col_ind')
        assert L.vkn_lsap_f32(cost.ctypes.data, nr, nc, r.ptr, c.ptr) == k
        A.check(f'lsap {nr}x{nc}')
        sr, sc = linear_sum_assignment(cost)
        assert np.array_equal(r.t.numpy(), sr) and np.array_equal(c.t.numpy(), sc) and np.array_equal(cost, before)
    from test_gpu_tracker import CFG
    trk = vkn.build_tracker(dict(CFG, type='QuasiDenseEmbedTracker', max_dets=16, max_tracklets=8))
    cfg = trk._make_cfg(32)
    A = Arena('cpu')
    off = A.out((12,), torch.int64, name='offsets12')
    assert L.vkn_qd_tracker_state_layout(ctypes.byref(cfg), ctypes.cast(off.ptr, ctypes.POINTER(ctypes.c_size_t))) == 0
    A.check('state layout')
    o = off.t.tolist()
    assert o == sorted(o) and o[0] == 0 and o[-1] < L.vkn_qd_tracker_state_bytes(ctypes.byref(cfg))
