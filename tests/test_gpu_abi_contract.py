"""GPU: the BUFFER contract of the C ABI (include/vkn.h "Conventions"): the library allocates nothing, scratch is the caller's `ws` of
exactly `vkn_*_workspace_bytes` bytes, a `ws` that is too small or NULL is VKN_E_WORKSPACE, every output is caller memory of exactly the
stated shape, every input is `const`.

Every entry point of `ENTRIES` is called through `vkn._lib.lib()` (raw ctypes, never `ops.*`: `ops._workspace` only grows and
`torch.empty` rounds its blocks up, so the binding hides a kernel that writes a row past its output or a size query that under-reports by
a tile).  Outputs and workspaces are carved out of a sentinel-filled arena (tests/abi_arena.py; its detection is proven on the CPU by
tests/test_abi_arena.py) at their exact sizes between guards, inputs are frozen, and after the call
  * every output word was written, nothing outside the outputs and the workspace was, no input changed,
  * the values are right: the LINEAR kernels bit for bit against the float64 references of tests/exact_cases.py (premise and
    non-vacuity checks on); every other entry bit for bit against the same call on plain `torch` buffers with a roomy workspace — the
    form the value tests of the suite pin against the goldens, the oracles and float64 (every entry documents that it is deterministic)
    — and, where a test owns an importable rule, against that rule (helpers.assert_pan_matches_oracle, test_gpu_semantic_fpn._rule, scipy).
The gates (`test_gate_*`): `ws_bytes = need - 1` and `ws = NULL` return VKN_E_WORKSPACE, a misaligned `ws` / output returns what the
entry's code says, before anything is launched — the sentinel-filled outputs stay untouched.  The only constants of this module are the
arena's guard sizes."""
import ctypes
import os

import numpy as np
import pytest
import torch

import exact_cases as ec
from abi_arena import SENT, Arena, frozen

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
OK, E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = 0, -1, -2, -3, -5

# entry point -> the test of this module that guards it (tests/test_abi_completeness.py reads this table)
ENTRIES = {
    'vkn_workspace_init': 'test_head_goldens', 'vkn_workspace_status': 'test_head_goldens',
    'vkn_mask_gather_f32': 'test_mask_gather', 'vkn_mask_gather_real_f32': 'test_mask_gather',
    'vkn_mask_decode_f32': 'test_mask_decode', 'vkn_mask_decode_scaled_f32': 'test_mask_decode', 'vkn_split_planes_f32': 'test_mask_decode',
    'vkn_mask_decode_planes_f32': 'test_mask_decode', 'vkn_mask_decode_planes_x': 'test_mask_decode',
    'vkn_mask_decode_planes_wg_f32': 'test_decode_on_a_workgroup_budget', 'vkn_mask_decode_planes_wg_x': 'test_decode_on_a_workgroup_budget',
    'vkn_decode_gather_f32': 'test_decode_gather', 'vkn_decode_gather_x': 'test_decode_gather',
    'vkn_upsample_bilinear_f32': 'test_upsample', 'vkn_upsample_bilinear_f16out': 'test_upsample', 'vkn_upsample_bilinear_bwd_f32': 'test_upsample',
    'vkn_split_weight_f32': 'test_linear', 'vkn_split_weight_t_f32': 'test_linear', 'vkn_split_weights_batch_f32': 'test_linear',
    'vkn_linear_f32': 'test_linear',
    'vkn_conv_prepare_f32': 'test_conv_gn', 'vkn_conv_gn_f32': 'test_conv_gn',
    'vkn_kernel_init_f32': 'test_kernel_init',
    'vkn_prepare_stage_f32': 'test_head_goldens', 'vkn_head_forward_f32': 'test_head_goldens', 'vkn_head_forward_link_f32': 'test_head_link_golden',
    'vkn_head_forward_prof_f32': 'test_head_goldens', 'vkn_stage_forward_link_f32': 'test_head_link_golden',
    'vkn_stage_forward_f32': 'test_stage_entries', 'vkn_track_link_f32': 'test_stage_entries', 'vkn_track_link_flags_f32': 'test_stage_entries',
    'vkn_stage_chain_f32': 'test_stage_entries', 'vkn_kernel_updator_f32': 'test_stage_entries',
    'vkn_link_block_f32': 'test_link_block', 'vkn_query_merge_f32': 'test_query_merge',
    'vkn_panoptic_joint_f32': 'test_panoptic_joint',
    'vkn_assign_costs_f32': 'test_assign_costs', 'vkn_assign_costs_batch_f32': 'test_assign_costs',
    'vkn_assign_costs_lowres_batch_f32': 'test_assign_costs_lowres', 'vkn_lsap_batch_f32': 'test_lsap_batch',
    'vkn_stage_targets': 'test_loss_tail', 'vkn_focal_loss_f32': 'test_loss_tail', 'vkn_mask_losses_fwd_lowres_f32': 'test_loss_tail',
    'vkn_mask_losses_fwd_bank_f32': 'test_loss_tail', 'vkn_stage_losses_final_f32': 'test_loss_tail',
    'vkn_mask_losses_bwd_lowres_f32': 'test_loss_tail', 'vkn_mask_losses_bwd_bank_f32': 'test_loss_tail',
    'vkn_mask_losses_fwd_f32': 'test_loss_tail', 'vkn_mask_losses_bwd_f32': 'test_loss_tail',
    'vkn_scale_by_f32': 'test_loss_tail', 'vkn_sum_n_f32': 'test_loss_tail', 'vkn_sgd_momentum_f32': 'test_loss_tail',
    'vkn_qd_tracker_reset': 'test_qd_tracker', 'vkn_qd_tracker_match_f32': 'test_qd_tracker',
    'vkn_localization_fpn_f32': 'test_localization_fpn',
    'vkn_pow2_scale_f32': 'test_backward_glue', 'vkn_scale_pad_rows_f32': 'test_backward_glue', 'vkn_transpose_pad_f32': 'test_backward_glue',
    'vkn_threshold_rows_f16': 'test_backward_glue', 'vkn_unscale_rows_f32': 'test_backward_glue', 'vkn_check_range_i64': 'test_backward_glue',
    'vkn_gt_classes': 'test_gt_classes', 'vkn_gt_match_indices': 'test_gt_match_indices',
    'vkn_panoptic_thing_first_u8': 'test_thing_first_merge', 'vkn_adamw_flat_f32': 'test_adamw_flat',
}
WS_BYTES = {}      # entry point -> the workspace sizes its size query answered at the tested shapes (_workspace_report)


@pytest.fixture(scope='module', autouse=True)
def _workspace_report():
    """when the module's tests are over: the workspace sizes the size queries answered at the shapes that ran, per entry point (smallest,
    largest, number of distinct sizes), recorded with the parity margins (helpers.record_margins prints each line and keeps the file)"""
    yield
    from helpers import record_margins
    for k, v in sorted(WS_BYTES.items()):
        record_margins(f'abi_contract_ws_bytes[{k}]', dict(min=min(v), max=max(v), distinct=len(v)))


def _lib(vkn):
    return vkn._lib.lib()


def p(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def st():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def _cuda(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


def _ws(entry, need):
    WS_BYTES.setdefault(entry, set()).add(int(need))
    return int(need)


def _bits_equal(name, got, want):
    a, b = got.contiguous().reshape(-1).view(torch.uint8), want.contiguous().reshape(-1).view(torch.uint8)
    assert got.shape == want.shape and got.dtype == want.dtype, (name, got.shape, want.shape)
    if not torch.equal(a, b):
        bad = (got.reshape(-1) != want.reshape(-1)).nonzero().reshape(-1)
        raise AssertionError(f'{name}: {int(bad.numel())} of {got.numel()} elements differ from the same call on plain buffers, first at {bad[:4].tolist()}')


def _exact(name, got, want):
    """`got` (a view of the arena) equals the float64 reference bit for bit: tests/test_gpu_exact.py's own comparison"""
    from test_gpu_exact import _diff
    return _diff(name, got, want)


def _close64(name, got, ref64, mag64, roundings):
    """an element-wise fp32 formula against its float64 value: every fp32 operation (and every constant handed over as fp32) rounds once,
    by at most 2^-24 of a partial result no larger than `mag64`, the sum of the |terms| (default |ref64|): |got - ref64| <= roundings
    2^-24 mag64.  The bound follows from the formula alone, not from a measurement."""
    mag64 = ref64.abs() if mag64 is None else mag64
    excess = (got.double().reshape(ref64.shape) - ref64).abs() - roundings * 2.0 ** -24 * mag64
    assert float(excess.max()) <= 0.0, f'{name}: off the float64 formula by {float(excess.max()):.3e} beyond {roundings} fp32 roundings'


class Call:
    """One entry point on plain buffers and in the arena.  `outs`: {name: (shape, dtype) | (shape, dtype, opts) | None (a NULL output)};
    `fn(o, ws, ws_bytes)` makes the call with `o[name]` the output pointers and returns its code; `inputs`: the tensors it reads.
    `header`: a stage-shaped entry — the 256-byte header is cleared with vkn_workspace_init, and afterwards vkn_workspace_status is VKN_OK
    and bytes 4..255 of the header are still zero (kernels "only ever OR into the first word").  Every other entry gets `ws` at offset 0
    of its range (no `+256` of the binding: the contract is the C one)."""

    def __init__(self, vkn, entry, name, outs, need, fn, inputs=(), header=False, pre=None, ws_align=256, compare=True):
        L = _lib(vkn)
        self.name = name
        need = _ws(entry, need) if need is not None else 0
        specs = {k: (v if len(v) == 3 else (v[0], v[1], {})) for k, v in outs.items() if v is not None}
        # ---- plain buffers: zero-filled outputs, a workspace with room to spare
        plain = {k: torch.zeros(sh, dtype=dt, device=DEV) for k, (sh, dt, _) in specs.items()}
        wsb = torch.zeros(need + 4096, dtype=torch.uint8, device=DEV)
        if pre is not None:
            pre(plain)
        rc = fn({k: p(plain.get(k)) for k in outs}, p(wsb) if need else None, wsb.numel() if need else 0)
        assert rc == OK, (name, 'plain buffers', rc)
        torch.cuda.synchronize()
        # ---- the arena: exact sizes, guards, frozen inputs
        A = Arena(DEV)
        rng = {k: A.out(sh, dt, name=k, **opts) for k, (sh, dt, opts) in specs.items()}
        w = A.ws(need, name='ws', align=ws_align) if need else None
        if pre is not None:
            pre({k: r.t for k, r in rng.items()})
        if header:
            assert L.vkn_workspace_init(w.ptr, need, st()) == OK
        with frozen(*inputs):
            rc = fn({k: (rng[k].ptr if k in rng else None) for k in outs}, w.ptr if need else None, need)
        assert rc == OK, (name, 'arena', rc)
        A.check(name)                                        # (synchronises the device: a side stream of the library's has finished too)
        if header:
            assert L.vkn_workspace_status(w.ptr, need, st()) == OK, name
            assert int(w.bytes[4:256].count_nonzero()) == 0, f'{name}: bytes 4..255 of the workspace header were written'
            A.check(name + ' after vkn_workspace_status')
        self.out = {k: r.t for k, r in rng.items()}
        self.plain, self.arena = plain, A
        if compare:
            for k, (_, _, opts) in specs.items():
                if opts.get('full', True):                    # (an output the entry may fill in part keeps the arena's sentinel elsewhere)
                    _bits_equal(f'{name} {k}', self.out[k], plain[k])


def _untouched(A, name):
    """nothing at all was written into the arena (a call refused by its host-side gate)"""
    torch.cuda.synchronize()
    A._materialise()
    assert bool((A.words == SENT).all()), f'{name}: a refused call wrote into the caller\'s memory'


# ====================================================================================================== linear kernels: gather
SWEEP = [s for s in ec.bncp_sweep(large=False) if (s.C == 256 and s.H * s.W in (1, 62, 66, 135)) or s.C == 32]
REF_KERNELS = 1


def test_the_sweep_subset_covers_what_it_promises():
    assert {s.N for s in SWEEP if s.C == 256} == set(ec.N_EDGES) and {s.B for s in SWEEP} == set(ec.B_ALL) and {s.C for s in SWEEP} == {32, 256}
    for P in (1, 62, 66, 135):
        assert {s.N for s in SWEEP if s.C == 256 and s.H * s.W == P} == set(ec.N_EDGES)


def test_mask_gather(vkn):
    """vkn_mask_gather_f32 with the MFMA and the reference kernels, cnt_out given and NULL (the count then lives in the workspace), and
    vkn_mask_gather_real_f32 with asum_out given and NULL"""
    L = _lib(vkn)
    fails = []
    for s in SWEEP:
        B, N, C, P, tag = s.B, s.N, s.C, s.H * s.W, ec.sid(s)
        x, z, xraw, cnt = ec.gather_case(s)
        xd, zd = _cuda(x, z)
        need = L.vkn_gather_workspace_bytes(B, N, C, P)
        assert need > 0
        for flags in (0, REF_KERNELS):
            for with_cnt in (True, False):
                c = Call(vkn, 'vkn_mask_gather_f32', f'gather flags={flags} cnt={with_cnt} {tag}',
                         dict(xraw=((B, N, C), torch.float32), cnt=((B, N), torch.float32) if with_cnt else None), need,
                         lambda o, ws, nb: L.vkn_mask_gather_f32(p(xd), p(zd), ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, flags, st()),
                         inputs=(xd, zd))
                fails.append(_exact(f'{c.name} xraw[b, n, c]', c.out['xraw'], xraw))
                if with_cnt:
                    fails.append(_exact(f'{c.name} cnt[b, n]', c.out['cnt'], cnt))
        x, a, out, asum = ec.gather_real_case(s, 16)
        xd, ad = _cuda(x, a)
        for with_sum in (True, False):
            c = Call(vkn, 'vkn_mask_gather_real_f32', f'gather_real asum={with_sum} {tag}',
                     dict(out=((B, N, C), torch.float32), asum=((B, N), torch.float32) if with_sum else None), need,
                     lambda o, ws, nb: L.vkn_mask_gather_real_f32(p(xd), p(ad), o['out'], o['asum'], B, N, C, P, ws, nb, st()), inputs=(xd, ad))
            fails.append(_exact(f'{c.name} out[b, n, c]', c.out['out'], out))
            if with_sum:
                fails.append(_exact(f'{c.name} asum[b, n]', c.out['asum'], asum))
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


# ====================================================================================================== decode
def _planes(vkn, kd, B, N, C, tag):
    """vkn_split_planes_f32 into planes of exactly [B][roundup(N, 32)][C] fp16: (hi, lo) views of the arena, kept alive by the caller"""
    L = _lib(vkn)
    npt = (N + 31) // 32 * 32
    c = Call(vkn, 'vkn_split_planes_f32', f'split_planes {tag}', dict(hi=((B, npt, C), torch.float16), lo=((B, npt, C), torch.float16)), None,
             lambda o, ws, nb: L.vkn_split_planes_f32(p(kd), o['hi'], o['lo'], B, N, C, st()), inputs=(kd,))
    return c


def test_mask_decode(vkn):
    """vkn_mask_decode_f32 (odd P takes the reference-kernel arm), bias given and NULL, with the reference kernels; the scaled decode;
    vkn_split_planes_f32 into exact-size planes and vkn_mask_decode_planes_f32 / _x from them (declined at odd P: nothing written)"""
    L = _lib(vkn)
    fails, odd, even = [], 0, 0
    for s in SWEEP:
        B, N, C, P, tag = s.B, s.N, s.C, s.H * s.W, ec.sid(s)
        x, k, kb, out = ec.decode_case(s)
        xd, kd, kbd = _cuda(x, k, kb)
        nobias = out - kb.double()[..., None, None]
        need = L.vkn_decode_workspace_bytes(B, N, C)
        assert need > 0
        shape = dict(out=((B, N, s.H, s.W), torch.float32))
        for flags in (0, REF_KERNELS):
            for bias, want in ((kbd, out), (None, nobias)):
                c = Call(vkn, 'vkn_mask_decode_f32', f'decode flags={flags} bias={bias is not None} {tag}', shape, need,
                         lambda o, ws, nb: L.vkn_mask_decode_f32(p(xd), p(kd), p(bias), o['out'], B, N, C, P, ws, nb, flags, st()),
                         inputs=(xd, kd, bias))
                fails.append(_exact(f'{c.name} [b, n, y, x]', c.out['out'], want))
        pl = _planes(vkn, kd, B, N, C, tag)
        hi, lo = pl.out['hi'], pl.out['lo']
        fails.append(_exact(f'split_planes hi {tag} [b, n, c]', hi[:, :N].float(), k.double()))
        assert int(lo.count_nonzero()) == 0 and int(hi[:, N:].count_nonzero()) == 0, f'split_planes {tag}: lo / padding rows not exactly zero'
        sc = torch.tensor(2.0 ** -7, device=DEV)
        if P % 2 == 0:
            even += 1
            c = Call(vkn, 'vkn_mask_decode_scaled_f32', f'decode scaled 2^-7 {tag}', shape, need,
                     lambda o, ws, nb: L.vkn_mask_decode_scaled_f32(p(xd), p(kd), p(kbd), p(sc), o['out'], B, N, C, P, ws, nb, 0, st()),
                     inputs=(xd, kd, kbd, sc))
            fails.append(_exact(f'{c.name} [b, n, y, x]', c.out['out'], out * 2.0 ** -7))
            for bias, want in ((kbd, out), (None, nobias)):
                c = Call(vkn, 'vkn_mask_decode_planes_f32', f'decode planes bias={bias is not None} {tag}', shape, None,
                         lambda o, ws, nb: L.vkn_mask_decode_planes_f32(p(xd), p(hi), p(lo), p(bias), o['out'], B, N, C, P, st()),
                         inputs=(xd, hi, lo, bias))
                fails.append(_exact(f'{c.name} [b, n, y, x]', c.out['out'], want))
            c = Call(vkn, 'vkn_mask_decode_planes_x', f'decode planes_x {tag}', shape, None,
                     lambda o, ws, nb: L.vkn_mask_decode_planes_x(p(xd), 0, p(hi), p(lo), p(kbd), o['out'], B, N, C, P, st()),
                     inputs=(xd, hi, lo, kbd))
            fails.append(_exact(f'{c.name} [b, n, y, x]', c.out['out'], out))
        else:
            odd += 1
            A = Arena(DEV)
            o, w = A.out((B, N, s.H, s.W), name='out'), A.ws(need, name='ws')
            assert L.vkn_mask_decode_planes_f32(p(xd), p(hi), p(lo), p(kbd), o.ptr, B, N, C, P, st()) == E_SHAPE, tag
            assert L.vkn_mask_decode_scaled_f32(p(xd), p(kd), p(kbd), p(sc), o.ptr, B, N, C, P, w.ptr, need, 0, st()) == E_SHAPE, tag
            _untouched(A, f'declined decodes at odd P {tag}')
        pl.arena.check(f'planes of {tag} after the decodes that read them')
    assert odd > 0 and even > 0
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


@pytest.mark.parametrize('budget', [3, 5, 0])
def test_decode_on_a_workgroup_budget(vkn, budget):
    """vkn_mask_decode_planes_wg_f32 / _x at P = 2560 on 3 and 5 workgroups: the pixel split leaves a ragged last workgroup
    (vkn_decode_px_per_wg does not divide P), which must stop at the end of `out`"""
    L = _lib(vkn)
    fails, ragged = [], 0
    for s in (ec.Shape(1, 33, 64, 40, 64, 2301, False), ec.Shape(2, 117, 256, 40, 64, 2302, False)):
        B, N, C, P, tag = s.B, s.N, s.C, s.H * s.W, ec.sid(s)
        assert P == 2560
        px = L.vkn_decode_px_per_wg(B, P, budget)
        assert px > 0
        assert B * ((P + px - 1) // px) <= max(budget, B) or not budget
        ragged += P % px != 0
        x, k, kb, out = ec.decode_case(s)
        xd, kd, kbd = _cuda(x, k, kb)
        pl = _planes(vkn, kd, B, N, C, tag)
        hi, lo = pl.out['hi'], pl.out['lo']
        shape = dict(out=((B, N, s.H, s.W), torch.float32))
        c = Call(vkn, 'vkn_mask_decode_planes_wg_f32', f'decode planes_wg budget={budget} {tag}', shape, None,
                 lambda o, ws, nb: L.vkn_mask_decode_planes_wg_f32(p(xd), p(hi), p(lo), p(kbd), o['out'], B, N, C, P, budget, st()),
                 inputs=(xd, hi, lo, kbd))
        fails.append(_exact(f'{c.name} [b, n, y, x]', c.out['out'], out))
        c = Call(vkn, 'vkn_mask_decode_planes_wg_x', f'decode planes_wg_x budget={budget} {tag}', shape, None,
                 lambda o, ws, nb: L.vkn_mask_decode_planes_wg_x(p(xd), 0, p(hi), p(lo), None, o['out'], B, N, C, P, budget, st()),
                 inputs=(xd, hi, lo))
        fails.append(_exact(f'{c.name} [b, n, y, x]', c.out['out'], out - kb.double()[..., None, None]))
    assert ragged or not budget, 'the budget leaves no ragged last workgroup at either shape'   # (3: 1024 px at B = 1; 5: 1536 px at B = 2)
    fails = [f for f in fails if f]
    assert not fails, '\n'.join(fails)


# ====================================================================================================== the fused pass
FUSED = [s for s in ec.bncp_sweep(large=False) if s.C in (64, 256) and s.H * s.W in (64, 128) and s.N in (1, 33, 117, 256)]


def test_decode_gather(vkn):
    """vkn_decode_gather_f32 / _x at P in {64, 128}, C in {64, 256}, N in {1, 33, 117, 256} (cnt_out is not optional there), bias given and NULL"""
    L = _lib(vkn)
    assert {(s.C, s.H * s.W, s.N) for s in FUSED} == {(C, P, N) for C in (64, 256) for P in (64, 128) for N in (1, 33, 117, 256)}
    fails = []
    for s in FUSED:
        B, N, C, P, tag = s.B, s.N, s.C, s.H * s.W, ec.sid(s)
        assert L.vkn_decode_gather_supported(C, P)
        x, k, kb, z, xraw, cnt = ec.fused_case(s)
        xd, kd, kbd = _cuda(x, k, kb)
        pl = _planes(vkn, kd, B, N, C, tag)
        hi, lo = pl.out['hi'], pl.out['lo']
        need = L.vkn_gather_workspace_bytes(B, N, C, P)
        outs = dict(xraw=((B, N, C), torch.float32), cnt=((B, N), torch.float32))
        c = Call(vkn, 'vkn_decode_gather_f32', f'fused {tag}', outs, need,
                 lambda o, ws, nb: L.vkn_decode_gather_f32(p(xd), p(hi), p(lo), p(kbd), ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, st()),
                 inputs=(xd, hi, lo, kbd))
        fails += [_exact(f'{c.name} xraw[b, n, c]', c.out['xraw'], xraw), _exact(f'{c.name} cnt[b, n]', c.out['cnt'], cnt)]
        c = Call(vkn, 'vkn_decode_gather_f32', f'fused nobias {tag}', outs, need,
                 lambda o, ws, nb: L.vkn_decode_gather_f32(p(xd), p(hi), p(lo), None, ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, st()),
                 inputs=(xd, hi, lo))
        c = Call(vkn, 'vkn_decode_gather_x', f'fused_x {tag}', dict(xraw=((B, N, C), torch.float32), cnt=((B, N), torch.float32)), need,
                 lambda o, ws, nb: L.vkn_decode_gather_x(p(xd), 0, p(hi), p(lo), p(kbd), ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, st()),
                 inputs=(xd, hi, lo, kbd))
        fails += [_exact(f'{c.name} xraw[b, n, c]', c.out['xraw'], xraw), _exact(f'{c.name} cnt[b, n]', c.out['cnt'], cnt)]
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


# ====================================================================================================== up-scaling
UP_HW = ((1, 1), (3, 5), (9, 15), (8, 16))
UP_PLANES = (1, 7, 33)


def test_upsample(vkn):
    """vkn_upsample_bilinear_f32 (staged and generic kernels), _f16out (also into an output that is 8-byte but not 16-byte aligned: the
    header asks for 8) and the adjoint at S = 1, 2, 3, 4, 8, on 1, 7 and 33 planes"""
    L = _lib(vkn)
    fails, seed = [], 2400
    for (H, W) in UP_HW:
        for planes in UP_PLANES:
            for S in (2, 4):
                seed += 1
                m, out = ec.up_case(1, planes, H, W, S, seed, f16=True)
                md = m.to(DEV)
                tag = f'x{S} {planes} planes of {H}x{W}'
                c = Call(vkn, 'vkn_upsample_bilinear_f32', f'up {tag}', dict(out=((1, planes, H * S, W * S), torch.float32)), None,
                         lambda o, ws, nb: L.vkn_upsample_bilinear_f32(p(md), o['out'], planes, H, W, S, st()), inputs=(md,))
                fails.append(_exact(f'{c.name} [_, plane, y, x]', c.out['out'], out))
                for skew in (0, 8):
                    spec = dict(out=((1, planes, H * S, W * S), torch.float16, dict(skew=skew)))
                    call = lambda o, ws, nb: L.vkn_upsample_bilinear_f16out(p(md), o['out'], planes, H, W, S, st())  # noqa: E731
                    if (W * S) % 4 == 0:
                        c = Call(vkn, 'vkn_upsample_bilinear_f16out', f'up f16 +{skew} {tag}', spec, None, call, inputs=(md,))
                        fails.append(_exact(f'{c.name} [_, plane, y, x]', c.out['out'], out))
                    else:
                        A = Arena(DEV)
                        o = A.out((1, planes, H * S, W * S), torch.float16, name='out', skew=skew)
                        assert call(dict(out=o.ptr), None, 0) == E_SHAPE, tag
                        _untouched(A, f'up f16 declined {tag}')
            for S in (1, 2, 3, 4, 8):
                seed += 1
                go, gin = ec.up_bwd_case(1, planes, H, W, S, seed)
                gd = go.to(DEV)
                c = Call(vkn, 'vkn_upsample_bilinear_bwd_f32', f'up_bwd x{S} {planes} planes of {H}x{W}', dict(gin=((1, planes, H, W), torch.float32)),
                         None, lambda o, ws, nb: L.vkn_upsample_bilinear_bwd_f32(p(gd), o['gin'], planes, H, W, S, st()), inputs=(gd,))
                if S != 3:                                   # (weights k / 6 are not dyadic: x3 stays with the plain-buffer run, which
                    fails.append(_exact(f'{c.name} [_, plane, y, x]', c.out['gin'], gin))     # tests/test_gpu_train.py pins to autograd)
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


# ====================================================================================================== GEMM engine
def test_linear(vkn):
    """vkn_linear_f32 (exact-fp32 MFMA and on the bf16x3 images of vkn_split_weight_f32, images of exactly 6 roundup(Nout, 256) K bytes)
    over gemm_shapes(); with ksplit > 1 the workspace is exactly ksplit M Nout 4 bytes — the header's figure, there is no size query"""
    L = _lib(vkn)
    fails, split = [], 0
    for i, (M, K, Nout) in enumerate(ec.gemm_shapes()):
        act = i % 2
        A_, W, b, y = ec.linear_case(M, K, Nout, 1100 + i, act=act)      # (the cases of tests/test_gpu_exact.py)
        Ad, Wd, bd = _cuda(A_, W, b)
        tag = f'M{M} K{K} N{Nout} act{act}'
        img = Call(vkn, 'vkn_split_weight_f32', f'split_weight {tag}', dict(img=((6 * ((Nout + 255) // 256 * 256) * K,), torch.uint8, dict(full=False))), None,
                   lambda o, ws, nb: L.vkn_split_weight_f32(p(Wd), o['img'], Nout, K, st()), inputs=(Wd,))
        imgd = img.out['img']
        forms = [('exact', None, 1), ('bf16x3', imgd, 1)]
        if Nout <= 256 and K > 256:
            ks = 8 if K >= 1024 else K // 256
            forms += [(f'exact ksplit{ks}', None, ks), (f'bf16x3 ksplit{ks}', imgd, ks)]
        if Nout <= 512:                                     # the images of the TRANSPOSE of a stored [K][Nout] matrix stand for the same W
            Wt = Wd.t().contiguous()
            imgt = Call(vkn, 'vkn_split_weight_t_f32', f'split_weight_t {tag}', dict(img=((6 * ((Nout + 255) // 256 * 256) * K,), torch.uint8, dict(full=False))),
                        None, lambda o, ws, nb: L.vkn_split_weight_t_f32(p(Wt), o['img'], Nout, K, st()), inputs=(Wt,))
            _bits_equal(f'split_weight_t {tag} against the images of W itself', imgt.out['img'], imgd)
            nimg = imgd.numel()

            def both(o, ws, nb):                            # W as stored and its transpose as two items of ONE launch
                items = (vkn._lib.VknSplitItem * 2)(vkn._lib.VknSplitItem(Wd.data_ptr(), o['a'].value, K, 1, Nout, K, K, 0),
                                                    vkn._lib.VknSplitItem(Wt.data_ptr(), o['b'].value, 1, Nout, Nout, K, K, 0))
                return L.vkn_split_weights_batch_f32(items, 2, st())
            ib = Call(vkn, 'vkn_split_weights_batch_f32', f'split_weights_batch {tag}',
                      dict(a=((nimg,), torch.uint8, dict(full=False)), b=((nimg,), torch.uint8, dict(full=False))), None, both, inputs=(Wd, Wt))
            _bits_equal(f'split_weights_batch {tag} item 0', ib.out['a'], imgd)
            _bits_equal(f'split_weights_batch {tag} item 1', ib.out['b'], imgd)
        for form, wsplit, ks in forms:
            need = ks * M * Nout * 4 if ks > 1 else None
            split += ks > 1
            c = Call(vkn, 'vkn_linear_f32', f'linear {form} {tag}', dict(y=((M, Nout), torch.float32)), need,
                     lambda o, ws, nb: L.vkn_linear_f32(p(Ad), p(Wd), p(wsplit), p(bd), o['y'], M, K, Nout, act, ks, ws, nb, st()),
                     inputs=(Ad, Wd, bd, wsplit))
            fails.append(_exact(f'{c.name} y[m, n]', c.out['y'], y))
        img.arena.check(f'weight images of {tag} after the GEMMs that read them')
    assert split >= 4
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


# ====================================================================================================== FPN conv
CONV = [(B, C, H, W, ks, stride, mode) for (H, W) in ((1, 1), (3, 5), (12, 39)) for ks in (1, 3) for stride in (1, 2) for mode in ('raw', 'pos')
        for (B, C) in (((2, 32),) if (H + ks + stride) % 2 else ((1, 256),))] + [(1, 256, 3, 5, 3, 1, 'raw'), (2, 32, 12, 39, 3, 2, 'pos')]


def test_conv_gn(vkn):
    """vkn_conv_prepare_f32 into an image of exactly vkn_conv_weight_bytes; vkn_conv_gn_f32 raw and with pos, k in {1, 3}, stride in
    {1, 2}: the raw output exact, its statistics (guarded too) bit-identical to the plain-buffer run, the 256-byte header kept"""
    L = _lib(vkn)
    assert {c[1] for c in CONV} == {32, 256}
    fails = []
    for i, (B, C, H, W, ks, stride, mode) in enumerate(CONV):
        x, pos, w, out = ec.conv_case(B, C, H, W, ks, stride, mode, 2600 + i)
        xd, pd, wd = _cuda(x, pos, w)
        tag = f'conv B{B} C{C} {H}x{W} k{ks} s{stride} {mode}'
        nimg = L.vkn_conv_weight_bytes(C, C, ks)
        assert nimg > 0
        img = Call(vkn, 'vkn_conv_prepare_f32', f'conv_prepare {tag}', dict(img=((nimg,), torch.uint8, dict(full=False))), None,
                   lambda o, ws, nb: L.vkn_conv_prepare_f32(p(wd), C, C, ks, o['img'], nimg, st()), inputs=(wd,))
        imgd = img.out['img']
        A = Arena(DEV)
        small = A.out((nimg - 1,), torch.uint8, name='img')
        assert L.vkn_conv_prepare_f32(p(wd), C, C, ks, small.ptr, nimg - 1, st()) == E_WORKSPACE
        _untouched(A, f'conv_prepare into a short image {tag}')
        Ho, Wo = (H - 1) // stride + 1, (W - 1) // stride + 1
        need = L.vkn_conv_gn_workspace_bytes(B, C, H, W, stride, 0)
        outs = dict(out=((B, C, Ho, Wo), torch.float32), stats=((B, 32, 2), torch.float32))
        call = lambda o, ws, nb: L.vkn_conv_gn_f32(p(xd), p(pd), None, None, None, 0, 0, p(imgd), ks, stride, 32, o['out'], o['stats'],  # noqa: E731
                                                   B, C, H, W, C, ws, nb, st())
        if ks == 1 and stride == 2:                         # outside the envelope (no shipped config has a strided 1x1 conv)
            A = Arena(DEV)
            o, s_, w_ = A.out((B, C, Ho, Wo), name='out'), A.out((B, 32, 2), name='stats'), A.ws(max(need, 256), name='ws')
            assert call(dict(out=o.ptr, stats=s_.ptr), w_.ptr, w_.nbytes) == E_SHAPE, tag
            _untouched(A, tag)
            continue
        assert need > 256
        c = Call(vkn, 'vkn_conv_gn_f32', tag, outs, need, call, inputs=(xd, pd, imgd), header=True)
        fails.append(_exact(f'{tag} [b, c, y, x]', c.out['out'], out))
        assert bool(torch.isfinite(c.out['stats']).all())
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


# ====================================================================================================== kernel-init pass
def _one_pass(Np, ncls, C, P):
    """csrc/vkn_init.hip: vkn_init_pass_supported, restated (it is not part of the C ABI)"""
    if C % 16 or C > 256 or P % 64 or C * P * 4 >= 1 << 31:
        return False
    nbl, slo, shi = (Np + 31) // 32, Np // 32, (Np + ncls - 1) // 32
    return (nbl, slo, shi) in ((4, 3, 3), (1, 0, 0))


@pytest.mark.parametrize('with_obj', [0, 1, 2])
@pytest.mark.parametrize('cat', [0, 1], ids=['nocat', 'cat'])
@pytest.mark.parametrize('separate', [0, 1], ids=['onepass', 'separate'])
def test_kernel_init(vkn, separate, cat, with_obj):
    """vkn_kernel_init_f32 as tests/test_gpu_exact.py::test_kernel_init builds it: one-pass and VKN_FLAG_INIT_SEPARATE, seg_preds given
    and NULL (then kept in the workspace), cat_stuff 0 / 1, with_obj 0 / 1 / 2, at shapes the one-pass kernel takes and shapes it leaves
    to the separate form; the workspace is exactly vkn_kernel_init_workspace_bytes"""
    L = _lib(vkn)
    flags = vkn._lib.CONSTS['VKN_FLAG_INIT_SEPARATE'] if separate else 0
    assert {_one_pass(sh[2], sh[3], sh[1], sh[5] * sh[6]) for sh in ec.INIT_SHAPES} == {True, False}
    fails = []
    for i, sh in enumerate(ec.INIT_SHAPES):
        B, C, Np, ncls, nth, H, W = sh
        P = H * W
        loc, sem, iw, sw, sb, ref = ec.init_case(*sh, 1400 + i, bool(cat))
        ld, sd, iwd, swd, sbd = _cuda(loc, sem, iw, sw, sb)
        N = Np + (ncls - nth if cat else 0)
        need = L.vkn_kernel_init_workspace_bytes(B, Np, ncls, C, P)
        assert need > 0
        for with_seg in (True, False):
            tag = f'init {sh} cat={cat} with_obj={with_obj} separate={separate} seg={with_seg}'
            outs = dict(x_feats=((B, C, H, W), torch.float32), mask_preds=((B, N, H, W), torch.float32),
                        seg_preds=((B, ncls, H, W), torch.float32) if with_seg else None, prop=((B, N, C), torch.float32))
            c = Call(vkn, 'vkn_kernel_init_f32', tag, outs, need,
                     lambda o, ws, nb: L.vkn_kernel_init_f32(p(ld), p(sd), p(iwd), p(swd), p(sbd), nth, cat, with_obj, ec.THR, o['x_feats'],
                                                             o['mask_preds'], o['seg_preds'], o['prop'], B, Np, ncls, C, P, ws, nb, flags, st()),
                     inputs=(ld, sd, iwd, swd, sbd))
            fails += [_exact(f'{tag} x_feats[b, c, y, x]', c.out['x_feats'], ref['x_feats']),
                      _exact(f'{tag} mask_preds[b, n, y, x]', c.out['mask_preds'], ref['mask_preds'])]
            if with_seg:
                fails.append(_exact(f'{tag} seg_preds[b, n, y, x]', c.out['seg_preds'], ref['seg_preds']))
            if with_obj == 1:
                fails.append(_exact(f'{tag} proposal_feats[b, n, c]', c.out['prop'], ref['prop']))
            elif with_obj == 0:                              # proposal_feats_with_obj off: the kernels themselves
                want = torch.cat([iw.double()[None].expand(B, -1, -1), ref['prop'][:, Np:]], 1)
                fails.append(_exact(f'{tag} proposal_feats[b, n, c]', c.out['prop'], want))
            elif cat:                                        # soft weights are not linear; the stuff rows are copies whatever the weights
                fails.append(_exact(f'{tag} proposal_feats[b, Np:, c]', c.out['prop'][:, Np:], ref['prop'][:, Np:]))
    fails = [f for f in fails if f]
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:20])


# ====================================================================================================== stage-shaped entries
def _prepared(vkn, dims, packs, tag):
    """the weights of `packs` (ops.StagePack) with `prepared` images of exactly vkn_prepared_bytes each, built by vkn_prepare_stage_f32
    in an arena: -> (array of VknStageWeights, the arenas: checked again after the calls that read the images)"""
    L = _lib(vkn)
    W = vkn._lib.VknStageWeights
    arr, arenas = (W * len(packs))(), []
    for i, pk in enumerate(packs):
        w = W.from_buffer_copy(pk.w)
        w.prepared, w.prepared_bytes = None, 0
        nb = L.vkn_prepared_bytes(ctypes.byref(dims), ctypes.byref(w))
        if nb:
            A = Arena(DEV)
            r = A.ws(_ws('vkn_prepare_stage_f32', nb), name=f'prepared{i}')
            assert r.addr % 256 == 0
            short = Arena(DEV)
            rs = short.ws(nb - 1, name='short')
            assert L.vkn_prepare_stage_f32(ctypes.byref(dims), ctypes.byref(w), rs.ptr, nb - 1, st()) == E_WORKSPACE
            _untouched(short, f'{tag}: vkn_prepare_stage_f32 into a short buffer')
            assert L.vkn_prepare_stage_f32(ctypes.byref(dims), ctypes.byref(w), r.ptr, nb, st()) == OK
            A.check(f'{tag}: prepared images of stage {i}')
            w.prepared, w.prepared_bytes = r.addr, nb
            arenas.append((A, r, r.bytes.clone()))
        arr[i] = w
    return arr, arenas


def _prepared_unchanged(arenas, tag):
    for A, r, before in arenas:
        A.check(f'{tag}: prepared images after the calls that read them')
        assert torch.equal(r.bytes, before), f'{tag}: the prepared images (const) were modified'


HEAD_FLAGS = dict(mfma=0, refkernels=1, exactgemm=2, allexact=3, persistent=512, persistent_ref=513, launches=256, ksplit=8192,
                  persistent_bf16x3=512 + 65536)          # every flag of tests/test_gpu_parity.py::test_head_vs_reference_golden
HEAD_CASES = [(n, f) for n in ('det_tiny', 'det_odd', 'video_tiny') for f in HEAD_FLAGS] + \
             [('video_cfg', f) for f in ('persistent', 'persistent_bf16x3', 'ksplit', 'launches')]


def _head_of(vkn, name):
    from helpers import load_golden
    from test_gpu_parity import _build_head
    g, case = load_golden(name)
    head, (x, pf, mp, prev) = _build_head(vkn, case)
    return g, case, head, _cuda(x, pf, mp, prev)


@pytest.mark.parametrize('name,form', HEAD_CASES, ids=[f'{n}-{f}' for n, f in HEAD_CASES])
def test_head_goldens(vkn, name, form):
    """vkn_head_forward_f32 on the goldens at every flag of test_head_vs_reference_golden, video goldens with the tracking link on the
    library's side stream and with VKN_FLAG_SERIAL_LINK: workspace of exactly vkn_head_workspace_bytes behind a cleared header, prepared
    images of exactly vkn_prepared_bytes; bit-identical to `head._head_forward` under the same flags — the call that test pins against the
    reference's own outputs"""
    L = _lib(vkn)
    flags = HEAD_FLAGS[form]
    g, case, head, (xd, pfd, mpd, prevd) = _head_of(vkn, name)
    B, N, C, H, W, up, ncls = case['B'], case['N'], case['C'], case['H'], case['W'], case['up'], case['ncls']
    video = bool(case['video'])
    with torch.no_grad():
        ref = head._head_forward(xd, pfd, mpd, prevd if video else None, want_track=video, flags=flags)
    dims = head.mask_head[0].make_dims(B, N, H, W)
    packs = [h.stage_pack(torch.device(DEV)) for h in head.mask_head]
    arr, prep = _prepared(vkn, dims, packs, f'{name} {form}')
    pf3, prev3 = pfd.reshape(B, N, C).contiguous(), (prevd.reshape(B, N, C).contiguous() if video else None)
    need = L.vkn_head_workspace_bytes(ctypes.byref(dims))
    assert need > 256
    outs = dict(obj=((B, N, C), torch.float32), cls=((B, N, ncls), torch.float32), masks=((B, N, H, W), torch.float32),
                scaled=((B, N, H * up, W * up), torch.float32) if up > 1 else None, track=((B, N, C), torch.float32) if video else None)
    for extra in ((0, vkn.ops.FLAG_SERIAL_LINK) if video else (0,)):
        c = Call(vkn, 'vkn_head_forward_f32', f'head {name} {form} flags={flags | extra}', outs, need,
                 lambda o, ws, nb: L.vkn_head_forward_f32(ctypes.byref(dims), len(packs), arr, p(xd), p(pf3), p(mpd), p(prev3), o['obj'], o['cls'],
                                                          o['masks'], o['scaled'], up, o['track'], ws, nb, flags | extra, st()),
                 inputs=(xd, pf3, mpd, prev3), header=True)
        _bits_equal(f'{c.name} obj', c.out['obj'], ref[0].reshape(B, N, C))
        _bits_equal(f'{c.name} cls', c.out['cls'], ref[1])
        _bits_equal(f'{c.name} masks', c.out['masks'], ref[2])
        if up > 1:
            _bits_equal(f'{c.name} scaled', c.out['scaled'], ref[3])
        if video:
            _bits_equal(f'{c.name} track', c.out['track'], ref[4].reshape(B, N, C))
    if form == 'mfma':                                      # the same call with two caller-owned events around the last decode
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        e1.record()
        c = Call(vkn, 'vkn_head_forward_prof_f32', f'head_prof {name}', outs, need,
                 lambda o, ws, nb: L.vkn_head_forward_prof_f32(ctypes.byref(dims), len(packs), arr, p(xd), p(pf3), p(mpd), p(prev3), o['obj'], o['cls'],
                                                               o['masks'], o['scaled'], up, o['track'], ws, nb, flags, st(), ctypes.c_void_p(e0.cuda_event),
                                                               ctypes.c_void_p(e1.cuda_event)), inputs=(xd, pf3, mpd, prev3), header=True)
        _bits_equal(f'{c.name} masks', c.out['masks'], ref[2])
        assert e0.elapsed_time(e1) >= 0.0
    _prepared_unchanged(prep, f'{name} {form}')


@pytest.mark.parametrize('name', ['video_upd_tiny', 'video_updobj_tiny'])
def test_head_link_golden(vkn, name):
    """vkn_head_forward_link_f32 (previous_link / previous_type "update" blocks in the last stage), side stream and serial"""
    L = _lib(vkn)
    g, case, head, (xd, pfd, mpd, prevd) = _head_of(vkn, name)
    B, N, C, H, W, up, ncls = case['B'], case['N'], case['C'], case['H'], case['W'], case['up'], case['ncls']
    with torch.no_grad():
        ref = head._head_forward(xd, pfd, mpd, prevd, want_track=True)
    dev = torch.device(DEV)
    dims = head.mask_head[0].make_dims(B, N, H, W)
    arr, prep = _prepared(vkn, dims, [h.stage_pack(dev) for h in head.mask_head], name)
    pre, trk, src = head.mask_head[-1].link_packs(dev)
    links, lprep = _prepared(vkn, dims, [pk for pk in (pre, trk) if pk is not None], name + ' links')
    lp = iter(range(len(links)))
    pre_w = ctypes.byref(links[next(lp)]) if pre is not None else None
    trk_w = ctypes.byref(links[next(lp)]) if trk is not None else None
    assert pre_w is not None or trk_w is not None
    pf3, prev3 = pfd.reshape(B, N, C).contiguous(), prevd.reshape(B, N, C).contiguous()
    need = L.vkn_head_workspace_bytes(ctypes.byref(dims))
    outs = dict(obj=((B, N, C), torch.float32), cls=((B, N, ncls), torch.float32), masks=((B, N, H, W), torch.float32),
                scaled=((B, N, H * up, W * up), torch.float32) if up > 1 else None, track=((B, N, C), torch.float32))
    for extra in (0, vkn.ops.FLAG_SERIAL_LINK):
        c = Call(vkn, 'vkn_head_forward_link_f32', f'head_link {name} flags={extra}', outs, need,
                 lambda o, ws, nb: L.vkn_head_forward_link_f32(ctypes.byref(dims), len(arr), arr, pre_w, trk_w, src if trk is not None else 0, p(xd),
                                                               p(pf3), p(mpd), p(prev3), o['obj'], o['cls'], o['masks'], o['scaled'], up, o['track'],
                                                               ws, nb, extra, st()),
                 inputs=(xd, pf3, mpd, prev3), header=True)
        for k, r in zip(('obj', 'cls', 'masks', 'scaled', 'track'), ref):
            if k in c.out:
                _bits_equal(f'{c.name} {k}', c.out[k], r.reshape(c.out[k].shape))
    S_ = len(arr)
    last = head.mask_head[-1]
    bnc = ((B, N, C), torch.float32)
    ns = L.vkn_stage_workspace_bytes(ctypes.byref(dims))
    c = Call(vkn, 'vkn_stage_forward_link_f32', f'stage_link {name}', dict(cls=((B, N, ncls), torch.float32), masks=((B, N, H, W), torch.float32), obj=bnc,
                                                                           xfeat=bnc, track=bnc), ns,
             lambda o, ws, nb: L.vkn_stage_forward_link_f32(ctypes.byref(dims), ctypes.byref(arr[S_ - 1]), pre_w, trk_w, src if trk is not None else 0, p(xd),
                                                            p(pf3), p(mpd), p(prev3), o['cls'], o['masks'], o['obj'], o['xfeat'], o['track'], ws, nb, 0, st()),
             inputs=(xd, pf3, mpd, prev3), header=True)
    with torch.no_grad():
        sref = vkn.ops.stage_forward(dims, last.stage_pack(dev), xd, pf3, mpd, prev3, want_track=True, link_pre=pre, link_track=trk, track_src=src)
    for k, r in zip(('cls', 'masks', 'obj', 'xfeat', 'track'), sref):
        _bits_equal(f'{c.name} {k} against ops.stage_forward', c.out[k], r)
    _prepared_unchanged(prep + lprep, name)


@pytest.mark.parametrize('name', ['det_odd', 'video_tiny'])
def test_stage_entries(vkn, name):
    """vkn_stage_forward_f32 (x_feat_out / track_out given and NULL), vkn_stage_chain_f32 (cls_logits given and NULL), vkn_track_link_f32 /
    _flags_f32 and vkn_kernel_updator_f32 on a golden's last stage, workspace of exactly vkn_stage_workspace_bytes"""
    L = _lib(vkn)
    g, case, head, (xd, pfd, mpd, prevd) = _head_of(vkn, name)
    B, N, C, H, W, ncls = case['B'], case['N'], case['C'], case['H'], case['W'], case['ncls']
    video = bool(case['video'])
    last = head.mask_head[-1]
    dims = last.make_dims(B, N, H, W)
    arr, prep = _prepared(vkn, dims, [last.stage_pack(torch.device(DEV))], f'{name} stage')
    w = ctypes.byref(arr[0])
    pf3, prev3 = pfd.reshape(B, N, C).contiguous(), (prevd.reshape(B, N, C).contiguous() if video else None)
    need = L.vkn_stage_workspace_bytes(ctypes.byref(dims))
    assert need > 256
    bnc = ((B, N, C), torch.float32)
    for full in (True, False):
        outs = dict(cls=((B, N, ncls), torch.float32), masks=((B, N, H, W), torch.float32), obj=bnc, xfeat=bnc if full else None,
                    track=bnc if (full and video) else None)
        c = Call(vkn, 'vkn_stage_forward_f32', f'stage {name} full={full}', outs, need,
                 lambda o, ws, nb: L.vkn_stage_forward_f32(ctypes.byref(dims), w, p(xd), p(pf3), p(mpd), p(prev3) if (full and video) else None,
                                                           o['cls'], o['masks'], o['obj'], o['xfeat'], o['track'], ws, nb, 0, st()),
                 inputs=(xd, pf3, mpd, prev3), header=True)
        if full:
            with torch.no_grad():
                ref = vkn.ops.stage_forward(dims, last.stage_pack(torch.device(DEV)), xd, pf3, mpd, prev3, want_track=video)
            for k, r in zip(('cls', 'masks', 'obj', 'xfeat', 'track'), ref):
                if k in c.out:
                    _bits_equal(f'{c.name} {k} against ops.stage_forward', c.out[k], r)
            xfeat = c.out['xfeat'].clone()
    for with_cls in (True, False):
        outs = dict(cls=((B, N, ncls), torch.float32) if with_cls else None, kern=bnc, kb=((B, N), torch.float32), obj=bnc)
        Call(vkn, 'vkn_stage_chain_f32', f'stage_chain {name} cls={with_cls}', outs, need,
             lambda o, ws, nb: L.vkn_stage_chain_f32(ctypes.byref(dims), w, p(xfeat), p(pf3), o['cls'], o['kern'], o['kb'], o['obj'], ws, nb, 0, st()),
             inputs=(xfeat, pf3), header=True)
    Call(vkn, 'vkn_kernel_updator_f32', f'kernel_updator {name}', dict(out=bnc), need,
         lambda o, ws, nb: L.vkn_kernel_updator_f32(ctypes.byref(dims), w, p(xfeat), p(pf3), o['out'], ws, nb, st()), inputs=(xfeat, pf3), header=True)
    if video:
        c = Call(vkn, 'vkn_track_link_f32', f'track_link {name}', dict(track=bnc), need,
                 lambda o, ws, nb: L.vkn_track_link_f32(ctypes.byref(dims), w, p(pf3), p(prev3), o['track'], ws, nb, st()), inputs=(pf3, prev3), header=True)
        with torch.no_grad():
            _bits_equal(f'{c.name} against ops.track_link', c.out['track'], vkn.ops.track_link(dims, last.stage_pack(torch.device(DEV)), pf3, prev3))
        for fl in (vkn.ops.FLAG_CHAIN_KSPLIT, vkn.ops.FLAG_CHAIN_LAUNCHES):
            Call(vkn, 'vkn_track_link_flags_f32', f'track_link flags={fl} {name}', dict(track=bnc), need,
                 lambda o, ws, nb: L.vkn_track_link_flags_f32(ctypes.byref(dims), w, p(pf3), p(prev3), o['track'], ws, nb, fl, st()),
                 inputs=(pf3, prev3), header=True)
    _prepared_unchanged(prep, f'{name} stage')


@pytest.mark.parametrize('with_updator', [False, True])
def test_link_block(vkn, with_updator):
    """vkn_link_block_f32 as tests/test_gpu_update_link.py::test_link_block_vs_oracle builds it"""
    from helpers import load_golden
    from oracle import synth
    from test_gpu_parity import _build_head
    L = _lib(vkn)
    _, case = load_golden('video_upd_tiny')
    head, _ = _build_head(vkn, case)
    last = head.mask_head[-1]
    B, N, C = 3, case['N'], case['C']
    cur, prev, uf = (torch.from_numpy(synth.normalish((B, N, C), s_, sd)).to(DEV) for s_, sd in ((971, 1.0), (972, 1.0), (973, 30.0)))
    named = dict(last.named_parameters())
    dev = torch.device(DEV)
    if with_updator:
        pack = vkn.ops.link_pack(named, dev, *last._link_names('link'))
    else:
        pack = vkn.ops.link_pack(named, dev, None, 'attention_previous_link', 'attention_previous_norm_link', 'link_ffn_link', 'link_ffn_norm_link')
    dims = last.make_dims(B, N, case['H'], case['W'])
    arr, prep = _prepared(vkn, dims, [pack], 'link_block')
    need = L.vkn_stage_workspace_bytes(ctypes.byref(dims))
    ufp = uf if with_updator else None
    c = Call(vkn, 'vkn_link_block_f32', f'link_block updator={with_updator}', dict(out=((B, N, C), torch.float32)), need,
             lambda o, ws, nb: L.vkn_link_block_f32(ctypes.byref(dims), ctypes.byref(arr[0]), p(ufp), p(cur), p(prev), o['out'], ws, nb, st()),
             inputs=(cur, prev, ufp), header=True)
    with torch.no_grad():
        _bits_equal(f'{c.name} against ops.link_block', c.out['out'], vkn.ops.link_block(dims, pack, cur, prev, ufp))
    _prepared_unchanged(prep, 'link_block')


@pytest.mark.parametrize('B,N,C,F,with_pos', [(2, 10, 256, 2, True), (1, 33, 128, 3, True), (2, 7, 128, 1, False), (3, 50, 256, 6, True)])
def test_query_merge(vkn, B, N, C, F, with_pos):
    """vkn_query_merge_f32 as tests/test_gpu_vis.py::test_query_merge_op_vs_oracle builds it (<= 256 keys and more), workspace of exactly
    vkn_query_merge_workspace_bytes"""
    from oracle import synth
    L = _lib(vkn)
    g = torch.Generator().manual_seed(1000 + N + F)
    shapes = {'query_merge_attn.attn.in_proj_weight': (3 * C, C), 'query_merge_attn.attn.in_proj_bias': (3 * C,),
              'query_merge_attn.attn.out_proj.weight': (C, C), 'query_merge_attn.attn.out_proj.bias': (C,),
              'query_merge_norm.weight': (C,), 'query_merge_norm.bias': (C,),
              'query_merge_ffn.layers.0.0.weight': (8 * C, C), 'query_merge_ffn.layers.0.0.bias': (8 * C,),
              'query_merge_ffn.layers.1.weight': (C, 8 * C), 'query_merge_ffn.layers.1.bias': (C,),
              'query_merge_ffn_norm.weight': (C,), 'query_merge_ffn_norm.bias': (C,)}
    named = {k: torch.from_numpy(v).to(DEV) for k, v in synth.state_dict_like(shapes, 77 + C).items()}
    query, keys = torch.randn(B, N, C, generator=g).to(DEV), torch.randn(B, F * N, C, generator=g).to(DEV)
    pos = torch.randn(N, C, generator=g).to(DEV) if with_pos else None
    pack = vkn.ops.link_pack(named, torch.device(DEV), None, 'query_merge_attn', 'query_merge_norm', 'query_merge_ffn', 'query_merge_ffn_norm')
    dims = vkn.ops.make_dims(B, N, C, 8, 8, 8, 8 * C, 1, 0, 0)
    arr, prep = _prepared(vkn, dims, [pack], 'query_merge')
    need = L.vkn_query_merge_workspace_bytes(ctypes.byref(dims), F)
    assert need > 256
    c = Call(vkn, 'vkn_query_merge_f32', f'query_merge B{B} N{N} C{C} F{F}', dict(out=((B, N, C), torch.float32)), need,
             lambda o, ws, nb: L.vkn_query_merge_f32(ctypes.byref(dims), F, ctypes.byref(arr[0]), p(query), p(keys), p(pos), o['out'], ws, nb, st()),
             inputs=(query, keys, pos), header=True)
    with torch.no_grad():
        _bits_equal(f'{c.name} against ops.query_merge', c.out['out'], vkn.ops.query_merge(dims, pack, query, keys, pos))
    _prepared_unchanged(prep, 'query_merge')


# ====================================================================================================== joint panoptic merge
def _pan_cfg(vkn, case):
    from helpers import PAN_CFG
    return vkn._lib.VknPanopticCfg(case['Np'], case['T'], case['Np'], PAN_CFG['instance_score_thr'], PAN_CFG['overlap_thr'], case['up'],
                                   case['Hm'], case['Wm'], case['Hb'], case['Wb'], case['h'], case['w'], case['Ho'], case['Wo'])


def _pan_call(vkn, name, case, cls, logits, with_bbox):
    L = _lib(vkn)
    cfg = _pan_cfg(vkn, case)
    B, N, ncls = case['B'], case['N'], case['ncls']
    K = case['Np'] + (N - case['Np'])
    need = L.vkn_panoptic_workspace_bytes(ctypes.byref(cfg), B, N)
    assert need > 0
    outs = dict(seg=((B, case['Ho'], case['Wo']), torch.int32), info=((B, K, 6), torch.int32), nseg=((B,), torch.int32),
                bbox=((B, K, 4), torch.int32) if with_bbox else None)
    return Call(vkn, 'vkn_panoptic_joint_f32', f'panoptic {name} bbox={with_bbox}', outs, need,
                lambda o, ws, nb: L.vkn_panoptic_joint_f32(ctypes.byref(cfg), p(cls), p(logits), B, N, ncls, o['seg'], o['info'], o['nseg'], o['bbox'],
                                                           ws, nb, st()), inputs=(cls, logits))


@pytest.mark.parametrize('name', ['pan_tiny', 'pan_ident'])
@pytest.mark.parametrize('with_bbox', [False, True], ids=['nobbox', 'bbox'])
def test_panoptic_joint(vkn, name, with_bbox):
    from helpers import assert_pan_matches_oracle, load_pan_golden, make_pan_case, run_pan_oracle
    g, case = load_pan_golden(name)
    cls, logits, _ = make_pan_case(case)
    cls, logits = _cuda(cls, logits)
    c = _pan_call(vkn, name, case, cls, logits, with_bbox)
    seg, info, nseg = (c.out[k].cpu().numpy() for k in ('seg', 'info', 'nseg'))
    for b in range(case['B']):
        assert int(nseg[b]) == int(g['nseg'][b])
        assert_pan_matches_oracle(seg[b], info[b], nseg[b], run_pan_oracle(case, b), want_seg=g['panoptic_seg'][b])


def test_panoptic_joint_cropped_and_resized(vkn):
    """B = 2, img_shape smaller than batch_input_shape (h, w < Hb, Wb) and an output size (Ho, Wo) different from both: the crop and the
    two resamplings all have ragged edges"""
    from helpers import assert_pan_matches_oracle, make_pan_case, run_pan_oracle
    case = dict(B=2, N=23, Np=15, T=3, ncls=11, Hm=12, Wm=20, up=4, Hb=48, Wb=80, h=41, w=67, Ho=59, Wo=93, seed=31)
    cls, logits, _ = make_pan_case(case)
    cls, logits = _cuda(cls, logits)
    for with_bbox in (False, True):
        c = _pan_call(vkn, 'cropped', case, cls, logits, with_bbox)
        seg, info, nseg = (c.out[k].cpu().numpy() for k in ('seg', 'info', 'nseg'))
        for b in range(2):
            assert_pan_matches_oracle(seg[b], info[b], nseg[b], run_pan_oracle(case, b))


# ====================================================================================================== assignment
ASSIGN_CFG = (2.0, 4.0, 1.0, 0.25, 2.0, 1e-12, 1e-3, 1e-3, 1e-2)       # the defaults of ops.assign_costs (the shipped assigner)


@pytest.mark.parametrize('name', ['assign_tiny', 'assign_odd'])
def test_assign_costs(vkn, name):
    """vkn_assign_costs_f32 and the batch form (two images sharing one workspace of the larger G) on the goldens' inputs: bit-identical to
    ops.assign_costs, whose values tests/test_gpu_parity.py::test_assignment_vs_reference pins; against the oracle's cost matrix with
    that test's own comparison of the assignment (scipy on both: the same rows and columns)"""
    from helpers import load_assign_golden, make_assign_case
    from scipy.optimize import linear_sum_assignment
    L = _lib(vkn)
    g, case = load_assign_golden(name)
    N, G, ncls, P = case['N'], case['G'], case['ncls'], case['H'] * case['W']
    logits, cls, gt, labels = _cuda(*make_assign_case(case))
    logits, gt, lab = logits.reshape(N, P).contiguous(), gt.reshape(G, P).float().contiguous(), labels.to(torch.int32).contiguous()
    cfg = vkn._lib.VknAssignCfg(*ASSIGN_CFG)
    need = L.vkn_assign_workspace_bytes(N, G, P)
    assert need > 0
    c = Call(vkn, 'vkn_assign_costs_f32', f'assign {name}', dict(cost=((N, G), torch.float32)), need,
             lambda o, ws, nb: L.vkn_assign_costs_f32(ctypes.byref(cfg), p(logits), p(cls), p(gt), p(lab), N, G, ncls, P, o['cost'], ws, nb, st()),
             inputs=(logits, cls, gt, lab))
    _bits_equal(f'{c.name} against ops.assign_costs', c.out['cost'], vkn.ops.assign_costs(logits, cls, gt, labels))
    assert [a.tolist() for a in linear_sum_assignment(c.out['cost'].cpu().numpy())] == [a.tolist() for a in linear_sum_assignment(g['cost'])]
    G2 = max(1, G // 2)                                     # a second image with fewer ground truths: the workspace is sized by the larger
    gt2, lab2 = gt[:G2].contiguous(), lab[:G2].contiguous()

    def batch(o, ws, nb):
        probs = (vkn._lib.VknAssignProblem * 2)(vkn._lib.VknAssignProblem(logits.data_ptr(), cls.data_ptr(), gt.data_ptr(), lab.data_ptr(), G, o['c0'].value),
                                                vkn._lib.VknAssignProblem(logits.data_ptr(), cls.data_ptr(), gt2.data_ptr(), lab2.data_ptr(), G2, o['c1'].value))
        return L.vkn_assign_costs_batch_f32(ctypes.byref(cfg), probs, 2, N, ncls, P, ws, nb, st())
    cb = Call(vkn, 'vkn_assign_costs_batch_f32', f'assign batch {name}', dict(c0=((N, G), torch.float32), c1=((N, G2), torch.float32)), need, batch,
              inputs=(logits, cls, gt, lab, gt2, lab2))
    _bits_equal(f'{cb.name} image 0', cb.out['c0'], c.out['cost'])
    _bits_equal(f'{cb.name} image 1 against ops.assign_costs', cb.out['c1'], vkn.ops.assign_costs(logits, cls, gt2, labels[:G2]))


def test_assign_costs_lowres(vkn):
    """vkn_assign_costs_lowres_batch_f32 on the n150_g70, odd_h and ragged_s2 cases of tests/test_gpu_assign_lowres.py, workspace of exactly
    vkn_assign_lowres_workspace_bytes: bit-identical to ops.assign_costs_lowres_batch (that module pins its values to `_want`), and the
    assignment scipy takes from `_want`'s float64 costs"""
    import test_gpu_assign_lowres as T
    from scipy.optimize import linear_sum_assignment
    L = _lib(vkn)
    ids = ['cfg3', 'stride2', 'n150_g70', 'n256', 'n37', 'kitti_step', 'odd_h', 'ragged_s2']
    cfg = vkn._lib.VknAssignCfg(*ASSIGN_CFG)
    for cid in ('n150_g70', 'odd_h', 'ragged_s2'):
        N, Gs, ncls, h, w, S, soft = T.CASES[ids.index(cid)]
        lows, clss, gts, labs = T._case(N, Gs, ncls, h, w, S, 11, soft)
        dl = [t[:N].contiguous().to(DEV) for t in lows]
        dc, dg = [t.to(DEV) for t in clss], [t.float().contiguous().to(DEV) for t in gts]
        dlab = [t.to(device=DEV, dtype=torch.int32) for t in labs]
        need = L.vkn_assign_lowres_workspace_bytes(len(Gs), N, max(Gs), h, w, S)
        assert need > 0

        def call(o, ws, nb):
            probs = (vkn._lib.VknAssignProblem * len(Gs))(*[vkn._lib.VknAssignProblem(dl[b].data_ptr(), dc[b].data_ptr(), dg[b].data_ptr(), dlab[b].data_ptr(),
                                                                                      Gs[b], o[f'c{b}'].value) for b in range(len(Gs))])
            return L.vkn_assign_costs_lowres_batch_f32(ctypes.byref(cfg), probs, len(Gs), N, ncls, h, w, S, ws, nb, st())
        c = Call(vkn, 'vkn_assign_costs_lowres_batch_f32', f'assign lowres {cid}', {f'c{b}': ((N, G), torch.float32) for b, G in enumerate(Gs)}, need,
                 call, inputs=dl + dc + dg + dlab, ws_align=16)
        ref = vkn.ops.assign_costs_lowres_batch(dl, S, dc, dg, [t.to(DEV) for t in labs])
        for b in range(len(Gs)):
            _bits_equal(f'{c.name} image {b} against ops.assign_costs_lowres_batch', c.out[f'c{b}'], ref[b].contiguous())
            want = T._want(lows[b][:N], clss[b], gts[b], labs[b], S)
            assert [a.tolist() for a in linear_sum_assignment(c.out[f'c{b}'].cpu().double().numpy())] == [a.tolist() for a in linear_sum_assignment(want.numpy())]


LSAP_SIZES = (1, 2, 63, 64, 65, 256)


def test_lsap_batch(vkn):
    """vkn_lsap_batch_f32 against scipy on nr, nc in {1, 2, 63, 64, 65, 256} (rectangular both ways), continuous and massively tied costs,
    with every combination of NULL outputs: gt_inds of exactly nr, the pairs of exactly min(nr, nc) elements, status of exactly nprob"""
    from scipy.optimize import linear_sum_assignment
    L = _lib(vkn)
    rng = np.random.default_rng(7)
    shapes = [(nr, nc) for nr in LSAP_SIZES for nc in LSAP_SIZES]
    mats = [(rng.integers(0, 4, s).astype(np.float32) if i % 2 else rng.standard_normal(s).astype(np.float32)) for i, s in enumerate(shapes)]
    dev = [torch.from_numpy(m).to(DEV) for m in mats]
    for combo in range(16):
        with_g, with_r, with_c, with_s = (bool(combo >> i & 1) for i in range(4))
        outs = {}
        for b, (nr, nc) in enumerate(shapes):
            outs[f'g{b}'] = ((nr,), torch.int64) if with_g else None
            outs[f'r{b}'] = ((min(nr, nc),), torch.int32) if with_r else None
            outs[f'c{b}'] = ((min(nr, nc),), torch.int32) if with_c else None
        outs['status'] = ((len(shapes),), torch.int32) if with_s else None

        def call(o, ws, nb):
            v = lambda q: q.value if q is not None else None      # noqa: E731
            probs = (vkn._lib.VknLsapProblem * len(shapes))(*[vkn._lib.VknLsapProblem(dev[b].data_ptr(), nr, nc, v(o[f'g{b}']), v(o[f'r{b}']), v(o[f'c{b}']))
                                                              for b, (nr, nc) in enumerate(shapes)])
            return L.vkn_lsap_batch_f32(probs, len(shapes), o['status'], st())
        c = Call(vkn, 'vkn_lsap_batch_f32', f'lsap outputs={combo:04b}', outs, None, call, inputs=dev)
        if with_s:
            assert c.out['status'].cpu().tolist() == [0] * len(shapes)
        for b, m in enumerate(mats):
            sr, sc = linear_sum_assignment(m)
            if with_r:
                assert np.array_equal(c.out[f'r{b}'].cpu().numpy(), sr), (combo, m.shape)
            if with_c:
                assert np.array_equal(c.out[f'c{b}'].cpu().numpy(), sc), (combo, m.shape)
            if with_g:
                want = np.zeros(m.shape[0], dtype=np.int64)
                want[sr] = sc + 1
                assert np.array_equal(c.out[f'g{b}'].cpu().numpy(), want), (combo, m.shape)


# ====================================================================================================== the loss tail
def _tail_case(B, Ns, h, w, S, K, masks):
    import test_gpu_lowres_tail_kernels as T
    return T._case(B, Ns, h, w, S, K, masks)


def _f64_small():
    import test_gpu_lowres_tail_kernels as T
    return [c for c in T.F64_CASES if c[2] * c[3] < 1000]


def test_the_five_small_cases_exist():
    assert len(_f64_small()) == 5


@pytest.mark.parametrize('i', range(5))
def test_loss_tail(vkn, i):
    """The loss tail of a training stage, entry by entry, on the five small F64_CASES of tests/test_gpu_lowres_tail_kernels.py; every
    partial-sum buffer has exactly vkn_*_chunks / _blocks elements.  The lse / top / bank outputs of the low-res forms sit 8-byte but not
    16-byte aligned (the header's rule for them).  Each entry is bit-identical to the same call on plain buffers (the form that module
    and tests/test_gpu_tail.py pin to float64 and to the reference); the rank target additionally equals helpers.lowres_tail_reference's
    exactly, and vkn_focal_loss_f32 is ops.focal_loss_fwd's bits (tests/test_gpu_train.py::test_fused_focal_loss_vs_torch_formula)."""
    import test_gpu_lowres_tail_kernels as T
    from helpers import lowres_tail_reference
    L, lib = _lib(vkn), vkn._lib
    B, Ns, h, w, S, K, masks = _f64_small()[i]
    _, low, bank, rowk, tgt, posd, K = _tail_case(B, Ns, h, w, S, K, masks)
    H, W = S * h, S * w
    P, R = H * W, B * Ns
    tag = f'{B}x{Ns}x{h}x{w}x{S}'
    skew8 = dict(skew=8)
    f32, i32, i64 = torch.float32, torch.int32, torch.int64
    # ---- vkn_stage_targets: the case's positives as one image per frame; image b's matched rows are its positive rows, target = bank row
    ncls, T_, pw = 5, 0, 0.7
    rk = rowk.cpu()
    imgs, keep, pos0 = (lib.VknTailImage * B)(), [], 0
    glab = torch.arange(K, dtype=i64, device=DEV) % ncls
    for b in range(B):
        rows = torch.nonzero(rk[b * Ns:(b + 1) * Ns] >= 0).flatten().to(dtype=i32)
        cols = torch.arange(rows.numel(), dtype=i32)
        rows, cols = rows.to(DEV), cols.to(DEV)
        keep += [rows, cols]
        imgs[b] = lib.VknTailImage(rows.data_ptr() if rows.numel() else None, cols.data_ptr() if rows.numel() else None, glab[pos0:].data_ptr(), None,
                                   int(rows.numel()), 0, pos0, 0, pos0, 0)
        pos0 += int(rows.numel())
    assert pos0 == K
    t = Call(vkn, 'vkn_stage_targets', f'stage_targets {tag}',
             dict(labels=((R,), i64), lw=((R, ncls), f32), rw=((R,), f32), rowk=((R,), i32), pos=((K,), i64), tgt=((R,), i32), status=((1,), i32)), None,
             lambda o, ws, nb: L.vkn_stage_targets(imgs, B, Ns, 0, T_, ncls, pw, o['labels'], o['lw'], o['rw'], o['rowk'], o['pos'], o['tgt'], o['status'], st()),
             inputs=keep + [glab], pre=lambda o: o['status'].zero_())
    assert int(t.out['status']) == 0
    assert torch.equal(t.out['rowk'], rowk) and torch.equal(t.out['pos'], posd.to(i64))
    assert torch.equal(t.out['tgt'][rowk >= 0], tgt[rowk >= 0]) and bool((t.out['tgt'][rowk < 0] == -1).all())
    labels, lw = t.out['labels'], t.out['lw']
    # ---- vkn_focal_loss_f32
    z = (torch.randn(R, ncls, generator=torch.Generator().manual_seed(3 + i)) * 4).to(DEV)
    nbf = L.vkn_focal_loss_blocks(R, ncls)
    f = Call(vkn, 'vkn_focal_loss_f32', f'focal {tag}', dict(part=((nbf,), f32), grad=((R, ncls), f32)), None,
             lambda o, ws, nb: L.vkn_focal_loss_f32(p(z), p(labels), p(lw), 1, R, ncls, 0.25, 2.0, o['part'], o['grad'], st()), inputs=(z, labels, lw))
    s_ref, g_ref = vkn.ops.focal_loss_fwd(z, labels, lw, 0.25, 2.0)
    _bits_equal(f'{f.name} grad against ops.focal_loss_fwd', f.out['grad'], g_ref)
    _bits_equal(f'{f.name} sum against ops.focal_loss_fwd', f.out['part'].sum(), s_ref)
    # ---- the forward sums from the low-res logits, and from their up-scaling
    ncl = L.vkn_mask_losses_lowres_chunks(h, w)
    ref = lowres_tail_reference(low, bank, tgt, rowk, S, T.W_LOSS, T.G_UP)
    fw = Call(vkn, 'vkn_mask_losses_fwd_lowres_f32', f'fwd_lowres {tag}',
              dict(rp=((K, ncl, 4), f32), lse=((B, P), f32, skew8), top=((B, P), i32, skew8), rkp=((B, ncl), f32)), None,
              lambda o, ws, nb: L.vkn_mask_losses_fwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), K, B, Ns, h, w, S, 1, o['rp'], o['lse'], o['top'], o['rkp'], st()),
              inputs=(low, bank, tgt, rowk))
    assert torch.equal(fw.out['top'], ref['top'])
    scaled = vkn.ops.upsample_bilinear(low, S)
    nch, nbl = L.vkn_mask_losses_chunks(P), L.vkn_mask_losses_blocks(P)
    if P % 4 == 0:
        fb = Call(vkn, 'vkn_mask_losses_fwd_bank_f32', f'fwd_bank {tag}', dict(rp=((K, nch, 4), f32), lse=((B, P), f32), top=((B, P), i32), rkp=((B, nbl), f32)),
                  None, lambda o, ws, nb: L.vkn_mask_losses_fwd_bank_f32(p(scaled), p(bank), p(tgt), p(posd), p(rowk), K, B, Ns, P, 1, o['rp'], o['lse'],
                                                                        o['top'], o['rkp'], st()), inputs=(scaled, bank, tgt, posd, rowk))
        assert torch.equal(fb.out['top'], ref['top'])
        target = torch.zeros(R, P, device=DEV)
        target[posd] = bank.reshape(-1, P)[tgt[posd].long()]
        fp = Call(vkn, 'vkn_mask_losses_fwd_f32', f'fwd {tag}', dict(rp=((K, nch, 4), f32), lse=((B, P), f32), top=((B, P), i32), rkp=((B, nbl), f32)), None,
                  lambda o, ws, nb: L.vkn_mask_losses_fwd_f32(p(scaled), p(target), p(posd), p(rowk), K, B, Ns, P, 1, o['rp'], o['lse'], o['top'], o['rkp'], st()),
                  inputs=(scaled, target, posd, rowk))
        for k in ('rp', 'lse', 'top', 'rkp'):
            _bits_equal(f'{fp.name} {k} against the bank form', fp.out[k], fb.out[k])
    # ---- vkn_stage_losses_final_f32 on the low-res sums
    tcfg = lib.VknTailCfg(2.0, T.W_LOSS[0], T.W_LOSS[1], 1e-3, T.W_LOSS[2], float(max(K, 1)), 1)
    rp, rkp = fw.out['rp'], fw.out['rkp']
    fin = Call(vkn, 'vkn_stage_losses_final_f32', f'final {tag}', dict(losses=((5,), f32), a=((K,), f32), bc=((K,), f32)), None,
               lambda o, ws, nb: L.vkn_stage_losses_final_f32(ctypes.byref(tcfg), None, p(f.out['part']), nbf, p(rp), K, ncl, p(rkp), B * ncl, p(z), p(labels),
                                                              p(t.out['pos']), ncls, B, P, o['losses'], o['a'], o['bc'], st()),
               inputs=(f.out['part'], rp, rkp, z, labels, t.out['pos']))
    assert bool(torch.isfinite(fin.out['losses']).all())
    # ---- the backward forms
    gs = [torch.full((1,), v, device=DEV) for v in T.G_UP]
    a_, bc = fin.out['a'], fin.out['bc']
    lse, top = fw.out['lse'], fw.out['top']
    assert lse.data_ptr() % 16 == 8 and top.data_ptr() % 16 == 8
    bl = Call(vkn, 'vkn_mask_losses_bwd_lowres_f32', f'bwd_lowres {tag}', dict(grad=((B, Ns, h, w), f32)), None,
              lambda o, ws, nb: L.vkn_mask_losses_bwd_lowres_f32(p(low), p(bank), p(tgt), p(rowk), p(a_), p(bc), p(gs[0]), p(gs[1]), p(gs[2]), *T.W_LOSS, K,
                                                                 p(lse), p(top), B, Ns, h, w, S, 1, o['grad'], st()),
              inputs=(low, bank, tgt, rowk, a_, bc, lse, top, *gs))
    if P % 4 == 0:
        bb = Call(vkn, 'vkn_mask_losses_bwd_bank_f32', f'bwd_bank {tag}', dict(grad=((R, P), f32)), None,
                  lambda o, ws, nb: L.vkn_mask_losses_bwd_bank_f32(p(scaled), p(bank), p(tgt), p(rowk), p(a_), p(bc), p(gs[0]), p(gs[1]), p(gs[2]), *T.W_LOSS, K,
                                                                   p(fb.out['lse']), p(fb.out['top']), B, Ns, P, 1, o['grad'], st()),
                  inputs=(scaled, bank, tgt, rowk, a_, bc, *gs))
        coef = torch.tensor([T.G_UP[0] * T.W_LOSS[0] / (K * P), T.G_UP[2] * T.W_LOSS[2] / (B * P)], device=DEV)
        rowcoef = torch.stack([-2 / bc, 4 * a_ / (bc * bc)], 1).mul(T.G_UP[1] * T.W_LOSS[1] / K).contiguous()
        Call(vkn, 'vkn_mask_losses_bwd_f32', f'bwd {tag}', dict(grad=((R, P), f32)), None,
             lambda o, ws, nb: L.vkn_mask_losses_bwd_f32(p(scaled), p(target), p(rowk), p(rowcoef), p(coef), p(fb.out['lse']), p(fb.out['top']), B, Ns, P, 1,
                                                         o['grad'], st()), inputs=(scaled, target, rowk, rowcoef, coef))
        assert bool(torch.isfinite(bb.out['grad']).all())
    # ---- glue: scale_by (n not a multiple of 4), sum_n (VKN_SUM_MAX sources), sgd (in place: param and mom are outputs AND inputs)
    n = R * ncls
    g1, d1 = torch.full((1,), 1.7, device=DEV), torch.full((1,), 3.0, device=DEV)
    sb = Call(vkn, 'vkn_scale_by_f32', f'scale_by {tag}', dict(out=((n,), f32)), None,
              lambda o, ws, nb: L.vkn_scale_by_f32(p(f.out['grad']), p(g1), p(d1), 2.0, o['out'], n, st()), inputs=(f.out['grad'], g1, d1))
    _close64(f'{sb.name}', sb.out['out'], f.out['grad'].reshape(-1).double() * 2.0 * 1.7 / 3.0, None, 4 + 2)   # 2 mul, 1 div; 1.7 and 2 / 3 as fp32
    parts = [bl.out['grad'].reshape(-1) * (j + 1) for j in range(vkn._lib.CONSTS['VKN_SUM_MAX'])]
    srcs = (ctypes.c_void_p * len(parts))(*[q.data_ptr() for q in parts])
    sm = Call(vkn, 'vkn_sum_n_f32', f'sum_n {tag}', dict(out=((parts[0].numel(),), f32)), None,
              lambda o, ws, nb: L.vkn_sum_n_f32(srcs, len(parts), parts[0].numel(), o['out'], st()), inputs=parts)
    want = parts[0]
    for q in parts[1:]:
        want = want + q
    _bits_equal(f'{sm.name} against torch adds in that order', sm.out['out'], want)
    par0, mom0 = torch.randn(n, generator=torch.Generator().manual_seed(5)).to(DEV), torch.randn(n, generator=torch.Generator().manual_seed(6)).to(DEV)
    grad = f.out['grad'].reshape(-1).contiguous()

    def fill(o):
        o['param'].copy_(par0)
        o['mom'].copy_(mom0)
    sg = Call(vkn, 'vkn_sgd_momentum_f32', f'sgd {tag}', dict(param=((n,), f32), mom=((n,), f32)), None,
              lambda o, ws, nb: L.vkn_sgd_momentum_f32(o['param'], p(grad), o['mom'], n, 0.01, 0.9, 1e-4, 0.5, st()), inputs=(grad,), pre=fill)
    assert not torch.equal(sg.out['param'], par0) and not torch.equal(sg.out['mom'], mom0)
    # torch.optim.SGD's rule in float64; the bound counts the fp32 roundings of the formula against the sum of the |terms| (see _close64)
    g64, p64, m64 = grad.double(), par0.double(), mom0.double()
    mom_ref = 0.9 * m64 + (g64 * 0.5 + 1e-4 * p64)
    mom_mag = 0.9 * m64.abs() + g64.abs() * 0.5 + 1e-4 * p64.abs()
    _close64(f'{sg.name} mom', sg.out['mom'], mom_ref, mom_mag, 5 + 3)             # 3 mul, 2 add; momentum, weight_decay, grad_scale as fp32
    _close64(f'{sg.name} param', sg.out['param'], p64 - 0.01 * mom_ref, p64.abs() + 0.01 * mom_mag, 7 + 4)   # + mul, sub; lr as fp32


# ====================================================================================================== tracker
@pytest.mark.parametrize('name', ['trk_a', 'trk_c'])
def test_qd_tracker(vkn, name):
    """vkn_qd_tracker_reset / _match_f32 on the `qd_tracker` golden: `state` of exactly vkn_qd_tracker_state_bytes, `ws` of exactly
    vkn_qd_tracker_workspace_bytes, outputs of exactly max_dets rows; ids, labels and boxes bit-exact against the reference's own"""
    from helpers import GOLDEN
    from oracle import synth
    from test_gpu_tracker import CFG
    L = _lib(vkn)
    g = dict(np.load(os.path.join(GOLDEN, 'qd_tracker.npz'), allow_pickle=False))
    T, n_obj, emb, n_cls, seed = (int(v) for v in g[name + '_case'])
    trk = vkn.build_tracker(dict(CFG, type='QuasiDenseEmbedTracker', match_metric=str(g[name + '_metric']), max_dets=64, max_tracklets=96))
    cfg = trk._make_cfg(emb)
    D = cfg.max_dets
    nstate, nws = L.vkn_qd_tracker_state_bytes(ctypes.byref(cfg)), L.vkn_qd_tracker_workspace_bytes(ctypes.byref(cfg))
    assert nstate > 0 and nws > 0
    _ws('vkn_qd_tracker_match_f32', nws)
    WS_BYTES.setdefault('vkn_qd_tracker_match_f32 (state)', set()).add(nstate)
    S_ = Arena(DEV)
    state = S_.ws(nstate, name='state')
    assert L.vkn_qd_tracker_reset(ctypes.byref(cfg), state.ptr, nstate - 1, st()) == E_WORKSPACE
    _untouched(S_, 'tracker reset of a short state')
    assert L.vkn_qd_tracker_reset(ctypes.byref(cfg), state.ptr, nstate, st()) == OK
    S_.check(f'{name} reset')
    for t, (bb, lab, em, _) in enumerate(synth.tracker_sequence(T, n_obj, emb, n_cls, seed)):
        bbd, labd, emd = torch.from_numpy(bb).to(DEV), torch.from_numpy(lab).to(DEV).long(), torch.from_numpy(em).to(DEV)
        n = int(bbd.shape[0])
        assert n <= D
        A = Arena(DEV)
        ob, ol = A.out((D, 5), torch.float32, name='out_bboxes', full=False), A.out((D,), torch.int64, name='out_labels', full=False)
        oi, oc, w = A.out((D,), torch.int64, name='out_ids', full=False), A.out((2,), torch.int32, name='out_count'), A.ws(nws, name='ws')
        with frozen(bbd, labd, emd):
            assert L.vkn_qd_tracker_match_f32(ctypes.byref(cfg), state.ptr, nstate, p(bbd), p(labd), p(emd), n, t, ob.ptr, ol.ptr, oi.ptr, oc.ptr,
                                              w.ptr, nws, st()) == OK
        A.check(f'{name} frame {t}')
        S_.check(f'{name} state after frame {t}')
        k, status = oc.t.cpu().tolist()
        assert status == 0
        assert np.array_equal(oi.t[:k].cpu().numpy(), g[f'{name}_ids{t}']), (name, t)
        assert np.array_equal(ol.t[:k].cpu().numpy(), g[f'{name}_labels{t}']) and np.array_equal(ob.t[:k].cpu().numpy(), g[f'{name}_bboxes{t}'])


# ====================================================================================================== localization FPN
FPN_LEVELS = [[(8, 8), (4, 4), (2, 2), (1, 1)], [(7, 15), (4, 8), (2, 4), (1, 2)]]       # ceil(H2 / 2) = H3 = 2 H4 = 4 H5: the header's rule
FPN_DECLINED = [(8, 10), (4, 5), (2, 3), (1, 2)]                                         # 2 W4 != W3: no stride-8 grid (VKN_E_SHAPE, size query 0)


def _fpn_module(vkn, C):
    """tests/test_gpu_semantic_fpn.py::_module with the positional encoding as wide as the features (num_feats = C / 2: the shipped
    128 is C = 256's)"""
    import copy
    import test_gpu_semantic_fpn as T
    if C == 256:
        return T._module(vkn)
    torch.manual_seed(0)
    cfg = copy.deepcopy(T.SHIPPED)
    cfg.update(in_channels=C, feat_channels=C, out_channels=C)
    cfg['positional_encoding']['num_feats'] = C // 2
    m = vkn.registry.HEADS.build(cfg)
    m.init_weights()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    return m.to(DEV).eval()


def _fpn(vkn, B, C, shapes, rule=True):
    import test_gpu_semantic_fpn as T
    L = _lib(vkn)
    m, ls, x = _fpn_module(vkn, C), T._loc_seg(vkn, C), T._levels(B, C, shapes)
    pos = m.positional_map(1, shapes[3][0], shapes[3][1], torch.device(DEV))[0].contiguous() if m.positional_encoding is not None else None
    imgs, gam, bet = m.prepared(ls)
    arr = lambda ts: (ctypes.c_void_p * 10)(*[q.data_ptr() for q in ts])      # noqa: E731
    dims = [int(d) for q in x for d in q.shape[2:]]
    need = L.vkn_localization_fpn_workspace_bytes(B, C, *dims)
    H3, W3 = shapes[1]
    call = lambda o, ws, nb: L.vkn_localization_fpn_f32(*[p(q) for q in x], p(pos), arr(imgs), arr(gam), arr(bet), m.num_groups, o['loc'], o['sem'], B, C,  # noqa: E731
                                                        *dims, ws, nb, st())
    outs = dict(loc=((B, C, H3, W3), torch.float32), sem=((B, C, H3, W3), torch.float32))
    if need == 0:
        return call, outs, None
    c = Call(vkn, 'vkn_localization_fpn_f32', f'fpn B{B} C{C} {shapes}', outs, need, call, inputs=list(x) + [pos] + list(imgs) + list(gam) + list(bet),
             header=True)
    if rule:
        with torch.no_grad():
            t_out, t_aux = m.forward_torch(x)
            r_out, r_aux = T.fpn_ref64(m, x)
            for n_, hip, tt, rr in (('loc', c.out['loc'], ls[0](t_out), T._cm64(ls[0], r_out)), ('sem', c.out['sem'], ls[1](t_aux), T._cm64(ls[1], r_aux))):
                T._rule(f'abi fpn B{B} C{C} {shapes[1]} {n_}', hip, tt, rr)
    return call, outs, c


@pytest.mark.parametrize('shapes', FPN_LEVELS, ids=['8x8', '7x15'])
def test_localization_fpn(vkn, shapes):
    """vkn_localization_fpn_f32 at C = 64 on the smallest pyramids the shape rule admits (one of them with an odd P2), workspace of
    exactly vkn_localization_fpn_workspace_bytes behind a cleared header; the rule of tests/test_gpu_semantic_fpn.py"""
    _fpn(vkn, 2, 64, shapes)


def test_localization_fpn_kitti_levels(vkn):
    import test_gpu_semantic_fpn as T
    _fpn(vkn, 1, 256, T.KITTI)


def test_localization_fpn_declines_levels_without_a_common_grid(vkn):
    """P2..P5 = (8, 10), (4, 5), (2, 3), (1, 2) — successive ceil-halving, as a backbone produces them from an 80-pixel-wide frame: the
    up-scaled P4 is 6 wide against P3's 5, the reference's own level sum fails there.  The size query answers 0 and the entry returns
    VKN_E_SHAPE before a launch."""
    call, outs, c = _fpn(vkn, 1, 64, FPN_DECLINED)
    assert c is None
    A = Arena(DEV)
    o = {k: A.out(sh, dt, name=k) for k, (sh, dt) in outs.items()}
    w = A.ws(1 << 16, name='ws')
    assert call({k: r.ptr for k, r in o.items()}, w.ptr, w.nbytes) == E_SHAPE
    _untouched(A, 'fpn on levels without a common grid')


# ====================================================================================================== thing-first merge, flat AdamW
@pytest.mark.parametrize('name', ['merge_tf_edges', 'merge_tf_video', 'merge_tf_empty_things'])
def test_thing_first_merge(vkn, name):
    """vkn_panoptic_thing_first_u8 on fixtures of tests/test_gpu_merge_thing_first.py, workspace of exactly vkn_merge_workspace_bytes:
    map, info and nseg exactly `oracle.thing_first_merge`'s (that module's rule)"""
    from helpers import load_merge_tf, merge_tf_oracle
    L = _lib(vkn)
    g, a, thr = load_merge_tf(name)
    a, r = merge_tf_oracle(a, thr)
    Kt, Ks = len(a['thing_order']), len(a['stuff_order'])
    HW = int(np.prod(a['thing_masks'].shape[1:]))
    u8 = lambda m: np.asarray(m).astype(np.uint8, copy=False).reshape(m.shape[0], HW)  # noqa: E731
    dev = lambda t, dt: None if t is None or t.size == 0 else torch.from_numpy(np.ascontiguousarray(t)).to(dt).to(DEV)  # noqa: E731  (empty: NULL at the ABI)
    d = [dev(u8(a['thing_masks']), torch.uint8), dev(a['thing_scores'], torch.float32), dev(a['thing_labels'], torch.int32),
         dev(a['thing_order'], torch.int32), dev(u8(a['stuff_masks']), torch.uint8), dev(a['stuff_labels'], torch.int32),
         dev(a['stuff_order'], torch.int32)]
    need = L.vkn_merge_workspace_bytes(Kt, Ks)
    assert need > 0
    c = Call(vkn, 'vkn_panoptic_thing_first_u8', f'thing_first {name}',
             dict(seg=((HW,), torch.int32), info=((Kt + Ks, 5), torch.int32) if Kt + Ks else None, nseg=((1,), torch.int32)), need,
             lambda o, ws, nb: L.vkn_panoptic_thing_first_u8(p(d[0]), p(d[1]), p(d[2]), p(d[3]), Kt, p(d[4]), p(d[5]), p(d[6]), Ks, HW,
                                                             float(thr['instance_score_thr']), float(thr['iou_thr']), int(thr['stuff_max_area']), o['seg'],
                                                             o['info'], o['nseg'], ws, nb, st()), inputs=d, ws_align=16)
    assert np.array_equal(c.out['seg'].cpu().numpy().reshape(r['panoptic_seg'].shape), r['panoptic_seg']) and int(c.out['nseg']) == r['nseg']
    _gate(vkn, 'vkn_panoptic_thing_first_u8', dict(seg=((HW,), torch.int32), info=((max(Kt + Ks, 1), 5), torch.int32), nseg=((1,), torch.int32)), need,
          lambda o, ws, nb: L.vkn_panoptic_thing_first_u8(p(d[0]), p(d[1]), p(d[2]), p(d[3]), Kt, p(d[4]), p(d[5]), p(d[6]), Ks, HW,
                                                          float(thr['instance_score_thr']), float(thr['iou_thr']), int(thr['stuff_max_area']), o['seg'],
                                                          o['info'], o['nseg'], ws, nb, st()), align_code=E_WORKSPACE)
    if Kt + Ks:
        assert np.array_equal(c.out['info'].cpu().numpy(), r['info'])


@pytest.mark.parametrize('max_norm', [0.0, 1.0], ids=['noclip', 'clip'])
def test_adamw_flat(vkn, max_norm):
    """vkn_adamw_flat_f32 over three work items (two chunks of one parameter — one of them ragged against the workgroup — and a parameter
    without a gradient): param / exp_avg / exp_avg_sq are updated in place inside the arena, the gradient is only read, the inactive
    parameter keeps its bits, the workspace is exactly vkn_adamw_workspace_bytes"""
    L, lib = _lib(vkn), vkn._lib
    f32 = torch.float32
    ns, pidx = (1024, 36, 8), (0, 0, 1)
    g = torch.Generator().manual_seed(3100)
    init = {k: [torch.randn(n, generator=g).abs().to(DEV) * sc for n in ns] for k, sc in (('p', 1.0), ('m', 0.1), ('v', 0.01))}
    grads = [torch.randn(n, generator=g).to(DEV) for n in ns]
    rows = torch.tensor([[1e-3, 0.05, 0.9, 0.999, 1e-8]], dtype=torch.float64, device=DEV)
    active = torch.tensor([1, 0], dtype=torch.uint8, device=DEV)
    need = L.vkn_adamw_workspace_bytes(3, 2, 1)
    assert need > 0
    outs = {f'{k}{i}': ((n,), f32) for k in 'pmv' for i, n in enumerate(ns)}
    outs.update(steps=((2,), torch.int32), norm=((1,), f32, dict(full=bool(max_norm))), coef=((1,), f32))
    keep = []

    def fill(o):
        for k in 'pmv':
            for i in range(3):
                o[f'{k}{i}'].copy_(init[k][i])
        o['steps'].copy_(torch.tensor([4, 9], dtype=torch.int32))

    def call(o, ws, nb):
        arr = (lib.VknAdamwItem * 3)(*[lib.VknAdamwItem(o[f'p{i}'].value, grads[i].data_ptr(), o[f'm{i}'].value, o[f'v{i}'].value, ns[i], pidx[i], 0, 0)
                                       for i in range(3)])
        items = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)
        keep.append(items)
        return L.vkn_adamw_flat_f32(p(items), 3, 2, p(rows), 1, o['steps'], p(active), max_norm, o['norm'], o['coef'], ws, nb, st())
    c = Call(vkn, 'vkn_adamw_flat_f32', f'adamw max_norm={max_norm}', outs, need, call, inputs=grads + [rows, active], pre=fill, ws_align=16)
    assert c.out['steps'].tolist() == [5, 9]
    for k in 'pmv':
        assert torch.equal(c.out[f'{k}2'], init[k][2]), 'a parameter without a gradient was touched'
        assert not torch.equal(c.out[f'{k}0'], init[k][0]) and not torch.equal(c.out[f'{k}1'], init[k][1])
    if max_norm:
        want = float(torch.cat(grads[:2]).double().norm())
        assert float(c.out['norm']) == float(torch.tensor(want, dtype=torch.float32)), 'the norm is an fp64 sum rounded once'


# ====================================================================================================== backward glue, ground truth
def test_backward_glue(vkn):
    """vkn_pow2_scale_f32, vkn_scale_pad_rows_f32, vkn_transpose_pad_f32, vkn_threshold_rows_f16, vkn_unscale_rows_f32 and
    vkn_check_range_i64 on ragged sizes (odd P: the element-wise arms; P % 4 == 0: the vector arms).  Every value is a power-of-two
    multiple or a 0 / 1: exact, compared with torch bit for bit; padding rows and columns are zero, nothing lies behind them"""
    L = _lib(vkn)
    f32 = torch.float32
    for (B, R, P) in ((2, 33, 135), (1, 117, 128), (3, 1, 1)):
        g = ec.gen(2900 + P)
        t = ec.ints((B, R, P), -8, 8, g).to(DEV) * 2.0 ** -20
        t[0, 0, 0] = 5 * 2.0 ** -20
        c = Call(vkn, 'vkn_pow2_scale_f32', f'pow2_scale {B}x{R}x{P}', dict(s8=((8,), f32, dict(full=False)), scratch=((2,), torch.int32)), None,
                 lambda o, ws, nb: L.vkn_pow2_scale_f32(p(t), t.numel(), 10, o['s8'], o['scratch'], st()), inputs=(t,), pre=lambda o: o['scratch'].zero_())
        want = ec.pow2_scale_of(t.cpu())
        assert float(c.out['s8'][0]) == want and float(c.out['s8'][4]) == 1.0 / want and c.out['scratch'].tolist() == [0, 0], (c.out['s8'], want)
        scale = c.out['s8'][0:1]
        Rp = (R + 31) // 32 * 32
        c = Call(vkn, 'vkn_scale_pad_rows_f32', f'scale_pad_rows {B}x{R}x{P}', dict(out=((B, Rp, P), f32)), None,
                 lambda o, ws, nb: L.vkn_scale_pad_rows_f32(p(t), p(scale), B, R, Rp, P, o['out'], st()), inputs=(t, scale))
        assert torch.equal(c.out['out'][:, :R], t * want) and int(c.out['out'][:, R:].count_nonzero()) == 0
        z = ec.mask_logits(B, R, P, g).to(DEV)
        c = Call(vkn, 'vkn_threshold_rows_f16', f'threshold_rows {B}x{R}x{P}', dict(rows=((B, Rp, P), torch.float16)), None,
                 lambda o, ws, nb: L.vkn_threshold_rows_f16(p(z), ec.THR, B, R, Rp, P, o['rows'], st()), inputs=(z,))
        assert torch.equal(c.out['rows'][:, :R], (z >= ec.THR).half()) and int(c.out['rows'][:, R:].count_nonzero()) == 0
        C = 64 if P > 1 else 36
        k = ec.ints((B, R, C), -8, 8, g).to(DEV)
        c = Call(vkn, 'vkn_transpose_pad_f32', f'transpose_pad {B}x{R}x{C}', dict(out=((B, C, Rp), f32)), None,
                 lambda o, ws, nb: L.vkn_transpose_pad_f32(p(k), p(scale), B, R, C, Rp, o['out'], st()), inputs=(k, scale))
        assert torch.equal(c.out['out'][:, :, :R], (k * want).transpose(1, 2)) and int(c.out['out'][:, :, R:].count_nonzero()) == 0
        dkp, dkbp = ec.ints((B, Rp, C), -8, 8, g).to(DEV), ec.ints((B, Rp), -8, 8, g).to(DEV)
        inv = c_inv = torch.full((1,), 1.0 / want, device=DEV)
        for with_b in (True, False):
            c = Call(vkn, 'vkn_unscale_rows_f32', f'unscale_rows {B}x{R}x{C} dkb={with_b}', dict(dk=((B, R, C), f32), dkb=((B, R), f32) if with_b else None), None,
                     lambda o, ws, nb: L.vkn_unscale_rows_f32(p(dkp), p(dkbp), p(inv), B, R, Rp, C, o['dk'], o['dkb'], st()), inputs=(dkp, dkbp, inv))
            assert torch.equal(c.out['dk'], dkp[:, :R] * c_inv)
            if with_b:
                assert torch.equal(c.out['dkb'], dkbp[:, :R] * c_inv)
    v = torch.arange(1001, dtype=torch.int64, device=DEV) % 5
    for bad, want in ((False, 0), (True, 2)):
        if bad:
            v[1000] = 5
        c = Call(vkn, 'vkn_check_range_i64', f'check_range bad={bad}', dict(status=((1,), torch.int32)), None,
                 lambda o, ws, nb: L.vkn_check_range_i64(p(v), v.numel(), 0, 5, 2, o['status'], st()), inputs=(v,), pre=lambda o: o['status'].zero_())
        assert int(c.out['status']) == want


@pytest.mark.parametrize('i64', [0, 1], ids=['u8', 'i64'])
def test_gt_classes(vkn, i64):
    """vkn_gt_classes: n_sem [B], flags [B][8], class lists and labels of exactly [B][256] (only the listed entries are written), status;
    against torch.unique over the valid part of every map"""
    L = _lib(vkn)
    B, Hp, Wp = 3, 9, 14
    g = ec.gen(3000)
    sem = torch.randint(0, 8, (B, Hp, Wp), generator=g)
    sem[sem == 7] = 255
    sem[1, 8, 13] = 6                                        # outside image 1's valid part: must not be listed
    sem[1][sem[1] == 6] = 5
    sem[1, 8, 13] = 6
    valid = [(9, 14), (7, 11), (0, 0)]
    table = [-1] * 256
    for c_ in range(2, 7):
        table[c_] = c_ + 10
    semd = sem.to(device=DEV, dtype=torch.int64 if i64 else torch.uint8).contiguous()
    step = Hp * Wp * semd.element_size()
    imgs = (vkn._lib.VknGtImage * B)(*[vkn._lib.VknGtImage(None, semd.data_ptr() + b * step, None, 0, 0, 0, vh, vw, 0, 0, 0) for b, (vh, vw) in enumerate(valid)])
    tab = (ctypes.c_int * 256)(*table)
    c = Call(vkn, 'vkn_gt_classes', f'gt_classes i64={i64}',
             dict(flags=((B, 8), torch.int32), n_sem=((B,), torch.int32), classes=((B, 256), torch.uint8, dict(full=False)),
                  labels=((B, 256), torch.int64, dict(full=False)), status=((1,), torch.int32)), None,
             lambda o, ws, nb: L.vkn_gt_classes(imgs, B, Hp, Wp, i64, tab, o['flags'], o['n_sem'], o['classes'], o['labels'], o['status'], st()),
             inputs=(semd,), pre=lambda o: o['status'].zero_())
    assert int(c.out['status']) == 0
    for b, (vh, vw) in enumerate(valid):
        listed = [int(v) for v in torch.unique(sem[b, :vh, :vw]).tolist() if table[int(v)] >= 0]
        assert int(c.out['n_sem'][b]) == len(listed), (b, listed)
        assert c.out['classes'][b, :len(listed)].tolist() == listed and c.out['labels'][b, :len(listed)].tolist() == [table[v] for v in listed]
    assert 6 not in c.out['classes'][1, :int(c.out['n_sem'][1])].tolist() and int(c.out['n_sem'][2]) == 0


def test_gt_match_indices(vkn):
    """vkn_gt_match_indices: match of exactly sum(key_len) and match_off of exactly B + 1 elements; `ref_ids.index(i) if i in ref_ids else -1`"""
    L = _lib(vkn)
    keys = [[3, 7, 7, 100], [], [5], list(range(40, 0, -1))]
    refs = [[7, 3, 7, 9], [1, 2], [], list(range(1, 80, 2)) + [40]]
    B = len(keys)
    kcat = torch.tensor([k for ks in keys for k in ks], dtype=torch.int64, device=DEV)
    rcat = torch.tensor([r for rs in refs for r in rs], dtype=torch.int64, device=DEV)
    klen, rlen = (ctypes.c_int * B)(*[len(k) for k in keys]), (ctypes.c_int * B)(*[len(r) for r in refs])
    c = Call(vkn, 'vkn_gt_match_indices', 'gt_match_indices', dict(match=((kcat.numel(),), torch.int64), off=((B + 1,), torch.int64)), None,
             lambda o, ws, nb: L.vkn_gt_match_indices(p(kcat), klen, p(rcat), rlen, B, o['match'], o['off'], st()), inputs=(kcat, rcat))
    want = [(rs.index(k) if k in rs else -1) for ks, rs in zip(keys, refs) for k in ks]
    assert c.out['match'].tolist() == want and c.out['off'].tolist() == [0, 4, 4, 5, 45]


# ====================================================================================================== gates
def _gate(vkn, name, outs, need, fn, align_code=None, null_code=E_WORKSPACE, out_align_code=E_ALIGN, first_out=None):
    """The argument checks of an entry with a `ws` argument are host arithmetic in front of every launch: a workspace one byte short and a
    NULL workspace are VKN_E_WORKSPACE; `ws + 4` is `align_code` (what the entry's code returns for it) and the output `first_out` at +4
    bytes `out_align_code` — and nothing is written."""
    assert need > 0, f'{name}: the size query answers 0 inside the envelope'
    A = Arena(DEV)
    rng = {k: A.out(sh, dt, name=k) for k, (sh, dt) in outs.items()}
    skew = {k: A.out(sh, dt, name=k + '+4', skew=4) for k, (sh, dt) in outs.items() if k == first_out}
    w = A.ws(need + 16, name='ws')
    o = {k: r.ptr for k, r in rng.items()}
    assert fn(o, w.ptr, need - 1) == E_WORKSPACE, f'{name}: ws_bytes = need - 1'
    assert fn(o, None, need) == null_code, f'{name}: ws = NULL'
    if align_code is not None:
        assert fn(o, ctypes.c_void_p(w.addr + 4), need) == align_code, f'{name}: ws + 4'
    for k, r in skew.items():
        assert fn(dict(o, **{k: r.ptr}), w.ptr, need) == out_align_code, f'{name}: {k} + 4'
    _untouched(A, name)


def test_gate_gather_decode_fused(vkn):
    L = _lib(vkn)
    s = ec.Shape(2, 33, 64, 8, 8, 2701, False)
    B, N, C, P = s.B, s.N, s.C, 64
    x, z, _, _ = ec.gather_case(s)
    xd, zd = _cuda(x, z)
    _, k, kb, _ = ec.decode_case(s)
    kd, kbd = _cuda(k, kb)
    hi, lo = vkn.ops.split_planes(kd)
    one = torch.ones(1, device=DEV)
    ng, nd = L.vkn_gather_workspace_bytes(B, N, C, P), L.vkn_decode_workspace_bytes(B, N, C)
    go = dict(xraw=((B, N, C), torch.float32), cnt=((B, N), torch.float32))
    do = dict(out=((B, N, 8, 8), torch.float32))
    # (`ws + 4`: VKN_E_WORKSPACE, in the same test as NULL and short — the planes and partial sums carved from it are read 16 bytes at a time)
    _gate(vkn, 'vkn_mask_gather_f32', go, ng, lambda o, ws, nb: L.vkn_mask_gather_f32(p(xd), p(zd), ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, 0, st()),
          align_code=E_WORKSPACE, first_out='xraw')
    _gate(vkn, 'vkn_mask_gather_real_f32', go, ng, lambda o, ws, nb: L.vkn_mask_gather_real_f32(p(xd), p(zd), o['xraw'], o['cnt'], B, N, C, P, ws, nb, st()),
          align_code=E_WORKSPACE, first_out='xraw')
    _gate(vkn, 'vkn_mask_decode_f32', do, nd, lambda o, ws, nb: L.vkn_mask_decode_f32(p(xd), p(kd), p(kbd), o['out'], B, N, C, P, ws, nb, 0, st()), align_code=E_WORKSPACE, first_out='out')
    _gate(vkn, 'vkn_mask_decode_scaled_f32', do, nd,
          lambda o, ws, nb: L.vkn_mask_decode_scaled_f32(p(xd), p(kd), p(kbd), p(one), o['out'], B, N, C, P, ws, nb, 0, st()), align_code=E_WORKSPACE, first_out='out')
    _gate(vkn, 'vkn_decode_gather_f32', go, ng,
          lambda o, ws, nb: L.vkn_decode_gather_f32(p(xd), p(hi), p(lo), p(kbd), ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, st()), align_code=E_WORKSPACE, first_out='xraw')
    _gate(vkn, 'vkn_decode_gather_x', go, ng,
          lambda o, ws, nb: L.vkn_decode_gather_x(p(xd), 0, p(hi), p(lo), p(kbd), ec.THR, o['xraw'], o['cnt'], B, N, C, P, ws, nb, st()), align_code=E_WORKSPACE, first_out='xraw')
    assert L.vkn_gather_workspace_bytes(0, N, C, P) == 0 and L.vkn_decode_workspace_bytes(B, 0, C) == 0


def test_gate_linear_init_conv_fpn(vkn):
    L = _lib(vkn)
    M, K, Nout, ks = 33, 512, 19, 2
    A_, W, b, _ = ec.linear_case(M, K, Nout, 2801)
    Ad, Wd, bd = _cuda(A_, W, b)
    _gate(vkn, 'vkn_linear_f32', dict(y=((M, Nout), torch.float32)), ks * M * Nout * 4,
          lambda o, ws, nb: L.vkn_linear_f32(p(Ad), p(Wd), None, p(bd), o['y'], M, K, Nout, 0, ks, ws, nb, st()), align_code=E_WORKSPACE)
    sh = ec.INIT_SHAPES[1]
    B, C, Np, ncls, nth, H, W_ = sh
    loc, sem, iw, sw, sb, _ = ec.init_case(*sh, 2802, True)
    ld, sd, iwd, swd, sbd = _cuda(loc, sem, iw, sw, sb)
    N, P = Np + ncls - nth, H * W_
    # (seg_preds NULL: they are then kept in the workspace, which is what the size query counts — with seg_preds given the call needs less)
    _gate(vkn, 'vkn_kernel_init_f32', dict(x_feats=((B, C, H, W_), torch.float32), mask_preds=((B, N, H, W_), torch.float32), prop=((B, N, C), torch.float32)),
          L.vkn_kernel_init_workspace_bytes(B, Np, ncls, C, P),
          lambda o, ws, nb: L.vkn_kernel_init_f32(p(ld), p(sd), p(iwd), p(swd), p(sbd), nth, 1, 1, ec.THR, o['x_feats'], o['mask_preds'], None,
                                                  o['prop'], B, Np, ncls, C, P, ws, nb, 0, st()), align_code=E_WORKSPACE, first_out='mask_preds')
    assert L.vkn_kernel_init_workspace_bytes(B, 0, ncls, C, P) == 0
    x, pos, w, _ = ec.conv_case(2, 32, 3, 5, 3, 1, 'raw', 2803)
    xd, wd = _cuda(x, w)
    img = vkn.ops.conv_prepare(wd)
    _gate(vkn, 'vkn_conv_gn_f32', dict(out=((2, 32, 3, 5), torch.float32), stats=((2, 32, 2), torch.float32)), L.vkn_conv_gn_workspace_bytes(2, 32, 3, 5, 1, 0),
          lambda o, ws, nb: L.vkn_conv_gn_f32(p(xd), None, None, None, None, 0, 0, p(img), 3, 1, 32, o['out'], o['stats'], 2, 32, 3, 5, 32, ws, nb, st()),
          align_code=E_ALIGN, first_out='out')
    assert L.vkn_conv_gn_workspace_bytes(0, 32, 3, 5, 1, 0) == 0 and L.vkn_conv_weight_bytes(32, 33, 3) == 0
    call, outs, _ = _fpn(vkn, 1, 64, FPN_LEVELS[0], rule=False)
    _gate(vkn, 'vkn_localization_fpn_f32', outs, L.vkn_localization_fpn_workspace_bytes(1, 64, 8, 8, 4, 4, 2, 2, 1, 1), call, align_code=E_ALIGN, first_out='loc')


def test_gate_stage_shaped_entries(vkn):
    """vkn_stage_* / vkn_head_* / link / updator / query merge: `ws` short, NULL or not 16-byte aligned is VKN_E_WORKSPACE (stage_ws and the
    head's own gate test all three in one line); an output at +4 is VKN_E_ALIGN"""
    L = _lib(vkn)
    g, case, head, (xd, pfd, mpd, prevd) = _head_of(vkn, 'video_tiny')
    B, N, C, H, W, up, ncls = case['B'], case['N'], case['C'], case['H'], case['W'], case['up'], case['ncls']
    dev = torch.device(DEV)
    dims = head.mask_head[0].make_dims(B, N, H, W)
    packs = [h.stage_pack(dev) for h in head.mask_head]
    for pk in packs:
        pk.ensure_prepared(dims)
    arr = (vkn._lib.VknStageWeights * len(packs))(*[pk.w for pk in packs])
    w = ctypes.byref(arr[len(packs) - 1])
    pf3, prev3 = pfd.reshape(B, N, C).contiguous(), prevd.reshape(B, N, C).contiguous()
    bnc = ((B, N, C), torch.float32)
    nh, ns = L.vkn_head_workspace_bytes(ctypes.byref(dims)), L.vkn_stage_workspace_bytes(ctypes.byref(dims))
    ho = dict(obj=bnc, cls=((B, N, ncls), torch.float32), masks=((B, N, H, W), torch.float32), scaled=((B, N, H * up, W * up), torch.float32), track=bnc)
    _gate(vkn, 'vkn_head_forward_f32', ho, nh,
          lambda o, ws, nb: L.vkn_head_forward_f32(ctypes.byref(dims), len(packs), arr, p(xd), p(pf3), p(mpd), p(prev3), o['obj'], o['cls'], o['masks'],
                                                   o['scaled'], up, o['track'], ws, nb, 0, st()), align_code=E_WORKSPACE, first_out='masks')
    _gate(vkn, 'vkn_head_forward_link_f32', ho, nh,
          lambda o, ws, nb: L.vkn_head_forward_link_f32(ctypes.byref(dims), len(packs), arr, None, None, 0, p(xd), p(pf3), p(mpd), p(prev3), o['obj'], o['cls'],
                                                        o['masks'], o['scaled'], up, o['track'], ws, nb, 0, st()), align_code=E_WORKSPACE, first_out='masks')
    _gate(vkn, 'vkn_head_forward_prof_f32', ho, nh,
          lambda o, ws, nb: L.vkn_head_forward_prof_f32(ctypes.byref(dims), len(packs), arr, p(xd), p(pf3), p(mpd), p(prev3), o['obj'], o['cls'], o['masks'],
                                                        o['scaled'], up, o['track'], ws, nb, 0, st(), None, None), align_code=E_WORKSPACE, first_out='masks')
    so = dict(cls=((B, N, ncls), torch.float32), masks=((B, N, H, W), torch.float32), obj=bnc, xfeat=bnc, track=bnc)
    _gate(vkn, 'vkn_stage_forward_link_f32', so, ns,
          lambda o, ws, nb: L.vkn_stage_forward_link_f32(ctypes.byref(dims), w, None, None, 0, p(xd), p(pf3), p(mpd), p(prev3), o['cls'], o['masks'], o['obj'],
                                                         o['xfeat'], o['track'], ws, nb, 0, st()), align_code=E_WORKSPACE, first_out='masks')
    _gate(vkn, 'vkn_stage_forward_f32', so, ns,
          lambda o, ws, nb: L.vkn_stage_forward_f32(ctypes.byref(dims), w, p(xd), p(pf3), p(mpd), p(prev3), o['cls'], o['masks'], o['obj'], o['xfeat'],
                                                    o['track'], ws, nb, 0, st()), align_code=E_WORKSPACE)
    _gate(vkn, 'vkn_stage_chain_f32', dict(cls=((B, N, ncls), torch.float32), kern=bnc, kb=((B, N), torch.float32), obj=bnc), ns,
          lambda o, ws, nb: L.vkn_stage_chain_f32(ctypes.byref(dims), w, p(pf3), p(pf3), o['cls'], o['kern'], o['kb'], o['obj'], ws, nb, 0, st()),
          align_code=E_WORKSPACE, first_out='kern')
    _gate(vkn, 'vkn_track_link_f32', dict(track=bnc), ns,
          lambda o, ws, nb: L.vkn_track_link_f32(ctypes.byref(dims), w, p(pf3), p(prev3), o['track'], ws, nb, st()), align_code=E_WORKSPACE, first_out='track')
    _gate(vkn, 'vkn_track_link_flags_f32', dict(track=bnc), ns,
          lambda o, ws, nb: L.vkn_track_link_flags_f32(ctypes.byref(dims), w, p(pf3), p(prev3), o['track'], ws, nb, 0, st()), align_code=E_WORKSPACE)
    _gate(vkn, 'vkn_link_block_f32', dict(out=bnc), ns,
          lambda o, ws, nb: L.vkn_link_block_f32(ctypes.byref(dims), w, p(pf3), p(pf3), p(prev3), o['out'], ws, nb, st()), align_code=E_WORKSPACE, first_out='out')
    _gate(vkn, 'vkn_kernel_updator_f32', dict(out=bnc), ns,
          lambda o, ws, nb: L.vkn_kernel_updator_f32(ctypes.byref(dims), w, p(pf3), p(prev3), o['out'], ws, nb, st()), align_code=E_WORKSPACE, first_out='out')
    bad = vkn.ops.make_dims(B, N, C + 1, H, W, case['heads'], case['ffn'], ncls, 1, 1)
    assert L.vkn_stage_workspace_bytes(ctypes.byref(bad)) == 0 and L.vkn_head_workspace_bytes(ctypes.byref(bad)) == 0
    A = Arena(DEV)
    hdr = A.ws(255, name='short header')
    assert L.vkn_workspace_init(hdr.ptr, 255, st()) == E_WORKSPACE and L.vkn_workspace_init(None, 256, st()) == E_WORKSPACE
    assert L.vkn_workspace_status(hdr.ptr, 255, st()) == E_WORKSPACE and L.vkn_workspace_status(None, 256, st()) == E_WORKSPACE
    _untouched(A, 'vkn_workspace_init / _status on a short header')


def test_gate_query_merge_panoptic_assign_tracker(vkn):
    from helpers import load_assign_golden, load_pan_golden, make_assign_case, make_pan_case
    from test_gpu_tracker import CFG
    L = _lib(vkn)
    B, N, C, F = 1, 10, 128, 2
    dims = vkn.ops.make_dims(B, N, C, 8, 8, 8, 8 * C, 1, 0, 0)
    q, k = torch.zeros(B, N, C, device=DEV), torch.zeros(B, F * N, C, device=DEV)
    # (the weight pointers are only read by kernels; every gate below returns before a launch.  vkn_query_merge_f32 checks its weights first:
    #  real ones)
    from oracle import synth
    shapes = {'query_merge_attn.attn.in_proj_weight': (3 * C, C), 'query_merge_attn.attn.in_proj_bias': (3 * C,),
              'query_merge_attn.attn.out_proj.weight': (C, C), 'query_merge_attn.attn.out_proj.bias': (C,),
              'query_merge_norm.weight': (C,), 'query_merge_norm.bias': (C,),
              'query_merge_ffn.layers.0.0.weight': (8 * C, C), 'query_merge_ffn.layers.0.0.bias': (8 * C,),
              'query_merge_ffn.layers.1.weight': (C, 8 * C), 'query_merge_ffn.layers.1.bias': (C,),
              'query_merge_ffn_norm.weight': (C,), 'query_merge_ffn_norm.bias': (C,)}
    named = {n_: torch.from_numpy(v).to(DEV) for n_, v in synth.state_dict_like(shapes, 77 + C).items()}
    pack = vkn.ops.link_pack(named, torch.device(DEV), None, 'query_merge_attn', 'query_merge_norm', 'query_merge_ffn', 'query_merge_ffn_norm')
    pack.ensure_prepared(dims)
    W = pack.w
    _gate(vkn, 'vkn_query_merge_f32', dict(out=((B, N, C), torch.float32)), L.vkn_query_merge_workspace_bytes(ctypes.byref(dims), F),
          lambda o, ws, nb: L.vkn_query_merge_f32(ctypes.byref(dims), F, ctypes.byref(W), p(q), p(k), None, o['out'], ws, nb, st()),
          align_code=E_WORKSPACE, first_out='out')
    # ---- panoptic
    g, case = load_pan_golden('pan_tiny')
    cls, logits, _ = make_pan_case(case)
    cls, logits = _cuda(cls, logits)
    cfg = _pan_cfg(vkn, case)
    Bp, Np_, K = case['B'], case['N'], case['N']
    _gate(vkn, 'vkn_panoptic_joint_f32', dict(seg=((Bp, case['Ho'], case['Wo']), torch.int32), info=((Bp, K, 6), torch.int32), nseg=((Bp,), torch.int32),
                                              bbox=((Bp, K, 4), torch.int32)), L.vkn_panoptic_workspace_bytes(ctypes.byref(cfg), Bp, Np_),
          lambda o, ws, nb: L.vkn_panoptic_joint_f32(ctypes.byref(cfg), p(cls), p(logits), Bp, Np_, case['ncls'], o['seg'], o['info'], o['nseg'], o['bbox'],
                                                     ws, nb, st()), align_code=E_WORKSPACE)
    assert L.vkn_panoptic_workspace_bytes(ctypes.byref(cfg), 0, Np_) == 0
    # ---- assignment costs (a misaligned `ws` is VKN_E_ALIGN there: csrc/vkn_assign.hip tests the three pointers together, before the size)
    ga, ca = load_assign_golden('assign_tiny')
    Na, G, nca, Pa = ca['N'], ca['G'], ca['ncls'], ca['H'] * ca['W']
    lg, cl, gt, lab = _cuda(*make_assign_case(ca))
    lg, gt, lab = lg.reshape(Na, Pa).contiguous(), gt.reshape(G, Pa).float().contiguous(), lab.to(torch.int32)
    acfg = vkn._lib.VknAssignCfg(*ASSIGN_CFG)
    na = L.vkn_assign_workspace_bytes(Na, G, Pa)
    _gate(vkn, 'vkn_assign_costs_f32', dict(cost=((Na, G), torch.float32)), na,
          lambda o, ws, nb: L.vkn_assign_costs_f32(ctypes.byref(acfg), p(lg), p(cl), p(gt), p(lab), Na, G, nca, Pa, o['cost'], ws, nb, st()), align_code=E_ALIGN)

    def batch(o, ws, nb):
        probs = (vkn._lib.VknAssignProblem * 1)(vkn._lib.VknAssignProblem(lg.data_ptr(), cl.data_ptr(), gt.data_ptr(), lab.data_ptr(), G, o['cost'].value))
        return L.vkn_assign_costs_batch_f32(ctypes.byref(acfg), probs, 1, Na, nca, Pa, ws, nb, st())
    _gate(vkn, 'vkn_assign_costs_batch_f32', dict(cost=((Na, G), torch.float32)), na, batch, align_code=E_ALIGN)
    import test_gpu_assign_lowres as T
    Nl, Gs, ncl_, h, w, S, soft = T.CASES[6]
    lows, clss, gts, labs = T._case(Nl, Gs, ncl_, h, w, S, 11, soft)
    dl, dc, dg = lows[0][:Nl].contiguous().to(DEV), clss[0].to(DEV), gts[0].float().contiguous().to(DEV)
    dlab = labs[0].to(device=DEV, dtype=torch.int32)

    def lowres(o, ws, nb):
        probs = (vkn._lib.VknAssignProblem * 1)(vkn._lib.VknAssignProblem(dl.data_ptr(), dc.data_ptr(), dg.data_ptr(), dlab.data_ptr(), Gs[0], o['cost'].value))
        return L.vkn_assign_costs_lowres_batch_f32(ctypes.byref(acfg), probs, 1, Nl, ncl_, h, w, S, ws, nb, st())
    _gate(vkn, 'vkn_assign_costs_lowres_batch_f32', dict(cost=((Nl, Gs[0]), torch.float32)), L.vkn_assign_lowres_workspace_bytes(1, Nl, Gs[0], h, w, S), lowres,
          align_code=E_WORKSPACE)
    assert L.vkn_assign_lowres_workspace_bytes(1, Nl, Gs[0], h, w, 3) == 0 and L.vkn_assign_lowres_workspace_bytes(17, Nl, Gs[0], h, w, S) == 0
    # ---- tracker: ws short / NULL is VKN_E_WORKSPACE, `state` or `ws` off a 256-byte boundary VKN_E_ALIGN; outside the envelope the queries answer 0
    trk = vkn.build_tracker(dict(CFG, type='QuasiDenseEmbedTracker', max_dets=16, max_tracklets=8))
    tc = trk._make_cfg(32)
    nstate, nws = L.vkn_qd_tracker_state_bytes(ctypes.byref(tc)), L.vkn_qd_tracker_workspace_bytes(ctypes.byref(tc))
    state = torch.zeros(nstate, dtype=torch.uint8, device=DEV)
    bb, lb, em = torch.zeros(4, 5, device=DEV), torch.zeros(4, dtype=torch.int64, device=DEV), torch.zeros(4, 32, device=DEV)
    _gate(vkn, 'vkn_qd_tracker_match_f32', dict(ob=((16, 5), torch.float32), ol=((16,), torch.int64), oi=((16,), torch.int64), oc=((2,), torch.int32)), nws,
          lambda o, ws, nb: L.vkn_qd_tracker_match_f32(ctypes.byref(tc), p(state), nstate, p(bb), p(lb), p(em), 4, 0, o['ob'], o['ol'], o['oi'], o['oc'], ws, nb, st()),
          align_code=E_ALIGN)
    wide = trk._make_cfg(2048)
    assert L.vkn_qd_tracker_state_bytes(ctypes.byref(wide)) == 0 and L.vkn_qd_tracker_workspace_bytes(ctypes.byref(wide)) == 0
