"""GPU: the linear kernels BIT FOR BIT against float64, on integer-valued operands (tests/exact_cases.py).

Small integers (dyadic fractions) are exact in the high term of every operand split this library uses, every partial sum stays below
2^24 (asserted per case from the actual operands before anything is launched), so fp32 accumulation is exact in any order and the HIP
result must EQUAL the reference: no tolerance anywhere in this file.  One dropped, doubled or misplaced pixel, channel or row at a
tile edge is a hard failure, and the message names the count of wrong elements and the first indices.

The shape sweep covers every pair (N edge, P edge) at C = 64 and C = 256, every C, every B, ragged P as 1 x P and as H x W with odd W,
and the two frame-sized P once per op.  Where an entry point documents that it declines a shape (include/vkn.h), the test asserts
VKN_E_SHAPE instead of skipping.  After each group the workspace's range flag must be clear (`workspace_status`)."""
import re

import pytest
import torch

import exact_cases as ec

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_SHAPE, E_ALIGN = -2, -5          # VKN_E_SHAPE, VKN_E_ALIGN (include/vkn.h)
SWEEP = ec.bncp_sweep()
GROUPS = {'C64': [s for s in SWEEP if s.C == 64], 'C256': [s for s in SWEEP if s.C == 256 and not s.large],
          'otherC': [s for s in SWEEP if s.C not in (64, 256)], 'large': [s for s in SWEEP if s.large]}


def _diff(name, got, want):
    """None when `got` (device tensor) equals the float64 reference `want` bit for bit, else the failure line"""
    g = got.detach().cpu()
    w = want.reshape(g.shape).to(g.dtype)
    assert torch.equal(w.double(), want.reshape(g.shape).double()), f'{name}: the reference is not representable in {g.dtype} (test bug)'
    if torch.equal(g, w):
        return None
    bad = g != w
    idx = bad.nonzero()[:6]
    first = ', '.join(f'{tuple(i.tolist())}: got {g[tuple(i)].item()!r} want {w[tuple(i)].item()!r}' for i in idx[:3])
    return f'{name}: {int(bad.sum())} of {bad.numel()} elements wrong, first indices {idx.tolist()} ({first})'


def _declines(vkn, fn):
    """the call is refused with VKN_E_SHAPE"""
    with pytest.raises(vkn.VknError) as e:
        fn()
    return e.value.code == E_SHAPE


def _finish(vkn, fails):
    torch.cuda.synchronize()
    vkn.ops.workspace_status()                      # raises VknError(VKN_E_RANGE) when a kernel flagged the f16-split envelope
    assert not fails, f'{len(fails)} mismatches:\n' + '\n'.join(fails[:40])


def _cuda(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


def _run_and_events(fn):
    """fn()'s result and the names of the device kernels it launched, one entry per launch (torch.profiler sees the library's launches)"""
    from torch.profiler import ProfilerActivity, profile
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        out = fn()
        torch.cuda.synchronize()
    cuda = getattr(torch.autograd, 'DeviceType', None)
    evs = [e for e in prof.events() if cuda is None or getattr(e, 'device_type', None) == cuda.CUDA]
    return out, [e.name for e in evs]


def _launches(names, kernel):
    """launches of exactly this kernel (`k_upsample` does not count `k_upsample_s`), demangled or mangled names"""
    rx = re.compile(re.escape(kernel) + r'(?![_a-z0-9])')
    return sum(1 for n in names if rx.search(n))


# ------------------------------------------------------------------------------------------------------------------- gather
@pytest.mark.parametrize('group', list(GROUPS))
@pytest.mark.parametrize('flags', [0, 1], ids=['mfma', 'ref_kernels'])
def test_mask_gather(vkn, group, flags):
    fails = []
    for s in GROUPS[group]:
        x, z, xraw, cnt = ec.gather_case(s)
        a, c = vkn.ops.mask_gather(*_cuda(x, z), flags=flags)
        fails += [f for f in (_diff(f'gather flags={flags} {ec.sid(s)} xraw[b, n, c]', a, xraw),
                              _diff(f'gather flags={flags} {ec.sid(s)} cnt[b, n]', c, cnt)) if f]
    _finish(vkn, fails)


@pytest.mark.parametrize('group', list(GROUPS))
def test_mask_gather_real(vkn, group):
    fails = []
    for s in GROUPS[group]:
        for denom in ((1,) if s.large else (1, 16)):
            x, a, out, asum = ec.gather_real_case(s, denom)
            o, su = vkn.ops.mask_gather_real(*_cuda(x, a))
            fails += [f for f in (_diff(f'gather_real a=k/{denom} {ec.sid(s)} out[b, n, c]', o, out),
                                  _diff(f'gather_real a=k/{denom} {ec.sid(s)} asum[b, n]', su, asum)) if f]
    _finish(vkn, fails)


# ------------------------------------------------------------------------------------------------------------------- decode
@pytest.mark.parametrize('group', list(GROUPS))
def test_mask_decode(vkn, group):
    """mask_decode with the MFMA and the reference kernels, with and without bias; split_planes (hi == K exactly, lo == 0 exactly) +
    mask_decode_planes; the scaled decode with out_scale = 2^-7 and 2^9.  Odd P: mask_decode takes the reference kernel, the planes
    and the scaled entry points decline (VKN_E_SHAPE)."""
    ops = vkn.ops
    fails = []
    for s in GROUPS[group]:
        P, tag = s.H * s.W, ec.sid(s)
        x, k, kb, out = ec.decode_case(s)
        xd, kd, kbd = _cuda(x, k, kb)
        nobias = out - kb.double()[..., None, None]
        fails.append(_diff(f'decode mfma bias {tag} [b, n, y, x]', ops.mask_decode(xd, kd, kbd), out))
        fails.append(_diff(f'decode mfma nobias {tag} [b, n, y, x]', ops.mask_decode(xd, kd), nobias))
        fails.append(_diff(f'decode ref bias {tag} [b, n, y, x]', ops.mask_decode(xd, kd, kbd, flags=ops.FLAG_REF_KERNELS), out))
        if not s.large:
            fails.append(_diff(f'decode ref nobias {tag} [b, n, y, x]', ops.mask_decode(xd, kd, flags=ops.FLAG_REF_KERNELS), nobias))
        hi, lo = ops.split_planes(kd)
        fails.append(_diff(f'split_planes hi {tag} [b, n, c]', hi[:, :s.N].float(), k.double()))
        assert int(lo.count_nonzero()) == 0 and int(hi[:, s.N:].count_nonzero()) == 0, f'split_planes {tag}: lo / padding rows not exactly zero'
        if P % 2 == 0:
            fails.append(_diff(f'decode planes bias {tag} [b, n, y, x]', ops.mask_decode_planes(xd, hi, lo, s.N, kbd), out))
            fails.append(_diff(f'decode planes nobias {tag} [b, n, y, x]', ops.mask_decode_planes(xd, hi, lo, s.N), nobias))
            for e in (-7, 9):
                sc = torch.tensor(2.0 ** e, device=DEV)
                fails.append(_diff(f'decode scaled 2^{e} {tag} [b, n, y, x]', ops.mask_decode(xd, kd, kbd, out_scale=sc), out * 2.0 ** e))
        else:
            assert _declines(vkn, lambda: ops.mask_decode_planes(xd, hi, lo, s.N, kbd)), f'planes decode, odd P: {tag}'
            assert _declines(vkn, lambda: ops.mask_decode(xd, kd, kbd, out_scale=torch.tensor(0.5, device=DEV))), f'scaled decode, odd P: {tag}'
    _finish(vkn, [f for f in fails if f])


@pytest.mark.parametrize('B,znb', [(1, 1), (65, 2), (129, 0)], ids=['one_nblock', 'two_nblocks', 'off'])
def test_mask_decode_row_split(vkn, B, znb):
    """The few-frame row split of the decode launcher (rows over blockIdx.z) at N = 100, C = 32, P = 128: one workgroup per frame, so
    B = 1 runs one n-block per workgroup (B G2 <= 64), B = 65 two (<= 128), B = 129 none (four n-blocks, no split).  The sweep above
    reaches the first form only.  Which form ran is read off the launch itself: the n-blocks per workgroup are the first template
    argument of the k_decode_mfma instantiation the profiler saw, so a change of the launcher's thresholds fails here."""
    ops = vkn.ops
    s = ec.Shape(B, 100, 32, 8, 16, 2000 + B, False)
    x, k, kb, out = ec.decode_case(s)
    xd, kd, kbd = _cuda(x, k, kb)
    hi, lo = ops.split_planes(kd)
    got, names = _run_and_events(lambda: ops.mask_decode_planes(xd, hi, lo, s.N, kbd))
    nbs = [int(m.group(1)) for m in (re.search(r'k_decode_mfma(?:<|ILi)(\d+)', n) for n in names) if m]
    assert nbs == [znb or 4], (nbs, sorted(set(names)))                    # one launch (N <= 128) of that many n-blocks per workgroup
    fails = [_diff(f'decode planes bias {ec.sid(s)} [b, n, y, x]', got, out),
             _diff(f'decode planes nobias {ec.sid(s)} [b, n, y, x]', ops.mask_decode_planes(xd, hi, lo, s.N), out - kb.double()[..., None, None]),
             _diff(f'decode scaled 2^-7 {ec.sid(s)} [b, n, y, x]', ops.mask_decode(xd, kd, kbd, out_scale=torch.tensor(2.0 ** -7, device=DEV)), out * 2.0 ** -7)]
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- fused pass
@pytest.mark.parametrize('group', list(GROUPS))
def test_decode_gather(vkn, group):
    """decode -> threshold -> gather in one pass: cnt and xraw exact, no flip budget (an integer logit is never near thr_logit)"""
    ops = vkn.ops
    fails, ran, declined = [], 0, 0
    for s in GROUPS[group]:
        P, tag = s.H * s.W, ec.sid(s)
        x, k, kb, z, xraw, cnt = ec.fused_case(s)
        xd, kd, kbd = _cuda(x, k, kb)
        hi, lo = ops.split_planes(kd)
        if vkn._lib.lib().vkn_decode_gather_supported(s.C, P):
            assert s.C in (64, 128, 256) and P % 64 == 0
            a, c = ops.decode_gather(xd, hi, lo, s.N, kbd)
            fails += [_diff(f'fused {tag} xraw[b, n, c]', a, xraw), _diff(f'fused {tag} cnt[b, n]', c, cnt)]
            ran += 1
        else:
            assert _declines(vkn, lambda: ops.decode_gather(xd, hi, lo, s.N, kbd)), f'fused pass outside its envelope: {tag}'
            declined += 1
            # the two-kernel chain it stands for, on the same operands
            zz = ops.mask_decode(xd, kd, kbd)
            a, c = ops.mask_gather(xd, zz)
            fails += [_diff(f'decode+gather {tag} logits[b, n, y, x]', zz, z), _diff(f'decode+gather {tag} xraw[b, n, c]', a, xraw),
                      _diff(f'decode+gather {tag} cnt[b, n]', c, cnt)]
    assert ran + declined == len(GROUPS[group]) and (ran > 0 if group == 'large' else ran > 0 and declined > 0)
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- half-storage x
@pytest.mark.parametrize('dt', [torch.float16, torch.bfloat16], ids=['fp16', 'bf16'])
def test_half_storage_x(vkn, dt):
    """x stored as fp16 / bf16 (integers up to 256 are exact in both): gather, decode, planes decode and the fused pass"""
    ops = vkn.ops
    fails, ran = [], 0
    for s in [s for s in SWEEP if (s.H * s.W) % 64 == 0]:
        tag = f'{ec.sid(s)} {dt}'
        x, z, xraw, cnt = ec.gather_case(s, x_span=256)
        a, c = ops.mask_gather(x.to(DEV).to(dt), z.to(DEV))
        fails += [_diff(f'gather {tag} xraw[b, n, c]', a, xraw), _diff(f'gather {tag} cnt[b, n]', c, cnt)]
        x, k, kb, out = ec.decode_case(s, x_span=256)
        xh, kd, kbd = x.to(DEV).to(dt), k.to(DEV), kb.to(DEV)
        fails.append(_diff(f'decode {tag} [b, n, y, x]', ops.mask_decode(xh, kd, kbd), out))
        hi, lo = ops.split_planes(kd)
        fails.append(_diff(f'decode planes {tag} [b, n, y, x]', ops.mask_decode_planes(xh, hi, lo, s.N, kbd), out))
        if vkn._lib.lib().vkn_decode_gather_supported(s.C, s.H * s.W):
            x, k, kb, z, xraw, cnt = ec.fused_case(s, x_span=256)
            hi, lo = ops.split_planes(k.to(DEV))
            a, c = ops.decode_gather(x.to(DEV).to(dt), hi, lo, s.N, kb.to(DEV))
            fails += [_diff(f'fused {tag} xraw[b, n, c]', a, xraw), _diff(f'fused {tag} cnt[b, n]', c, cnt)]
        ran += 1
    assert ran >= 40
    s = next(s for s in SWEEP if s.H * s.W == 130 and s.N == 117)                    # half-storage x needs whole 64-pixel tiles
    x, z, _, _ = ec.gather_case(s)
    assert _declines(vkn, lambda: ops.mask_gather(x.to(DEV).to(dt), z.to(DEV)))
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- kernel-init pass
@pytest.mark.parametrize('cat', [False, True], ids=['nocat', 'cat'])
@pytest.mark.parametrize('use_binary', [True, False], ids=['binary', 'soft'])
@pytest.mark.parametrize('separate', [False, True], ids=['onepass', 'separate'])
def test_kernel_init(vkn, cat, use_binary, separate):
    """the outputs of pass 0 that are linear (x_feats, mask_preds, seg_preds) or linear -> threshold -> linear (proposal_feats with
    use_binary=True) in the operands; the soft gather weights (use_binary=False) are not, and stay with test_gpu_parity.py"""
    ops = vkn.ops
    fails = []
    for i, sh in enumerate(ec.INIT_SHAPES):
        loc, sem, iw, sw, sb, ref = ec.init_case(*sh, 1400 + i, cat)
        prop, xf, mp, seg = ops.kernel_init(*_cuda(loc, sem, iw, sw, sb), sh[4], cat, True, use_binary=use_binary,
                                            flags=ops.FLAG_INIT_SEPARATE if separate else 0)
        tag = f'init {sh} cat={cat} binary={use_binary} separate={separate}'
        fails += [_diff(f'{tag} x_feats[b, c, y, x]', xf, ref['x_feats']), _diff(f'{tag} mask_preds[b, n, y, x]', mp, ref['mask_preds']),
                  _diff(f'{tag} seg_preds[b, n, y, x]', seg, ref['seg_preds'])]
        if use_binary:
            fails.append(_diff(f'{tag} proposal_feats[b, n, c]', prop, ref['prop']))
        elif cat:                                       # the stuff rows are copies of conv_seg.weight whatever the gather weights
            Np = sh[2]
            fails.append(_diff(f'{tag} proposal_feats[b, Np:, c]', prop[:, Np:], ref['prop'][:, Np:]))
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- up-scaling
def _abi_upsample_code(vkn, m, S, offset_floats):
    """return code of vkn_upsample_bilinear_f32 through the C ABI with an output pointer `offset_floats` floats behind a 16-byte
    boundary; whatever the code, nothing may be written outside the output"""
    B, N, H, W = m.shape
    n = B * N * H * S * W * S
    buf = torch.zeros(n + 8, dtype=torch.float32, device=m.device)
    assert buf.data_ptr() % 16 == 0
    out = buf[offset_floats:offset_floats + n]
    rc = vkn._lib.lib().vkn_upsample_bilinear_f32(vkn.ops._ptr(m), vkn.ops._ptr(out), B * N, H, W, S, vkn.ops._stream())
    torch.cuda.synchronize()
    assert int(buf[:offset_floats].count_nonzero()) == 0 and int(buf[offset_floats + n:].count_nonzero()) == 0, 'wrote outside its output'
    return rc, out.view(B, N, H * S, W * S)


def test_upsample_forward(vkn):
    """x2 / x4 into fp32 — the staged kernel where W S % 4 == 0, the generic one otherwise — and into fp16 (declined where
    W S % 4 != 0).  The forward entry point holds every pointer to the header's 16-byte rule: an output pointer 8 bytes off is refused
    with VKN_E_ALIGN and nothing is written, so the generic kernel is reached through ragged widths only."""
    ops = vkn.ops
    fails = []
    for i, (B, N, H, W, S) in enumerate(ec.UP_FWD):
        m, out = ec.up_case(B, N, H, W, S, 700 + i, f16=True)
        md = m.to(DEV)
        tag = f'up x{S} {B}x{N}x{H}x{W}'
        fails.append(_diff(f'{tag} fp32 [b, n, y, x]', ops.upsample_bilinear(md, S), out))
        rc, got = _abi_upsample_code(vkn, md, S, 0)
        assert rc == 0
        fails.append(_diff(f'{tag} fp32 through the C ABI [b, n, y, x]', got, out))
        rc, got = _abi_upsample_code(vkn, md, S, 2)
        assert rc == E_ALIGN and int(got.count_nonzero()) == 0, (tag, rc)
        if (W * S) % 4 == 0:
            fails.append(_diff(f'{tag} fp16 [b, n, y, x]', ops.upsample_bilinear(md, S, out_f16=True), out))
        else:
            assert _declines(vkn, lambda: ops.upsample_bilinear(md, S, out_f16=True)), tag
    _finish(vkn, [f for f in fails if f])


def _abi_upsample_bwd(vkn, go, S, offset_floats):
    B, N, OH, OW = go.shape
    H, W = OH // S, OW // S
    buf = torch.zeros(go.numel() + 8, dtype=torch.float32, device=go.device)
    src = buf[offset_floats:offset_floats + go.numel()]
    src.copy_(go.reshape(-1))
    out = torch.empty((B, N, H, W), dtype=torch.float32, device=go.device)
    vkn._lib.check(vkn._lib.lib().vkn_upsample_bilinear_bwd_f32(vkn.ops._ptr(src), vkn.ops._ptr(out), B * N, H, W, S, vkn.ops._stream()))
    return out


def test_upsample_backward(vkn):
    """the adjoint at S = 1, 2, 4, 8: the W % 64 == 0 kernels of S = 2 / 4 and the generic one (every such case also through a
    grad_out pointer 4 bytes off, which only the generic kernel takes); any other S is declined"""
    fails = []
    for i, (B, N, H, W, S) in enumerate(ec.UP_BWD):
        go, gin = ec.up_bwd_case(B, N, H, W, S, 800 + i)
        gd = go.to(DEV)
        tag = f'up_bwd x{S} {B}x{N}x{H}x{W}'
        fails.append(_diff(f'{tag} [b, n, y, x]', vkn.ops.upsample_bilinear_bwd(gd, S), gin))
        fails.append(_diff(f'{tag}, grad_out 4 bytes off [b, n, y, x]', _abi_upsample_bwd(vkn, gd, S, 1), gin))
    assert _declines(vkn, lambda: vkn.ops.upsample_bilinear_bwd(torch.zeros(1, 1, 5, 5, device=DEV), 5))
    _finish(vkn, [f for f in fails if f])


def test_upsample_many_planes(vkn):
    """planes = 32768 + 5: the second iteration of each launcher's chunk loop (its pointer arithmetic has never run otherwise); the
    profiler must see every kernel launched at least twice"""
    ops = vkn.ops
    fails = []
    seen = dict(staged=0, generic=0, f16=0, bwd=0, bwd_w64=0)
    for i, (planes, H, W) in enumerate(ec.UP_PLANES):
        for S in (2, 4):
            m, out = ec.up_case(1, planes, H, W, S, 900 + i, f16=True)
            md = m.to(DEV)
            tag = f'up x{S} {planes} planes of {H}x{W}'
            got, names = _run_and_events(lambda: ops.upsample_bilinear(md, S))
            fails.append(_diff(f'{tag} fp32 [_, plane, y, x]', got, out))
            kind = 'staged' if (W * S) % 4 == 0 else 'generic'
            n = _launches(names, 'k_upsample_s' if kind == 'staged' else 'k_upsample')
            assert n >= 2, (tag, kind, n, sorted(set(names)))
            seen[kind] += 1
            if (W * S) % 4 == 0:
                got, names = _run_and_events(lambda: ops.upsample_bilinear(md, S, out_f16=True))
                fails.append(_diff(f'{tag} fp16 [_, plane, y, x]', got, out))
                assert _launches(names, 'k_upsample_s') >= 2, (tag, sorted(set(names)))
                seen['f16'] += 1
            go, gin = ec.up_bwd_case(1, planes, H, W, S, 950 + i)
            gd = go.to(DEV)
            got, names = _run_and_events(lambda: ops.upsample_bilinear_bwd(gd, S))
            fails.append(_diff(f'up_bwd x{S} {planes} planes of {H}x{W} [_, plane, y, x]', got, gin))
            assert _launches(names, 'k_upsample_bwd') >= 2, (tag, sorted(set(names)))
            seen['bwd'] += 1
    for S, kern in ((2, 'k_upsample_bwd2'), (4, 'k_upsample_bwd4')):       # the W % 64 == 0 adjoint kernels have a chunk loop of their own
        go, gin = ec.up_bwd_case(1, 32768 + 5, 1, 64, S, 990 + S)
        gd = go.to(DEV)
        got, names = _run_and_events(lambda: ops.upsample_bilinear_bwd(gd, S))
        fails.append(_diff(f'up_bwd x{S} 32773 planes of 1x64 [_, plane, y, x]', got, gin))
        assert _launches(names, kern) >= 2, (kern, sorted(set(names)))
        seen['bwd_w64'] += 1
    assert all(v > 0 for v in seen.values()), seen
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- autograd
def test_autograd_of_decode_and_gather(vkn):
    """gradients w.r.t. x, kernels and bias under an integer upstream gradient: the power-of-two scaling inside must cancel exactly"""
    ag = vkn.autograd
    fails = []
    for s in ec.GRAD_SHAPES:
        tag = ec.sid(s)
        x, k, kb, dz, dx, dk, dkb = ec.decode_grad_case(s)
        xd, kd, kbd = (t.to(DEV).requires_grad_(True) for t in (x, k, kb))
        ag.mask_decode(xd, kd, kbd).backward(dz.to(DEV))
        fails += [_diff(f'decode grad x {tag} [b, c, y, x]', xd.grad, dx), _diff(f'decode grad kernels {tag} [b, n, c]', kd.grad, dk),
                  _diff(f'decode grad bias {tag} [b, n]', kbd.grad, dkb)]
        x, z, d, dx = ec.gather_grad_case(s)
        xd = x.to(DEV).requires_grad_(True)
        xraw, cnt = ag.mask_gather(xd, z.to(DEV))
        xraw.backward(d.to(DEV))
        fails.append(_diff(f'gather grad x {tag} [b, c, y, x]', xd.grad, dx))
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- GEMM engine
def test_ops_linear_every_arithmetic(vkn):
    """ops.linear: exact-fp32 MFMA, the bf16x3 split, and the split-K forms (Nout <= 256), act 0 / 1"""
    ops = vkn.ops
    fails = []
    for i, (M, K, Nout) in enumerate(ec.gemm_shapes()):
        act = i % 2
        A, W, b, y = ec.linear_case(M, K, Nout, 1100 + i, act=act)
        Ad, Wd, bd = _cuda(A, W, b)
        tag = f'M{M} K{K} N{Nout} act{act} y[m, n]'
        fails.append(_diff(f'linear exact {tag}', ops.linear(Ad, Wd, bd, act=act), y))
        img = ops.split_weight(Wd)
        fails.append(_diff(f'linear bf16x3 {tag}', ops.linear(Ad, Wd, bd, w_split=img, act=act), y))
        if Nout <= 256 and K > 256:
            ks = 8 if K >= 1024 else K // 256
            fails.append(_diff(f'linear bf16x3 ksplit{ks} {tag}', ops.linear(Ad, Wd, bd, w_split=img, act=act, ksplit=ks), y))
            fails.append(_diff(f'linear exact ksplit{ks} {tag}', ops.linear(Ad, Wd, bd, act=act, ksplit=ks), y))
    _finish(vkn, [f for f in fails if f])


def _train_shapes():
    """chain_train.linear: in features % 32 == 0; the transposed-weight form also needs out features % 32 == 0"""
    return [(M, K, Nout) for (M, K, Nout) in ec.gemm_shapes() if not (M > 512 and K == 2048 and Nout == 2048)]


@pytest.mark.parametrize('act', [0, 1], ids=['act0', 'relu'])
def test_chain_train_linear_forward_and_gradients(vkn, act):
    """chain_train.linear: forward, da, dW, db — computed in the layer's own backward"""
    ct = vkn.chain_train
    fails = []
    for i, (M, K, Nout) in enumerate(_train_shapes()):
        c = ec.linear_bwd_case(M, K, Nout, 1200 + i, act=act)
        A, W, b = (c[n].to(DEV).requires_grad_(True) for n in ('A', 'W', 'b'))
        y = ct.linear(A, W, b, act=act)
        y.backward(c['dy'].to(DEV))
        tag = f'M{M} K{K} N{Nout} act{act}'
        fails += [_diff(f'train linear y[m, n] {tag}', y, c['y']), _diff(f'train linear da[m, k] {tag}', A.grad, c['da']),
                  _diff(f'train linear dW[n, k] {tag}', W.grad, c['dW']), _diff(f'train linear db[n] {tag}', b.grad, c['db'])]
    _finish(vkn, [f for f in fails if f])


def test_chain_train_linear_transposed_weight(vkn):
    ct = vkn.chain_train
    fails = []
    for i, (M, K, Nout) in enumerate([t for t in _train_shapes() if t[2] % 32 == 0]):
        c = ec.linear_bwd_case(M, K, Nout, 1250 + i, wt=True)
        A, W = (c[n].to(DEV).requires_grad_(True) for n in ('A', 'W'))
        y = ct.linear(A, W, wt=True)
        y.backward(c['dy'].to(DEV))
        tag = f'wt M{M} K{K} N{Nout}'
        fails += [_diff(f'train linear y[m, n] {tag}', y, c['y'] - c['b'].double()), _diff(f'train linear da[m, k] {tag}', A.grad, c['da']),
                  _diff(f'train linear dW[k, n] {tag}', W.grad, c['dW'])]
    _finish(vkn, [f for f in fails if f])


def test_chain_train_linear_gradients_through_the_queue(vkn):
    """the same weight / bias gradients out of ONE vkn_linear_dw_batch_f32 launch per row count (DwQueue, flushed by ChainEntryFn)"""
    ct = vkn.chain_train
    fails = []
    by_m = {}
    for (M, K, Nout) in _train_shapes():
        by_m.setdefault(M, []).append((K, Nout))
    for M, shapes in sorted(by_m.items()):
        cases = [ec.linear_bwd_case(M, K, Nout, 1300 + 7 * j + M, act=j % 2) for j, (K, Nout) in enumerate(shapes)]
        Ws = [c['W'].to(DEV).requires_grad_(True) for c in cases]
        bs = [c['b'].to(DEV).requires_grad_(True) for c in cases]
        As = [c['A'].to(DEV).requires_grad_(True) for c in cases]
        queue = ct.DwQueue()
        imgs = ct.WeightImages(Ws, queue)
        ins = ct.ChainEntryFn.apply(queue, len(As), *As, *Ws, *bs)
        ys = [ct.linear(a, w, b, act=j % 2, images=imgs) for j, (a, w, b) in enumerate(zip(ins, Ws, bs))]
        torch.autograd.backward(ys, [c['dy'].to(DEV) for c in cases])
        for (K, Nout), c, a, w, b, y in zip(shapes, cases, As, Ws, bs, ys):
            tag = f'queued M{M} K{K} N{Nout}'
            fails += [_diff(f'{tag} y[m, n]', y, c['y']), _diff(f'{tag} da[m, k]', a.grad, c['da']), _diff(f'{tag} dW[n, k]', w.grad, c['dW']),
                      _diff(f'{tag} db[n]', b.grad, c['db'])]
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- FPN conv
def test_conv_gn_raw_output(vkn):
    """conv_gn modes raw and pos (integer pos), kernel 1 and 3, stride 1 and 2: the RAW conv output is exact (its GroupNorm statistics
    are not linear: tests/test_gpu_semantic_fpn.py judges them)"""
    ops = vkn.ops
    fails = []
    for i, (B, C, H, W, ks, stride, mode) in enumerate(ec.conv_shapes()):
        x, pos, w, out = ec.conv_case(B, C, H, W, ks, stride, mode, 1300 + i)
        xd, pd, wd = _cuda(x, pos, w)
        if ks == 1 and stride == 2:                     # a strided 1x1 conv is outside the envelope (no shipped config has one)
            assert _declines(vkn, lambda: ops.conv_gn(xd, ops.conv_prepare(wd), C, ks, stride, 32, pos=pd)), (B, C, H, W)
            continue
        got, st = ops.conv_gn(xd, ops.conv_prepare(wd), C, ks, stride, 32, pos=pd)
        fails.append(_diff(f'conv B{B} C{C} {H}x{W} k{ks} s{stride} {mode} [b, c, y, x]', got, out))
        assert bool(torch.isfinite(st).all())
    _finish(vkn, [f for f in fails if f])


# ------------------------------------------------------------------------------------------------------------------- paths reached
def test_the_sweep_reaches_both_kernel_variants(vkn):
    """once per op: the MFMA and the reference / generic kernels really ran (the decode's MFMA kernel of the release build is
    k_decode_mfma; k_decode4 exists in the debug build only), the fused pass is k_fused_il, the staged and the generic up-scaling"""
    ops = vkn.ops
    s = next(s for s in SWEEP if s.N == 117 and s.C == 256 and s.H * s.W == 128)
    x, z, _, _ = ec.gather_case(s)
    xd, zd = _cuda(x, z)
    _, names = _run_and_events(lambda: (ops.mask_gather(xd, zd), ops.mask_gather(xd, zd, flags=ops.FLAG_REF_KERNELS), ops.mask_gather_real(xd, zd)))
    assert _launches(names, 'k_gather_mfma') >= 2 and _launches(names, 'k_gather_ref') == 1 and _launches(names, 'k_gather_reduce') >= 2, sorted(set(names))
    x, k, kb, _ = ec.decode_case(s)
    xd, kd, kbd = _cuda(x, k, kb)
    odd = next(t for t in SWEEP if t.N == 117 and t.C == 256 and t.H * t.W == 135)
    xo, ko, kbo, _ = ec.decode_case(odd)
    xo, ko, kbo = _cuda(xo, ko, kbo)
    _, names = _run_and_events(lambda: (ops.mask_decode(xd, kd, kbd), ops.mask_decode(xd, kd, kbd, flags=ops.FLAG_REF_KERNELS)))
    assert _launches(names, 'k_decode_mfma') == 1 and _launches(names, 'k_decode_ref') == 1 and _launches(names, 'k_split_planes') == 1, sorted(set(names))
    _, names = _run_and_events(lambda: ops.mask_decode(xo, ko, kbo))                    # odd P: the reference kernel, silently
    assert _launches(names, 'k_decode_ref') == 1 and _launches(names, 'k_decode_mfma') == 0, sorted(set(names))
    hi, lo = ops.split_planes(kd)
    _, names = _run_and_events(lambda: ops.decode_gather(xd, hi, lo, s.N, kbd))
    assert _launches(names, 'k_fused_il') == 1, sorted(set(names))
    m = torch.zeros(1, 2, 3, 6, device=DEV)
    _, names = _run_and_events(lambda: (ops.upsample_bilinear(m, 2), ops.upsample_bilinear(m[..., :5].contiguous(), 2)))
    assert _launches(names, 'k_upsample_s') == 1 and _launches(names, 'k_upsample') == 1, sorted(set(names))
    g = torch.zeros(1, 2, 4, 128, device=DEV)
    _, names = _run_and_events(lambda: (ops.upsample_bilinear_bwd(g, 2), _abi_upsample_bwd(vkn, g, 2, 1), ops.upsample_bilinear_bwd(g, 4)))
    assert _launches(names, 'k_upsample_bwd2') == 1 and _launches(names, 'k_upsample_bwd') == 2, sorted(set(names))
    g = torch.zeros(1, 2, 4, 256, device=DEV)
    _, names = _run_and_events(lambda: ops.upsample_bilinear_bwd(g, 4))
    assert _launches(names, 'k_upsample_bwd4') == 1, sorted(set(names))
    vkn.ops.workspace_status()
