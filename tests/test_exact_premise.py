"""CPU: the premise of tests/test_gpu_exact.py and of the bit-for-bit part of tests/test_gpu_fpn_conv_pins.py, proved without a GPU.

For every case of the sweep the case builders of exact_cases.py assert the PREMISE (max sum |terms| < 2^24 from the actual operands;
fp16 outputs fit 11 bits) and NON-VACUITY (non-zero outputs, ON share in [0.05, 0.95], special rows as named).  Here, in addition,
torch's own CPU fp32 op on the same operands — whose summation order is none of the orders the HIP kernels use — must equal the
float64 reference bit for bit: with these operands fp32 accumulation is exact in any order."""
import pytest
import torch
import torch.nn.functional as F

import exact_cases as ec

SWEEP = ec.bncp_sweep()


def _same(got, want):
    return got.dtype == torch.float32 and torch.equal(got.double(), want.double().reshape(got.shape))


def test_sweep_covers_what_it_promises():
    c = ec.sweep_covers()
    assert c['N'] >= set(ec.N_EDGES) and c['C'] == set(ec.C_ALL) and c['P'] >= set(ec.P_EDGES) | set(ec.P_LARGE) and c['B'] == set(ec.B_ALL)
    for C in (64, 256):
        for N in ec.N_EDGES:
            for P in ec.P_EDGES:
                assert (C, N, P) in c['pairs'], (C, N, P)
    for P in (62, 66, 126, 130, 135):                                  # ragged P as 1 x P and as H x W with W odd
        assert (P, True) in c['forms'] and (P, False) in c['forms'], P
        assert all(hw[1] % 2 == 1 for hw in ec.HW_OF[P][1:])
    g = ec.gemm_shapes()
    assert {m for m, _, _ in g} == set(ec.GEMM_M) and {k for _, k, _ in g} == set(ec.GEMM_K) and {n for _, _, n in g} == set(ec.GEMM_NOUT)
    cs = ec.conv_shapes()
    assert {c_[1] for c_ in cs} == {32, 64, 256} and {c_[0] for c_ in cs} == {1, 2, 3} and {(c_[2], c_[3]) for c_ in cs} == set(ec.CONV_SIZES)
    assert {(c_[4], c_[5], c_[6]) for c_ in cs} == {(k, s, m) for k in (1, 3) for s in (1, 2) for m in ('raw', 'pos')}
    assert any((W * S) % 4 for (_, _, _, W, S) in ec.UP_FWD)


def test_special_rows_are_named():
    rows = ec.special_rows(117, 135)
    assert set(rows) == {'all_off', 'all_on', 'one_p0', 'one_plast', 'one_p63', 'one_p64', 'one_p127', 'one_p128'}
    assert len({r for r, _ in rows.values()}) == len(rows)
    assert set(ec.special_rows(31, 64)) == {'all_off', 'all_on', 'one_p0', 'one_plast', 'one_p63'}
    assert ec.special_rows(1, 64) == {}


def test_a_case_outside_the_premise_fails_as_a_test_bug():
    with pytest.raises(ec.PremiseError):
        ec.premise('too large', torch.tensor([2.0 ** 24]))
    with pytest.raises(ec.PremiseError):
        ec.non_vacuous('zero', torch.zeros(3))
    with pytest.raises(ec.PremiseError):
        ec.on_share('all on', torch.ones(8, dtype=torch.bool))
    with pytest.raises(ec.PremiseError):
        ec.premise_f16('12 bits', torch.tensor([2049.0]), 1.0)


@pytest.mark.parametrize('C', [64, 256, 0], ids=['C64', 'C256', 'otherC_and_large'])
def test_bncp_ops_fp32_equal_integer_reference(C):
    for s in [s for s in SWEEP if (s.C == C if C else s.C not in (64, 256) or s.large)]:
        x, z, xraw, cnt = ec.gather_case(s)
        bits = (z >= ec.THR).float().flatten(2)
        assert _same(torch.einsum('bnp,bcp->bnc', bits, x.flatten(2)), xraw), ('gather', s)
        assert _same(bits.sum(-1), cnt), ('cnt', s)
        for denom in ((1,) if s.large else (1, 16)):
            x, a, out, asum = ec.gather_real_case(s, denom)
            assert _same(torch.einsum('bnp,bcp->bnc', a.flatten(2), x.flatten(2)), out), ('gather_real', denom, s)
            assert _same(a.flatten(2).sum(-1), asum), ('asum', denom, s)
        x, k, kb, out = ec.decode_case(s)
        assert _same(torch.einsum('bnc,bcp->bnp', k, x.flatten(2)) + kb[..., None], out), ('decode', s)
        x, k, kb, zf, xraw, cnt = ec.fused_case(s)
        z32 = torch.einsum('bnc,bcp->bnp', k, x.flatten(2)) + kb[..., None]
        assert _same(z32, zf), ('fused logits', s)
        assert _same(torch.einsum('bnp,bcp->bnc', (z32 >= ec.THR).float(), x.flatten(2)), xraw), ('fused', s)
        if s.H * s.W % 64 == 0:                                   # the half-storage variants: integers up to 256 in fp16 and bf16
            x, z, xraw, cnt = ec.gather_case(s, x_span=256)
            assert torch.equal(x.half().float(), x) and torch.equal(x.bfloat16().float(), x), s


def test_upscaling_fp32_and_fp16_equal_float64_reference():
    for i, (B, N, H, W, S) in enumerate(ec.UP_FWD):
        m, out = ec.up_case(B, N, H, W, S, 700 + i, f16=True)
        got = F.interpolate(m, scale_factor=S, mode='bilinear', align_corners=False)
        assert _same(got, out), (B, N, H, W, S)
        assert torch.equal(got.half().double(), out)
    for i, (B, N, H, W, S) in enumerate(ec.UP_BWD):
        go, gin = ec.up_bwd_case(B, N, H, W, S, 800 + i)
        z = torch.zeros((B, N, H, W), requires_grad=True)
        F.interpolate(z, scale_factor=S, mode='bilinear', align_corners=False).backward(go)
        assert _same(z.grad, gin), (B, N, H, W, S)
    for i, (planes, H, W) in enumerate(ec.UP_PLANES[:2]):          # (the many-planes cases are tiny per plane: two of them here)
        for S in (2, 4):
            m, out = ec.up_case(1, planes, H, W, S, 900 + i, f16=True)
            assert _same(F.interpolate(m, scale_factor=S, mode='bilinear', align_corners=False), out)


def test_gemm_fp32_equals_integer_reference():
    for i, (M, K, Nout) in enumerate(ec.gemm_shapes()):
        A, W, b, y = ec.linear_case(M, K, Nout, 1100 + i, act=i % 2)
        got = F.linear(A, W, b)
        assert _same(got.clamp_min(0) if i % 2 else got, y), (M, K, Nout)
    for i, (M, K, Nout) in enumerate([(117, 256, 256), (33, 64, 19), (513, 512, 124), (234, 2048, 256)]):
        for act in (0, 1):
            c = ec.linear_bwd_case(M, K, Nout, 1200 + i, act=act)
            A, W = c['A'].clone().requires_grad_(True), c['W'].clone().requires_grad_(True)
            b = c['b'].clone().requires_grad_(True)
            y = F.linear(A, W, b)
            y = y.relu() if act else y
            y.backward(c['dy'])
            assert _same(y.detach(), c['y']) and _same(A.grad, c['da']) and _same(W.grad, c['dW']) and _same(b.grad, c['db']), (M, K, Nout, act)


def test_dw_fp32_equals_integer_reference():
    """the cases of tests/test_gpu_chain_blocks.py's weight-gradient tests: plain, accumulating on integer old values, the batch items"""
    cases = [(M, K, Nout, 1500 + i) for i, (M, K, Nout) in enumerate(ec.DW_SHAPES)]
    cases += [(ec.DW_BATCH_M, K, Nout, 1600 + i) for i, (K, Nout) in enumerate(ec.dw_batch_shapes(max(ec.DW_BATCH_ITEMS)))]
    for M, K, Nout, seed in cases:
        dy, A, old_w, old_b, dW, db = ec.dw_case(M, K, Nout, seed)
        assert _same(dy.t() @ A, dW) and _same(dy.sum(0), db), (M, K, Nout)
        assert _same(old_w + dy.t() @ A, old_w.double() + dW) and _same(old_b + dy.sum(0), old_b.double() + db), (M, K, Nout)
        w, b = torch.zeros(Nout, K, requires_grad=True), torch.zeros(Nout, requires_grad=True)
        (F.linear(A, w, b) * dy).sum().backward()
        assert _same(w.grad, dW) and _same(b.grad, db), (M, K, Nout)


def test_conv_fp32_equals_integer_reference():
    for i, (B, C, H, W, ks, stride, mode) in enumerate(ec.conv_shapes()):
        if H * W > 1000 and i % 4:                                 # the frame-sized maps: a quarter of them (they dominate the time)
            continue
        x, pos, w, out = ec.conv_case(B, C, H, W, ks, stride, mode, 1300 + i)
        got = F.conv2d(x + pos if pos is not None else x, w, stride=stride, padding=ks // 2)
        assert _same(got, out), (B, C, H, W, ks, stride, mode)


def test_autograd_and_init_cases_hold():
    for s in ec.GRAD_SHAPES:
        x, k, kb, dz, dx, dk, dkb = ec.decode_grad_case(s)
        xx, kk, bb = x.clone().requires_grad_(True), k.clone().requires_grad_(True), kb.clone().requires_grad_(True)
        (torch.einsum('bnc,bcp->bnp', kk, xx.flatten(2)) + bb[..., None]).backward(dz.flatten(2))
        assert _same(xx.grad, dx) and _same(kk.grad, dk) and _same(bb.grad, dkb), s
        x, z, d, dx = ec.gather_grad_case(s)
        xx = x.clone().requires_grad_(True)
        torch.einsum('bnp,bcp->bnc', (z >= ec.THR).float().flatten(2), xx.flatten(2)).backward(d)
        assert _same(xx.grad, dx), s
    for i, sh in enumerate(ec.INIT_SHAPES):
        for cat in (False, True):
            loc, sem, iw, sw, sb, ref = ec.init_case(*sh, 1400 + i, cat)
            mp = F.conv2d(loc, iw[:, :, None, None])
            assert _same(mp, ref['mask_preds'][:, :iw.shape[0]]), sh
            assert _same(F.conv2d(sem, sw[:, :, None, None], sb), ref['seg_preds']), sh
            obj = torch.einsum('bnhw,bchw->bnc', (mp.sigmoid() > 0.5).float(), sem + loc)
            assert _same(iw[None] + obj, ref['prop'][:, :iw.shape[0]]), sh


# ---- the FPN conv per element (tests/test_gpu_fpn_conv_pins.py): on-load transforms, low halves, Cin != Cout, probes
def test_fpn_shapes_cover_what_they_promise():
    for mode in ('norm', 'up'):
        c = ec.fpn_covers(ec.fpn_norm_shapes(mode))
        assert c['Wo'] >= set(ec.FPN_WO) and c['H'] >= set(ec.FPN_H) and c['B'] == {1, 2, 3} and c['CC'] >= set(ec.FPN_CC), mode
        assert c['KS'] == set(ec.FPN_KS) and c['groups'] == {1, 8, 'Cin'}, mode
        for (ks, st) in (ec.FPN_KS if mode == 'norm' else ((3, 2),)):       # no axis is locked to a kernel variant ('up': the variant with all nine widths)
            assert {(ci, co) for (k, s_, ci, co) in c['KS_CC'] if (k, s_) == (ks, st)} >= set(ec.FPN_CC), (mode, ks, st)
            assert {g for (k, s_, g) in c['KS_groups'] if (k, s_) == (ks, st)} == {1, 8, 'Cin'}, (mode, ks, st)
            assert {b for (k, s_, b) in c['KS_B'] if (k, s_) == (ks, st)} == {1, 2, 3}, (mode, ks, st)
        for Wo in ec.FPN_WO:                                # every (ksize, stride) at every width the mode can produce
            for (ks, st) in ec.FPN_KS:
                possible = mode == 'norm' or st == 2 or Wo % 2 == 0          # 'up' at stride 1: Wo = 2 W
                assert ((Wo, ks, st) in c['WoKS']) == possible, (mode, Wo, ks, st)
        if mode == 'up':
            assert c['one_row'] and c['one_col']            # Hs = 1, Ws = 1: both clamps of the bilinear taps are zero
        else:
            assert c['s2_parity'] == {(0, 0), (0, 1), (1, 0), (1, 1)}        # stride 2 on odd and even Hin / Win
    low = ec.fpn_low_shapes()
    assert {c.mode for c in low} == {'norm', 'up'} and all(c.Cin == 32 for c in low if c.mode == 'norm')
    assert {c.Cout for c in low} >= {32, 96, 160, 288, 512} and {(c.ks, c.stride) for c in low} == set(ec.FPN_KS)
    assert {co for (_, _, co, *_) in ec.CONV_UNEQ} >= {96, 160, 512} and all(ci != co or ci == 512 for (_, ci, co, *_) in ec.CONV_UNEQ)
    assert {co for (_, _, co, *_) in ec.FPN_PROBE} >= {96, 160, 512} and all(ci != co for (_, ci, co, *_) in ec.FPN_PROBE)


def test_a_fpn_case_outside_its_premise_fails_as_a_test_bug():
    with pytest.raises(ec.PremiseError):                    # the low-half recipe at Cin = 512: sums of about 2^26 units of 2^-10
        ec.fpn_case(ec.FpnCase(1, 512, 32, 3, 5, 3, 1, 'up', 512, True, 3599))
    hi, lo = ec.split_f16(torch.tensor([1.0 + 2.0 ** -12, 3.0]))
    assert lo.tolist() == [2.0 ** -12, 0.0] and hi.tolist() == [1.0, 3.0]


@pytest.mark.parametrize('which', ['norm', 'up', 'low'])
def test_fpn_load_chain_fp32_equals_float64_reference(which):
    """torch's CPU fp32 chain (normalise, ReLU, bilinear x2) and its fp32 conv2d equal the float64 reference bit for bit on every case;
    `fpn_case` itself asserts premise, exact split, non-vacuity, clip share and (low) the low-half share"""
    cases = ec.fpn_low_shapes() if which == 'low' else ec.fpn_norm_shapes(which)
    lows = []
    for c in cases:
        d = ec.fpn_case(c)
        x32 = ec.fpn_chain(d['x'], d['stats'], d['gamma'], d['beta'], c.mode == 'up')
        assert _same(x32, d['xin']), ('chain', c)
        assert _same(F.conv2d(x32, d['w'], stride=c.stride, padding=c.ks // 2), d['out']), ('conv', c)
        assert d['out'].shape[2:] == ec.fpn_out_hw(c)[2:], c
        lows.append(d['low_share'])
    if which == 'low':
        assert min(lows) >= ec.FPN_LOW_SHARE
    else:
        assert max(lows) == 0.0                             # (the plain dyadic cases leave every low half zero: that is why `low` exists)


def test_conv_unequal_channels_and_probes_fp32_equal_integer_reference():
    for i, (B, Ci, Co, H, W, ks, stride, mode) in enumerate(ec.CONV_UNEQ):
        x, pos, w, out = ec.conv_case(B, Ci, H, W, ks, stride, mode, 3600 + i, Cout=Co)
        assert _same(F.conv2d(x + pos if pos is not None else x, w, stride=stride, padding=ks // 2), out), (B, Ci, Co, H, W, ks, stride, mode)
    for i, (B, Ci, Co, H, W, ks, stride) in enumerate(ec.FPN_PROBE):
        for mode in ('raw', 'pos'):
            x, pos, w, out, n = ec.conv_probe_case(B, Ci, Co, H, W, ks, stride, mode, 3700 + i)
            assert _same(F.conv2d(x + pos if pos is not None else x, w, stride=stride, padding=ks // 2), out), (B, Ci, Co, H, W, ks, stride, mode)
            assert n >= 1 and int((x != 0).sum()) + (int((pos != 0).sum()) if pos is not None else 0) == n      # one pixel per probe
    assert (0, 63) in ec.probe_pixels(3, 65, 1) and (0, 64) in ec.probe_pixels(3, 65, 1) and (2, 0) in ec.probe_pixels(3, 65, 1)
    assert (4, 126) in ec.probe_pixels(5, 129, 2) and (4, 128) in ec.probe_pixels(5, 129, 2)                   # output columns 63 and 64


# ---- the FPN backward's two MFMA gradients bit for bit (tests/test_gpu_fpn_bwd_pins.py)
def _wgrad_nsplit(vkn, shape):
    """the split count of a shape as the LIBRARY carves it (a host function: no device), checked against the header's constants"""
    B, Ci, Co, H, W, k, s = shape
    nb = vkn._lib.lib().vkn_conv_wgrad_workspace_bytes(B, Ci, H, W, Co, k, s)
    nsplit = ec.wgrad_nsplit_of(nb, shape)
    K = vkn._lib.FPN_TRAIN
    nruns, _ = ec.wgrad_runs(shape)
    tiles = (Ci // 32) * ((Co + 127) // 128)
    assert nsplit == min(max(1, K['VKN_FPN_WGRAD_TARGET_WGS'] // tiles), K['VKN_FPN_WGRAD_MAX_SPLITS'], nruns), (shape, nsplit)
    return nsplit


def test_fpn_bwd_pins_walk_several_runs_per_split(vkn):
    """The reason these cases exist: a split of the weight gradient that sums MORE THAN ONE pixel run.  From the split count read back
    from the library: the structure each case names, some split with >= 3 runs, some split across a frame boundary, runs not divisible
    by the splits, the VKN_FPN_WGRAD_MAX_SPLITS clamp at work, a stride-2 case behind the 64-pixel seam, more than 5 image rows."""
    most, crossing, uneven, clamped = 0, 0, 0, 0
    for shape, (want_runs, want_splits, want_sizes) in ec.FPN_BWD_PINS.items():
        nruns, per_frame = ec.wgrad_runs(shape)
        nsplit = _wgrad_nsplit(vkn, shape)
        spans = ec.wgrad_split_runs(nruns, nsplit)
        sizes = {}
        for a, b in spans:
            sizes[b - a] = sizes.get(b - a, 0) + 1
        assert (nruns, nsplit, sizes) == (want_runs, want_splits, want_sizes), \
            f'{shape}: {nruns} runs in {nsplit} splits of {sizes} runs — the split rule changed: this case no longer pins what exact_cases.FPN_BWD_PINS says'
        assert spans[0][0] == 0 and spans[-1][1] == nruns and all(p[1] == q[0] for p, q in zip(spans, spans[1:]))
        most = max(most, max(sizes))
        crossing += sum(1 for a, b in spans if b > a and a // per_frame != (b - 1) // per_frame)
        uneven += nruns % nsplit != 0
        clamped += nsplit == vkn._lib.FPN_TRAIN['VKN_FPN_WGRAD_MAX_SPLITS'] < nruns
    assert most >= 3, f'every split of every case owns at most {most} runs: the run loop of k_conv_wgrad is pinned nowhere'
    assert crossing >= 2 and uneven >= 1 and clamped >= 1, (crossing, uneven, clamped)
    s2 = [sh for sh in ec.FPN_BWD_PINS if sh[6] == 2]
    assert any((sh[4] - 1) // 2 + 1 > 64 and ((sh[4] - 1) // 2 + 1) % 64 for sh in s2)          # a ragged run behind the seam, odd W: both parities differ
    assert max(sh[3] for sh in ec.FPN_BWD_PINS) > 5 and {(sh[5], sh[6]) for sh in ec.FPN_BWD_PINS} == set(ec.FPN_KS)
    # ... and the cases of tests/fpn_bwd_ref.py before these: one run per split, all of them (what the pins add)
    import fpn_bwd_ref as R
    old = [c[:7] for n, c in R.BLOCK_CASES.items() if n not in ('k3s1-32to32-33x65-g8-B1', 'k3s2-32to32-9x131-g8')]
    assert all(ec.wgrad_runs(sh)[0] <= _wgrad_nsplit(vkn, sh) for sh in old)
    assert [c[:7] for c in R.CONV_CASES.values()] == list(ec.FPN_BWD_PINS)[:2]


@pytest.mark.parametrize('i', range(len(ec.FPN_BWD_PINS)), ids=[ec.fpn_bwd_id(s) for s in ec.FPN_BWD_PINS])
def test_fpn_bwd_pins_fp32_equal_float64_reference(i):
    """`conv_bwd_case` asserts premise, non-vacuity and empty low halves; torch's CPU fp32 autograd — another summation order than the
    kernels' — equals the float64 reference bit for bit"""
    shape = list(ec.FPN_BWD_PINS)[i]
    d = ec.conv_bwd_case(shape, 3800 + i)
    dw, dx = ec.conv_grads(d['x'], d['w'], d['dr'], shape[6])
    assert _same(dw, d['dw']) and _same(dx, d['dx']), shape
    assert all(float(d[k].abs().max()) <= 3.0 and torch.equal(d[k], d[k].round()) for k in ('x', 'w', 'dr'))


@pytest.mark.parametrize('variant', ec.FPN_BWD_LOW_VARIANTS)
def test_fpn_bwd_low_halves_stay_exact(variant):
    """`conv_bwd_low_case` asserts the exact split of the staged wide operand, its low-half share, the partner's empty low halves and
    the premise on the halves; here the staged scale is the kernel's (max |v| 2^(15 - e) in [2^14, 2^15)), the wide operand really is
    wider than an f16 significand, and fp32 autograd equals float64"""
    kernel, which = variant.split('-')
    for j, shape in enumerate(ec.FPN_BWD_LOW):
        d = ec.conv_bwd_low_case(shape, variant, 3900 + 4 * j + ec.FPN_BWD_LOW_VARIANTS.index(variant))
        wide = d[which]
        assert 2.0 ** 14 <= float(wide.abs().max()) * ec.staged_pow2(wide) < 2.0 ** 15 and 4095 < float(wide.abs().max()) <= ec.FPN_BWD_WIDE
        assert d['low_share'] >= ec.FPN_LOW_SHARE
        narrow = [k for k in ('x', 'w', 'dr') if k != which]
        assert all(set(d[k].unique().tolist()) == {-1.0, 0.0, 1.0} for k in narrow)
        dw, dx = ec.conv_grads(d['x'], d['w'], d['dr'], shape[6])
        assert _same(dw if kernel == 'wgrad' else dx, d['out']), (shape, variant)


def test_a_fpn_bwd_case_outside_its_premise_fails_as_a_test_bug():
    with pytest.raises(ec.PremiseError, match='fp32 accumulation is not exact'):       # |v| <= 200 at 512 channels: dx sums of about 2^25
        ec.conv_bwd_case((3, 512, 512, 3, 65, 3, 1), 3800, span=200)
    with pytest.raises(ec.PremiseError, match='non-empty low half'):                   # 13-bit integers as a "plain" operand
        ec.conv_bwd_case((1, 32, 32, 1, 1, 1, 1), 3800, span=8191)
    with pytest.raises(ec.PremiseError, match='fp32 accumulation is not exact'):       # the low-half recipe at 512 channels, 15-bit integers
        ec.conv_bwd_low_case((3, 512, 512, 3, 65, 3, 1), 'dgrad-dr', 3900, wide=32767)
    with pytest.raises(ec.PremiseError, match='low half'):                             # 11 bits: nothing reaches the low half
        ec.conv_bwd_low_case(ec.FPN_BWD_LOW[0], 'wgrad-x', 3900, wide=2047)
    assert ec.staged_pow2(torch.tensor([3.0, -1.0])) == 2.0 ** 13 and ec.staged_pow2(torch.tensor([8191.0])) == 4.0 and ec.staged_pow2(torch.zeros(2)) == 1.0
