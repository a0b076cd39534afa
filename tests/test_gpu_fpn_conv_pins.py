"""GPU: the FPN conv engine (csrc/vkn_fpn.hip: k_fpn_conv, k_fpn_gn_finish; include/vkn.h: vkn_conv_gn_f32) element by element.

tests/test_gpu_semantic_fpn.py judges each tensor against its maximum on unit-scale Gaussian operands, test_gpu_exact.py pins the raw
and pos modes on integers at Cin == Cout.  Neither sees a lost LOW half of the activation split, a wrong border clamp of the bilinear
taps on a small row, a wave that owns one 32-row block, or one group's statistics.  Here:

1. Bit for bit (`torch.equal` with float64).  Modes `norm` and `up` on dyadic operands (exact_cases.fpn_case: integers, means k/4,
   rstd in {1/2, 1, 2}, gamma in {1/2, 1, 3/2}): every step of the load — (v - mean) rstd gamma + beta, ReLU, the x2 taps 1/4 and 3/4, the
   split hi + lo — and the accumulation are exact in fp32 in any order.  The `low` cases (means k/64 / k/1024, |x| <= 32) put bits into
   the low half of at least a fifth of the staged values and stay exact.  Modes raw / pos at Cin != Cout, dense and as single-pixel
   probes under the corners and under the first and last column of every 64-pixel run.  Premise, exact split, non-vacuity, ReLU clip
   share and low-half share are asserted on the CPU from the actual operands (tests/test_exact_premise.py proves the order-independence).
2. Conditioned float operands, the rule and the recorder of tests/test_gpu_conditioned.py (`_judge`, imported): per output element
   r = |hip - ref64| / T, bound_r = max(4 max r32, 2^-22), r32 from torch's fp32 F.conv2d on the same device applied to the fp32 load
   chain.  T = sum |w| |v| over the taps and input channels, v the STAGED conv input in float64 (x, x + pos, the normalised and
   ReLU'd value, its bilinear x2), in all four modes; where T == 0 the output must be exactly 0.  The f16 low half of a staged
   activation 0 < |v| < 2^-3, and of a weight 0 < |w scale| < 2^-3 after the stored power-of-two scale, is subnormal: exactly
   2^-24 sum(|w| [0 < |v| < 2^-3] + |v| [0 < |w scale| < 2^-3] / scale) is allowed beside bound_r T, the resolution include/vkn.h states
   at vkn_conv_gn_f32.  How many elements are over the purely relative rule is recorded (`over_rel`) next to max r, max r32, bound_r.
3. The output statistics per (frame, group) against float64 statistics of the kernel's OWN raw output: the mean relative to the
   group's mean |out|, rstd relative to itself, each within max(4 x the largest such error of torch's fp32 var_mean on that output
   on the device AMONG THE GROUPS OF THE SAME CLASS, 2^-22).  The classes follow the conditioning |mean| / std of the group, which is
   what the error of a variance grows with: constant groups (std == 0), benign groups (ratio < 8), high-mean groups (ratio >= 8) —
   so the groups built with a mean 2^6 times their deviation do not widen the bound of the others.
4. The gates of vkn_conv_gn_f32: VKN_E_SHAPE before any launch, nothing written.

Measured on an MI355X (profiles/fpn_conv_margins.json; 0 elements over the rule everywhere): conditioned max r 8.7e-7 .. 4.2e-6 against
bound_r 2.2e-5 .. 1.05e-4 at the stride-1 3x3 convs — there the bound is set by torch's own device conv, max r32 5.5e-6 .. 2.6e-5, so
those four cases pin less than the others —, 1.0e-6 .. 1.3e-6 against 2.7e-6 .. 3.7e-6 at stride 2; at the 1x1 conv 32 -> 512, 15 / 8 / 7
of 131072 outputs (raw / pos / norm) lie over the purely relative rule (max r 3.4e-5 / 3.2e-5 / 3.4e-6 against bound_r 1.6e-6 ..
1.8e-6), every one of them with an operand in 0 < |v| < 2^-3, and all inside the 2^-24 term: the engine has the resolution of the
real-operand gather.  Statistics: mean error <= 8.1e-8, rstd error <= 8.8e-7 (on per-channel groups with a mean 80 times their
deviation, where torch's var_mean has 8.6e-7); no group above 0.34 of the bound of its class.
What these tests see that test_gpu_semantic_fpn.py does not, tried with one-line breaks of csrc/vkn_fpn.hip (not committed): a
one-pixel run weighted as two pixels in k_fpn_gn_finish (the three cases with Wo = 65 / 129 here fail), and the low half of every
weight with |w| scale < 1 dropped in k_fpn_wsplit (all ten conditioned cases fail); both leave test_gpu_semantic_fpn.py green.
Dropping the activations' low half — everywhere, or only for one channel of a chunk at one patch column (of one image row) — shifting
one tap, and clamping the x2 taps a column early turn BOTH modules red."""
import ctypes
import math

import pytest
import torch
import torch.nn.functional as F

import exact_cases as ec
from abi_arena import SENT, Arena
from helpers import record_margins
from test_gpu_conditioned import _g, _judge, _scales, _tiny
from test_gpu_exact import _diff, _finish

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_SHAPE = -2
EPS = float(torch.tensor(1e-5, dtype=torch.float32))          # (double)1e-5f, as k_fpn_gn_finish adds it


def _cuda(*ts):
    return [t.to(DEV) if t is not None else None for t in ts]


# ------------------------------------------------------------------------------------------------------------ 1. bit for bit
@pytest.mark.parametrize('which', ['norm', 'up', 'low'])
def test_norm_up_on_load_bit_for_bit(vkn, which):
    ops = vkn.ops
    cases = ec.fpn_low_shapes() if which == 'low' else ec.fpn_norm_shapes(which)
    fails = []
    for c in cases:
        d = ec.fpn_case(c)                                     # (premise, exact split, clip share, low-half share: asserted in there)
        x, st, gam, bet, w = _cuda(d['x'], d['stats'], d['gamma'], d['beta'], d['w'])
        got, stats = ops.conv_gn(x, ops.conv_prepare(w), c.Cout, c.ks, c.stride, 32, in_stats=st, in_gamma=gam, in_beta=bet, upsample=c.mode == 'up')
        fails.append(_diff(f'{ec.fpn_id(c)} [b, co, y, x]', got, d['out']))
        assert bool(torch.isfinite(stats).all()), c
    _finish(vkn, [f for f in fails if f])


def test_raw_pos_unequal_channels_and_probes_bit_for_bit(vkn):
    """raw / pos at Cin != Cout (Cout 96 / 160 / 288: a wave with one 32-row block; 512: both grid slices; Cin = 512: sixteen chunks),
    dense integers and single-pixel probes (the output is the weight stencil)"""
    ops = vkn.ops
    fails = []
    for i, (B, Ci, Co, H, W, ks, stride, mode) in enumerate(ec.CONV_UNEQ):
        x, pos, w, out = ec.conv_case(B, Ci, H, W, ks, stride, mode, 3600 + i, Cout=Co)
        xd, pd, wd = _cuda(x, pos, w)
        got, _ = ops.conv_gn(xd, ops.conv_prepare(wd), Co, ks, stride, 32, pos=pd)
        fails.append(_diff(f'conv B{B} {Ci}->{Co} {H}x{W} k{ks} s{stride} {mode} [b, co, y, x]', got, out))
    for i, (B, Ci, Co, H, W, ks, stride) in enumerate(ec.FPN_PROBE):
        for mode in ('raw', 'pos'):
            x, pos, w, out, _ = ec.conv_probe_case(B, Ci, Co, H, W, ks, stride, mode, 3700 + i)
            xd, pd, wd = _cuda(x, pos, w)
            got, _ = ops.conv_gn(xd, ops.conv_prepare(wd), Co, ks, stride, 32, pos=pd)
            fails.append(_diff(f'probes B{B} {Ci}->{Co} {H}x{W} k{ks} s{stride} {mode} [b, co, y, x]', got, out))
    _finish(vkn, [f for f in fails if f])


def test_norm_on_load_is_the_apply_kernel_bit_for_bit(vkn):
    """One pre-activation (csrc/vkn_convtile.h: gn_preact) behind the conv's load and behind vkn_gn_relu_apply_f32: a conv that
    normalises a raw output r on load equals the same conv on the materialised relu(GN(r)), raw output and statistics, on float operands
    (a pre-activation near zero rounded two ways would clip in one and not in the other).  One full 64-pixel run plus one pixel."""
    ops = vkn.ops
    g = _g(2300)
    B, C, H, W, G = 1, 32, 3, 65, 8
    x = torch.randn(B, C, H, W, generator=g)
    w1, w2 = (0.05 * torch.randn(C, C, 3, 3, generator=g) for _ in range(2))
    gamma = (0.5 + torch.rand(C, generator=g)) * (torch.randint(0, 2, (C,), generator=g) * 2 - 1)
    beta = 0.3 * torch.randn(C, generator=g)
    x, w1, w2, gamma, beta = _cuda(x, w1, w2, gamma, beta)
    r, st = ops.conv_gn(x, ops.conv_prepare(w1), C, 3, 1, G)
    img2 = ops.conv_prepare(w2)
    y = ops.gn_relu_apply(r, st, gamma, beta)
    assert 0.25 < float((y == 0).float().mean()) < 0.75 and bool((y > 0).any())          # the ReLU clips a good share, not all
    on_load, on_load_st = ops.conv_gn(r, img2, C, 3, 1, G, in_stats=st, in_gamma=gamma, in_beta=beta)
    applied, applied_st = ops.conv_gn(y, img2, C, 3, 1, G)
    assert torch.equal(on_load, applied) and torch.equal(on_load_st, applied_st)
    torch.cuda.synchronize()
    ops.workspace_status()


# ------------------------------------------------------------------------------------------------------------ 2. conditioned
COND = [(mode, B, Ci, Co, H, W, ks, st) for (B, Ci, Co, H, W, ks, st) in ((2, 64, 96, 3, 65, 3, 1), (1, 256, 64, 5, 33, 3, 2), (1, 32, 512, 4, 64, 1, 1))
        for mode in ('raw', 'pos', 'norm')] + [('up', 2, 64, 96, 2, 33, 3, 1)]
CPG = 4                                                        # channels per input group of the norm / up cases


def _cond_operands(mode, B, Ci, Co, H, W, ks, g):
    """-> (x, pos | None, stats | None, gamma | None, beta | None, w), CPU fp32.  Per-input-channel scales over 2^-8 .. 2^8 (raw / pos: in
    x itself, about half exact zeros by a ReLU; norm / up: per-group scales in x with matching in_stats, per-channel scales in in_gamma,
    the kernel's own ReLU makes the zeros), per-output-row weight scales over the same span, channel 1 a copy of channel 0 under
    NEGATED weight columns (raw / pos: the negated channel under equal columns), 6.0e4 next to 1e-6."""
    w = torch.randn(Co, Ci, ks, ks, generator=g) * _scales(Co, g)[:, None, None, None]
    pos = stats = gamma = beta = None
    if mode in ('raw', 'pos'):
        s = _scales(Ci, g)[None, :, None, None]
        x = torch.relu(torch.randn(B, Ci, H, W, generator=g) * s + s * 0.2 * torch.randn(1, Ci, 1, 1, generator=g))
        x[:, 1] = -x[:, 0]
        w[:, 1] = w[:, 0]
        if mode == 'pos':
            pos = torch.randn(Ci, H, W, generator=g) * s[0] * 0.5 * (torch.rand(Ci, H, W, generator=g) < 0.25)
            pos[1] = -pos[0]
            pos[2:4] = 0.0                                     # (the 6.0e4 pixels stay inside the 65504 envelope)
        x[0, 2, 0, 0], x[0, 2, 0, 1 % W], x[0, 3, H - 1, W - 1], x[0, 3, H - 1, W - 2] = 6.0e4, 1e-6, -6.0e4, 1e-6
        x[B - 1, Ci - 1, H // 2, W // 2], x[B - 1, Ci - 1, H // 2, W // 2 - 1] = 6.0e4, -1e-6
    else:
        G = Ci // CPG
        sg = _scales(B * G, g).view(B, G)
        mean = sg * 0.5 * torch.randn(B, G, generator=g)
        sg[:, 0], mean[:, 0] = 1.0, 0.0                        # group 0 (channels 0 .. 3) carries the extreme values as they are
        x = torch.randn(B, Ci, H, W, generator=g) * sg.repeat_interleave(CPG, 1)[..., None, None] + mean.repeat_interleave(CPG, 1)[..., None, None]
        stats = torch.stack([mean, 1.0 / sg], -1).contiguous()
        gamma = _scales(Ci, g) * (torch.randint(0, 2, (Ci,), generator=g) * 2 - 1)
        beta = gamma.abs() * 0.2 * torch.randn(Ci, generator=g)
        x[:, 1], gamma[1], beta[1] = x[:, 0], gamma[0], beta[0]
        w[:, 1] = -w[:, 0]
        gamma[2:4], beta[2:4] = 1.0, 0.0
        x[0, 2, 0, 0], x[0, 2, 0, 1 % W], x[0, 3, H - 1, W - 1], x[0, 3, H - 1, W - 2] = 6.0e4, 1e-6, 6.0e4, 1e-6
    return x, pos, stats, gamma, beta, w


@pytest.mark.parametrize('mode,B,Ci,Co,H,W,ks,stride', COND, ids=[f'{c[0]}-{c[1]}-{c[2]}to{c[3]}-{c[4]}x{c[5]}-k{c[6]}s{c[7]}' for c in COND])
def test_conv_conditioned(vkn, mode, B, Ci, Co, H, W, ks, stride):
    ops = vkn.ops
    tid = f'test_gpu_fpn_conv_pins::conditioned[{mode}-{B}-{Ci}to{Co}-{H}x{W}-k{ks}s{stride}]'
    x, pos, stats, gamma, beta, w = _cuda(*_cond_operands(mode, B, Ci, Co, H, W, ks, _g(900 + Ci + Co + len(mode))))
    conv = lambda a, b: F.conv2d(a, b, stride=stride, padding=ks // 2)  # noqa: E731
    if mode in ('raw', 'pos'):
        xin64 = x.double() + (pos.double()[None] if pos is not None else 0.0)
        xin32 = x + pos[None] if pos is not None else x
    else:
        xin64 = ec.fpn_chain(x.double(), stats.double(), gamma.double(), beta.double(), mode == 'up')
        xin32 = ec.fpn_chain(x, stats, gamma, beta, mode == 'up')
    # the operands are what the docstring says
    taps64 = ec.fpn_chain(x.double(), stats.double(), gamma.double(), beta.double(), False) if mode == 'up' else xin64     # (x2 blends zeros away)
    assert 5.9e4 < float(xin64.abs().max()) < 65504 and 0.3 < float((taps64 == 0).double().mean()) < 0.7
    nz = xin64[xin64 != 0].abs()
    assert float(nz.max() / nz.min()) > 1e9 and float(w.abs().amax((1, 2, 3)).max() / w.abs().amax((1, 2, 3)).min()) > 2.0 ** 10
    wd = w.double()
    ref, T = conv(xin64, wd), conv(xin64.abs(), wd.abs())
    t32 = conv(xin32, w)
    scale = 2.0 ** (15 - math.frexp(float(w.abs().max()))[1])   # k_fpn_wscale: max |w| scale in [2^14, 2^15)
    sub = conv(_tiny(xin64), wd.abs()) + conv(xin64.abs(), _tiny(wd * scale)) / scale
    got, _ = ops.conv_gn(x, ops.conv_prepare(w), Co, ks, stride, 32, pos=pos, in_stats=stats, in_gamma=gamma, in_beta=beta, upsample=mode == 'up')
    err, e32 = (got.double() - ref).abs(), (t32.double() - ref).abs()
    Ts = torch.where(T == 0, torch.ones_like(T), T)             # (T == 0: ref == 0, and `_judge` asserts that the output is exactly 0)
    bound = max(4.0 * float((e32 / Ts).max()), 2.0 ** -22)
    over_rel = err > bound * T
    record_margins(tid + '::relative_only', dict(over_rel=int(over_rel.sum()), elements=over_rel.numel(), max_r=float((err / Ts).max()),
                                                 over_rel_without_tiny_operand=int((over_rel & (sub == 0)).sum()),
                                                 tiny_share_x=float(_tiny(xin64).mean()), tiny_share_w=float(_tiny(wd * scale).mean())))
    _judge(tid, 'conv', got, t32, ref, T, sub)
    torch.cuda.synchronize()
    ops.workspace_status()


# ------------------------------------------------------------------------------------------------------------ 3. statistics
STATS = [(2, 64, 96, 3, 65, 3, 1), (1, 32, 512, 4, 129, 1, 1), (2, 32, 32, 5, 1, 3, 1), (1, 64, 160, 1, 1, 3, 1), (1, 96, 64, 5, 130, 3, 2)]


def _stats_operands(B, Ci, Co, H, W, ks, g):
    """x unit Gaussian with channel 0 constant 1; w ~ N(0, 0.05^2).  Output rows 8 .. 15 (group 1 of Co / 8 groups): the centre tap of
    channel 0 adds 64 x the standard deviation of a row away from the border (a mean about 2^6 times the deviation).  The last eight
    rows: that tap is 0.75 and everything else zero — the output is the constant 0.75 (the centre tap is always inside the image)."""
    x = torch.randn(B, Ci, H, W, generator=g)
    x[:, 0] = 1.0
    w = torch.randn(Co, Ci, ks, ks, generator=g) * 0.05
    w[:, 0] = 0.0
    w[8:16, 0, ks // 2, ks // 2] = 64.0 * 0.05 * math.sqrt((Ci - 1) * ks * ks)
    w[Co - 8:] = 0.0
    w[Co - 8:, 0, ks // 2, ks // 2] = 0.75
    return x, w


@pytest.mark.parametrize('B,Ci,Co,H,W,ks,stride', STATS, ids=[f'{c[0]}-{c[1]}to{c[2]}-{c[3]}x{c[4]}-k{c[5]}s{c[6]}' for c in STATS])
def test_output_statistics_per_group(vkn, B, Ci, Co, H, W, ks, stride):
    ops = vkn.ops
    x, w = _cuda(*_stats_operands(B, Ci, Co, H, W, ks, _g(1700 + Co + W)))
    img = ops.conv_prepare(w)
    for G in (1, Co // 8, Co):
        tid = f'test_gpu_fpn_conv_pins::stats[{B}-{Ci}to{Co}-{H}x{W}-k{ks}s{stride}-G{G}]'
        out, st = ops.conv_gn(x, img, Co, ks, stride, G)
        v = out.double().view(B, G, -1)
        mean64, var64 = v.mean(-1), v.var(-1, unbiased=False)
        rstd64 = 1.0 / torch.sqrt(var64 + EPS)
        var32, mean32 = torch.var_mean(out.view(B, G, -1), dim=-1, unbiased=False)
        mag = v.abs().mean(-1)
        assert bool((mag > 0).all())
        e_mean, e_mean32 = (st[..., 0].double() - mean64).abs() / mag, (mean32.double() - mean64).abs() / mag
        e_rstd = (st[..., 1].double() - rstd64).abs() / rstd64
        e_rstd32 = (1.0 / torch.sqrt(var32.double() + EPS) - rstd64).abs() / rstd64
        cond = (mean64.abs() / var64.sqrt().clamp_min(1e-300))
        const = var64 == 0
        b_mean, b_rstd = torch.zeros_like(e_mean), torch.zeros_like(e_rstd)        # per group: the bound of its class (module docstring)
        for cls in (const, ~const & (cond < 8.0), ~const & (cond >= 8.0)):
            if bool(cls.any()):
                b_mean[cls] = max(4.0 * float(e_mean32[cls].max()), 2.0 ** -22)
                b_rstd[cls] = max(4.0 * float(e_rstd32[cls].max()), 2.0 ** -22)
        if G == Co // 8:                                       # the case is what it says: group 1 has its mean far above its deviation, the last is constant
            assert 32.0 < float(cond[:, 1].min()) < 1024.0 and bool(const[:, G - 1].all()) and bool((out.view(B, G, -1)[:, G - 1] == 0.75).all())
        if G == Co:
            assert int(const.sum()) >= B * 8
        record_margins(tid, dict(mean_err=float(e_mean.max()), mean_err32=float(e_mean32.max()), mean_bound_min=float(b_mean.min()),
                                 mean_bound_max=float(b_mean.max()), rstd_err=float(e_rstd.max()), rstd_err32=float(e_rstd32.max()),
                                 rstd_bound_min=float(b_rstd.min()), rstd_bound_max=float(b_rstd.max()),
                                 worst_mean_err_over_bound=float((e_mean / b_mean).max()), worst_rstd_err_over_bound=float((e_rstd / b_rstd).max()), over=int((e_mean > b_mean).sum() + (e_rstd > b_rstd).sum()),
                                 constant_groups=int(const.sum()), max_mean_over_std=float(cond[~const].max()) if bool((~const).any()) else 0.0))
        bad = ((e_mean > b_mean) | (e_rstd > b_rstd)).nonzero().tolist()
        assert not bad, (f'G = {G}: (frame, group) {bad[:6]} over the bound of their class: worst mean err / bound {float((e_mean / b_mean).max()):.3g}, '
                         f'worst rstd err / bound {float((e_rstd / b_rstd).max()):.3g}')
    torch.cuda.synchronize()
    ops.workspace_status()


# ------------------------------------------------------------------------------------------------------------ 4. gates
def test_gates_refuse_before_any_launch(vkn):
    """VKN_E_SHAPE, and not one word of the caller's memory written: in_stats together with pos, upsample without in_stats, k = 1 with
    stride 2, Cin or Cout = 544, Cin % in_groups != 0"""
    L = vkn._lib.lib()
    ops = vkn.ops
    p = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None  # noqa: E731
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    B, H, W = 1, 3, 5

    def refused(name, Ci, Co, ks, stride, pos=False, stats=False, up=False, in_groups=8):
        x = torch.ones(B, Ci, H, W, device=DEV)
        pd = torch.ones(Ci, H, W, device=DEV) if pos else None
        sd = torch.ones(B, max(in_groups, 1), 2, device=DEV) if stats else None
        gd = torch.ones(Ci, device=DEV) if stats else None
        nimg = L.vkn_conv_weight_bytes(Co, Ci, ks)
        assert nimg > 0
        img = torch.zeros(nimg, dtype=torch.uint8, device=DEV)
        Hin, Win = (2 * H, 2 * W) if up else (H, W)
        Ho, Wo = (Hin - 1) // stride + 1, (Win - 1) // stride + 1
        need = max(L.vkn_conv_gn_workspace_bytes(B, Co, H, W, stride, int(up)), 512)
        A = Arena(DEV)
        o, s_, w_ = A.out((B, Co, Ho, Wo), name='out'), A.out((B, 32, 2), name='stats'), A.ws(need, name='ws')
        rc = L.vkn_conv_gn_f32(p(x), p(pd), p(sd), p(gd), p(gd), in_groups if stats else 0, int(up), p(img), ks, stride, 32, o.ptr, s_.ptr,
                               B, Ci, H, W, Co, w_.ptr, need, stream)
        assert rc == E_SHAPE, (name, rc)
        torch.cuda.synchronize()
        A._materialise()
        assert bool((A.words == SENT).all()), f'{name}: a refused call wrote into the caller\'s memory'

    refused('in_stats with pos', 32, 32, 3, 1, pos=True, stats=True)
    refused('upsample without in_stats', 32, 32, 3, 1, up=True)
    refused('k = 1 with stride 2', 32, 64, 1, 2)
    refused('k = 1 with stride 2 on normalised input', 32, 64, 1, 2, stats=True)
    refused('Cin = 544', 544, 32, 3, 1)
    refused('Cout = 544', 32, 544, 1, 1)
    refused('Cin % in_groups != 0', 96, 32, 3, 1, stats=True, in_groups=64)
    refused('Cin % in_groups != 0 with upsample', 96, 32, 3, 1, stats=True, up=True, in_groups=5)
    # ... and the neighbours inside the envelope run (the gate is no blanket refusal)
    x = torch.ones(B, 512, H, W, device=DEV)
    out, _ = ops.conv_gn(x, ops.conv_prepare(torch.ones(512, 512, 1, 1, device=DEV)), 512, 1, 1, 32)
    assert bool((out == 512.0).all())
    ops.workspace_status()
