"""GPU: float operands whose magnitudes vary INSIDE one tensor, judged element by element.

Integer operands (test_gpu_exact.py) cannot see a lost LOW half of the f16 hi+lo split: their low halves are zero.  Unit-scale Gaussian
operands judged against the tensor's max-abs cannot see it either on a small row inside a large tensor.  Here, for the gather, the
real-operand gather, the decode, the fused pass and ops.linear:
  * x = ReLU(normal * s_c + t_c) with per-channel scales s_c log-uniform over 2^-8 .. 2^8 (about half exact zeros, five decades);
  * kernels / weight rows with per-row scales over the same span;
  * a few elements at +-6.0e4 (inside the 65504 envelope) next to elements of 1e-6 — the status word must stay clear;
  * cancelling pairs (+a, -a inside one mask; a channel and its negation under equal kernel columns): outputs near zero, terms not;
  * mask logits with |z| >= 1, so the bits are not in question (fused pass: its logits are computed, so the case picks each row's
    bias, from the float64 reference alone, such that no logit lies within the decode's allowed error of the threshold).

Rule, per output element:  r = |hip - ref64| / T,  T = sum |terms| in float64; where T == 0 the output must be exactly 0.  The same
ratio r32 is measured for torch's own fp32 op on the same device and operands, and
        bound_r = max(4 * max r32, 2^-22)
(4 = the split's documented 2^-22 over fp32's 2^-24; the factor of test_gpu_semantic_fpn.py::_rule).  Where the f16 low
half goes subnormal (0 < |v| < 2^-3) the documented resolution is absolute, 2^-24 per operand (include/vkn.h at
vkn_mask_gather_real_f32), and exactly that is allowed:
        |hip - ref64| <= bound_r * T + 2^-24 * sum_c (|a_c| [0 < |x_c| < 2^-3] + |x_c| [0 < |a_c| < 2^-3])
(an exactly zero operand contributes an exactly zero product: it earns no allowance; ops.linear runs on fp32 / bf16x3 operands with
the full exponent range and gets none at all).  max r, max r32 and the bound of every case go to the parity-margins file.

Measured on an MI355X (all cases, 0 elements over the rule): gather max r 2.7e-7 .. 4.8e-7 against bound_r 8.8e-7 .. 2.4e-6; fused pass
3.0e-7 .. 5.6e-7 against 1.9e-6 .. 3.2e-6; ops.linear 2.2e-7 .. 2.3e-6 against 3.0e-6 .. 6.4e-6.  The decode and the real-operand gather
are the two ops that split a REAL operand below 2^-3 (rows scaled down to 2^-8): there max r alone is 4.7e-7 .. 1.1e-4 against bound_r
1.9e-6 .. 6.2e-6, i.e. some small-magnitude outputs exceed the relative part and pass only through the documented 2^-24 absolute term —
the resolution the header states, measured here rather than assumed."""
import pytest
import torch

from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SHAPES = [(2, 117, 256, 8, 16), (1, 100, 64, 9, 15), (1, 129, 128, 16, 64), (1, 33, 256, 48, 156)]      # (B, N, C, H, W)
TINY = 2.0 ** -3
U = 2.0 ** -24


def _g(seed):
    return torch.Generator(device='cpu').manual_seed(seed)


def _scales(n, g):
    return torch.exp2(torch.rand(n, generator=g) * 16 - 8)


def _x(B, C, P, g):
    s = _scales(C, g)[None, :, None]
    t = s * 0.2 * torch.randn(1, C, 1, generator=g)
    x = torch.relu(torch.randn(B, C, P, generator=g) * s + t)
    x[:, 1] = -x[:, 0]                                     # a channel and its negation (the decode cancels them under equal kernel columns)
    if P > 12:
        x[:, :, 10] = s[0, :, 0] * 100.0                   # (at most 25600: inside the 65504 envelope)
        x[:, :, 11] = -x[:, :, 10]                         # +a, -a in two pixels that every mask row switches ON
    x[0, 2, 0], x[0, 2, 1], x[0, 3, P - 1], x[0, 3, P - 2] = 6.0e4, 1e-6, -6.0e4, 1e-6
    x[B - 1, C - 1, P // 2], x[B - 1, C - 1, P // 2 - 1] = 6.0e4, -1e-6
    return x


def _kernels(B, N, C, g):
    k = torch.randn(B, N, C, generator=g) * _scales(N, g)[None, :, None]
    k[:, :, 1] = k[:, :, 0]
    return k


def _logits(B, N, P, g):
    z = torch.randn(B, N, P, generator=g)
    z = torch.sign(z) * (1.0 + 3.0 * z.abs())
    z[z == 0] = 1.0
    if P > 12:
        z[:, :, 10:12] = 2.0
    return z


def _judge(test_id, name, hip, t32, ref64, T, sub=None):
    """the rule of the module docstring; records the measured figures, then asserts"""
    err, e32 = (hip.double() - ref64).abs(), (t32.double() - ref64).abs()
    zero = T == 0
    assert bool((hip[zero] == 0).all()), f'{name}: an output whose every term is zero is not exactly zero'
    Ts = torch.where(zero, torch.ones_like(T), T)
    r, r32 = torch.where(zero, torch.zeros_like(T), err / Ts), torch.where(zero, torch.zeros_like(T), e32 / Ts)
    bound = max(4.0 * float(r32.max()), 2.0 ** -22)
    allow = bound * T + (U * sub if sub is not None else 0.0)
    over = err > allow
    record_margins(f'{test_id}::{name}', dict(max_r=float(r.max()), max_r32=float(r32.max()), bound=bound, over=int(over.sum()),
                                              min_T_over_max_T=float(T[~zero].min() / T.max()) if bool((~zero).any()) else 0.0))
    if bool(over.any()):
        idx = over.nonzero()[:6].tolist()
        i0 = tuple(idx[0])
        raise AssertionError(f'{name}: {int(over.sum())} of {over.numel()} elements over the bound (max r {float(r.max()):.3g}, max r32 '
                             f'{float(r32.max()):.3g}, bound_r {bound:.3g}); first {idx}: hip {hip[i0].item()!r} ref {ref64[i0].item()!r} '
                             f'T {T[i0].item():.6g}')


def _tiny(t):
    return ((t != 0) & (t.abs() < TINY)).double()


def _sub(eq, a, x):
    """sum (|a| [0 < |x| < 2^-3] + |x| [0 < |a| < 2^-3]) over the contraction of `eq`, float64"""
    ad, xd = a.double().abs(), x.double().abs()
    return torch.einsum(eq, ad, _tiny(x)) + torch.einsum(eq, _tiny(a), xd)


@pytest.mark.parametrize('B,N,C,H,W', SHAPES)
def test_gather_decode_fused_conditioned(vkn, B, N, C, H, W):
    ops = vkn.ops
    P = H * W
    tid = f'test_gpu_conditioned::gdf[{B}-{N}-{C}-{H}x{W}]'
    g = _g(7 + N + C)
    x, k, z = _x(B, C, P, g).to(DEV), _kernels(B, N, C, g).to(DEV), _logits(B, N, P, g).to(DEV)
    a = (torch.randn(B, N, P, generator=g) * _scales(N, g)[None, :, None]).to(DEV)
    kb = (torch.randn(B, N, generator=g) * 0.5).to(DEV)
    assert float(x.abs().max()) == 6.0e4 and float((x == 0).double().mean()) > 0.3
    x4, z4, a4 = x.view(B, C, H, W), z.view(B, N, H, W), a.view(B, N, H, W)
    xd, kd = x.double(), k.double()
    # binarised gather
    bits = z >= ops.thr_logit(0.5)
    assert bool(((z.abs() >= 1.0)).all()) and 0.05 <= float(bits.double().mean()) <= 0.95
    bf = bits.float()
    xraw, cnt = ops.mask_gather(x4, z4)
    assert torch.equal(cnt, bf.sum(-1))
    _judge(tid, 'gather', xraw, torch.einsum('bnp,bcp->bnc', bf, x), torch.einsum('bnp,bcp->bnc', bf.double(), xd),
           torch.einsum('bnp,bcp->bnc', bf.double(), xd.abs()), _sub('bnp,bcp->bnc', bf, x))
    # real-operand gather
    out, asum = ops.mask_gather_real(x4, a4)
    _judge(tid, 'gather_real', out, torch.einsum('bnp,bcp->bnc', a, x), torch.einsum('bnp,bcp->bnc', a.double(), xd),
           torch.einsum('bnp,bcp->bnc', a.double().abs(), xd.abs()), _sub('bnp,bcp->bnc', a, x))
    ones = torch.ones(B, 1, P, device=DEV)
    _judge(tid, 'gather_real_asum', asum, a.sum(-1), a.double().sum(-1), a.double().abs().sum(-1), _sub('bnp,bcp->bnc', a, ones)[..., 0])
    # decode
    ref = torch.einsum('bnc,bcp->bnp', kd, xd) + kb.double()[..., None]
    T = torch.einsum('bnc,bcp->bnp', kd.abs(), xd.abs()) + kb.double().abs()[..., None]
    t32 = torch.einsum('bnc,bcp->bnp', k, x) + kb[..., None]
    zz = ops.mask_decode(x4, k, kb)
    _judge(tid, 'decode', zz.view(B, N, P), t32, ref, T, _sub('bnc,bcp->bnp', k, x))
    if P % 2 == 0:
        hi, lo = ops.split_planes(k)
        assert int(lo.count_nonzero()) > 0.8 * B * N * C                  # the low halves are alive here (they are all zero in test_gpu_exact.py)
        assert torch.equal(ops.mask_decode_planes(x4, hi, lo, N, kb), zz)
    # fused decode -> gather (where supported).  Its logits are computed, so |z| >= 1 cannot be imposed pixel by pixel; the BIAS is a
    # free operand instead: per row, the first of 32 candidates kb (1 + j / 16) under which every float64 logit of the row lies farther
    # from the threshold than TWICE the error the decode is allowed on these operands (bound_r T + 2^-24 sub, the rule above with the
    # decode's own bound_r).  Chosen from the float64 reference alone; then no bit is in question and there is no flip budget.
    if vkn._lib.lib().vkn_decode_gather_supported(C, P):
        thr = ops.thr_logit(0.5)
        nob, Tnob = ref - kb.double()[..., None], T - kb.double().abs()[..., None]
        br = max(4.0 * float(((t32.double() - ref).abs() / T).max()), 2.0 ** -22)
        sub = _sub('bnc,bcp->bnp', k, x)
        kbf = torch.full_like(kb, float('nan'), dtype=torch.float64)
        for j in range(32):
            cand = kb.double() * (1.0 + j / 16.0)
            clear = ((nob + cand[..., None] - thr).abs() > 2.0 * (br * (Tnob + cand.abs()[..., None]) + U * sub)).all(-1)
            kbf = torch.where(kbf.isnan() & clear, cand, kbf)
        assert not bool(kbf.isnan().any()), f'case bug: {int(kbf.isnan().sum())} rows have no bias candidate that clears the threshold'
        kb = kbf.float()                                   # (rounded to fp32: the margin is re-checked on the rounded bias)
        ref = nob + kb.double()[..., None]
        T = Tnob + kb.double().abs()[..., None]
        assert bool(((ref - thr).abs() > br * T + U * sub).all()), 'case bug: a logit inside the decode allowance of the threshold'
        b64 = (ref >= thr)
        assert 0.05 <= float(b64.double().mean()) <= 0.95
        hi, lo = ops.split_planes(k)
        fx, fc = ops.decode_gather(x4, hi, lo, N, kb)
        assert torch.equal(fc, b64.float().sum(-1)), 'fused pass: ON counts differ from the float64 logits'
        _judge(tid, 'fused', fx, torch.einsum('bnp,bcp->bnc', b64.float(), x), torch.einsum('bnp,bcp->bnc', b64.double(), xd),
               torch.einsum('bnp,bcp->bnc', b64.double(), xd.abs()), _sub('bnp,bcp->bnc', b64.float(), x))
    torch.cuda.synchronize()
    ops.workspace_status()


@pytest.mark.parametrize('M,K,Nout', [(117, 256, 256), (33, 2048, 124), (513, 512, 257), (234, 768, 19)])
def test_linear_conditioned(vkn, M, K, Nout):
    """ops.linear, exact-fp32 MFMA and the bf16x3 split: rows of A and of W over 2^-8 .. 2^8, +-6e4 next to 1e-6, cancelling columns"""
    ops = vkn.ops
    tid = f'test_gpu_conditioned::linear[{M}-{K}-{Nout}]'
    g = _g(100 + M)
    A = torch.relu(torch.randn(M, K, generator=g) * _scales(K, g)[None, :])
    W = torch.randn(Nout, K, generator=g) * _scales(Nout, g)[:, None]
    A[:, 1], W[:, 1] = -A[:, 0], W[:, 0]
    A[0, 2], A[0, 3], A[M - 1, K - 1], A[M - 1, K - 2] = 6.0e4, 1e-6, -6.0e4, 1e-6
    b = torch.randn(Nout, generator=g)
    A, W, b = A.to(DEV), W.to(DEV), b.to(DEV)
    ref = A.double() @ W.double().t() + b.double()
    T = A.double().abs() @ W.double().abs().t() + b.double().abs()
    t32 = torch.nn.functional.linear(A, W, b)
    _judge(tid, 'exact', ops.linear(A, W, b), t32, ref, T)
    _judge(tid, 'bf16x3', ops.linear(A, W, b, w_split=ops.split_weight(W)), t32, ref, T)
    torch.cuda.synchronize()
    ops.workspace_status()
