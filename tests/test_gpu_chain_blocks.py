"""GPU (-m gpu): the building blocks of the training chain (csrc/vkn_train.hip) through the C ABI, element by element against float64
torch autograd of the same op on the same fp32 inputs (tests/chain_block_refs.py, pinned on the CPU by tests/test_chain_block_refs.py) —
at every launch arm: the gated-update core (`k_gprod_*`, `k_mix_*`), every arm of the attention backward (`k_attn_bwd<HD, TQ>`,
`k_attn_bwd_mfma<HD>`; each case asserts the arm that ran), LayerNorm with NULL parameters / strides / ragged widths, and the weight
gradient kernels with strides, `accumulate` and the batch form.

Every output lives in a `Guard`: a buffer pre-filled with a NaN bit pattern, with guard rows above and below and guard columns to the
right of what the kernel may write.  After the call every element inside must have been written and every element outside must be
bitwise untouched.  Nothing is sampled: every element of every output is compared.

Tolerances: the project's (tests/test_gpu_chain_train.py: forward 2e-5 of the tensor's max-abs, LayerNorm forward 1e-5, single-op
gradients 5e-5 of the max-abs) tightened to 4 x the largest error measured on the MI355X (`LIM`; the measured value stands beside each
limit, profiles/chain_blocks_margins.json holds the records of that run); the project's own where a case is conditioned worse by
construction (saturated gates, a +-150 score spread) or runs a GEMM inside (the autograd wrappers).  Derived bounds: the gate product is ONE
fp32 multiply per element (|got - ref| <= 2^-24 |ref|); the weight gradients on integer operands are exact (tests/test_exact_premise.py
proves the premise on the CPU)."""
import ctypes
import re

import pytest
import torch
import torch.nn.functional as F

import chain_block_refs as R
import exact_cases as ec
from helpers import record_margins, run_and_kernels

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SENT = 0x7FC0BEEF          # a NaN with a payload: what an untouched element holds
GR = 4                     # guard rows on either side (4 rows: any row stride keeps the first written row 16-byte aligned)

# The asserted limits, relative to the reference tensor's max-abs.  The project's own (tests/test_gpu_chain_train.py) are forward 2e-5,
# LayerNorm forward 1e-5, single-op gradients 5e-5; every limit below is tighter: 4 x the largest error of that quantity over all the
# cases of this module, measured on the MI355X (the value beside each limit; profiles/chain_blocks_margins.json has every record).
# 4 x because boxes and compiler versions move the order of fp32 reductions.
LIM = dict(
    core_F=7.6e-7,            # 1.91e-7  features of the mix forward
    core_mean=9.3e-7,         # 2.32e-7  stats: the four means
    core_rstd=5.1e-7,         # 1.27e-7  stats: the four 1 / sqrt(var + eps)
    core_dgt=1.0e-6,          # 2.58e-7  d_gates
    core_dpi=7.4e-7,          # 1.84e-7  second halves of d_params / d_inputs
    core_dn=3.7e-6,           # 9.33e-7  the eight parameter gradients (column sums over up to 3744 rows; the largest is at M = 1, C = 4)
    attn_out=2.4e-6,          # 6.02e-7  forward (VALU 6.0e-7, matrix cores 4.9e-7)
    attn_dq=2.4e-6,           # 5.98e-7  (VALU arms 6.0e-7, matrix-core arms 5.7e-7)
    attn_dk=2.3e-6,           # 5.86e-7  (VALU 5.7e-7, matrix cores 5.9e-7)
    attn_dv=2.4e-6,           # 6.10e-7  (VALU 6.0e-7, matrix cores 6.1e-7)
    ln_out=6.5e-7,            # 1.62e-7
    ln_mean=5.4e-7,           # 1.35e-7
    ln_rstd=4.9e-7,           # 1.24e-7
    ln_dx=9.4e-7,             # 2.35e-7
    ln_dgamma=1.3e-6,         # 3.16e-7
    ln_dbeta=9.3e-7,          # 2.32e-7
    dw=1.3e-6,                # 3.26e-7  dW on float operands (3744 rows), accumulating form included
    db=7.7e-7,                # 1.92e-7
    dw_batch=2.4e-6)          # 6.03e-7  the batch form, dW and db


def P(t):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else None


def stream():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


class Guard:
    """[rows, cols] fp32 output with row stride ld >= cols inside a sentinel-filled buffer of rows + 2 GR rows"""

    def __init__(self, rows, cols, ld=None):
        self.rows, self.cols, self.ld = rows, cols, ld or cols
        self.bits = torch.full((rows + 2 * GR, self.ld), SENT, dtype=torch.int32, device=DEV)
        self.buf = self.bits.view(torch.float32)
        self.v = self.buf[GR:GR + rows, :cols]

    def ptr(self, col=0):
        return ctypes.c_void_p(self.v.data_ptr() + 4 * col)

    def check(self, name, lo=0, hi=None, written=True):
        """columns [lo, hi) of every row were written (no NaN left), everything else still holds the sentinel bits"""
        hi = self.cols if hi is None else hi
        outside = torch.ones_like(self.bits, dtype=torch.bool)
        if written:
            outside[GR:GR + self.rows, lo:hi] = False
            assert not bool(torch.isnan(self.buf[GR:GR + self.rows, lo:hi]).any()), f'{name}: an element inside was not written (or is NaN)'
        assert bool((self.bits[outside] == SENT).all()), f'{name}: an element outside the output was written'


def rel(got, ref):
    """max |got - ref| over max |ref|, every element"""
    got, ref = got.detach().double(), ref.detach().double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    return float((got - ref).abs().max()) / max(float(ref.abs().max()), 1e-30) if ref.numel() else 0.0


def gen(seed):
    return torch.Generator().manual_seed(seed)


def randn(g, *shape, std=1.0, mean=0.0):
    return (torch.randn(*shape, generator=g) * std + mean).to(DEV)


def E(vkn, name):
    return vkn._lib.CONSTS[name]


# ====================================================================================================== 1. the gated-update core
CORE_SHAPES = [(1, 4), (3, 36), (15, 60), (16, 64), (17, 68), (117, 100), (127, 128), (128, 64), (129, 252), (468, 256), (468, 252),
               (3744, 256), (3744, 100), (117, 36)]
EPS = 1e-5


def core_case(M, C, seed, gate_scale=1.0):
    """params, inputs, gates [M, 2C]; the eight norm vectors off their init values (weights 1 + N(0, 0.5), biases N(0, 0.3)), all
    distinct; the two gate biases; upstream gradients dF, dG [M, C]"""
    g = gen(seed)
    c = dict(p=randn(g, M, 2 * C), i=randn(g, M, 2 * C), gt=randn(g, M, 2 * C, std=1.5),
             norms=[randn(g, C, std=0.3 if k % 2 else 0.5, mean=0.0 if k % 2 else 1.0) for k in range(8)],
             bi=randn(g, C, std=0.3), bu=randn(g, C, std=0.3), dF=randn(g, M, C, std=1e-2), dG=randn(g, M, C, std=1e-2))
    c['norms'][0] *= gate_scale       # norm_in / input_norm_in weights: the gates' pre-activations
    c['norms'][4] *= gate_scale
    return c


def core_reference(c, use_bi=True, use_bu=True):
    d = lambda t: t.double().requires_grad_(True)      # noqa: E731
    p, i, gt = d(c['p']), d(c['i']), d(c['gt'])
    norms = [d(t) for t in c['norms']]
    bi, bu = (c['bi'].double() if use_bi else None), (c['bu'].double() if use_bu else None)
    feats, stats, zu, zi = R.updator_mix(p, i, gt, norms, bi, bu, EPS, with_stats=True)
    G = R.gate_product(p, i)
    grads = torch.autograd.grad((feats * c['dF'].double()).sum() + (G * c['dG'].double()).sum(), [p, i, gt] + norms)
    return dict(F=feats.detach(), G=G.detach(), stats=stats, zu=zu, zi=zi, dp=grads[0], di=grads[1], dgt=grads[2], dn=grads[3:])


def run_core(vkn, c, M, C, use_bi=True, use_bu=True, dn_null=()):
    """the four entry points on guarded outputs; dn_null: 'all' (d_norms = NULL) or the indices of NULL members.  -> dict of outputs
    after every written / untouched check has passed"""
    L, lib = vkn._lib.lib(), vkn._lib
    st = stream()
    nw = lib.VknUpdatorNorms(*[t.data_ptr() for t in c['norms']], c['bi'].data_ptr() if use_bi else None, c['bu'].data_ptr() if use_bu else None)
    G, Fo, S = Guard(M, C), Guard(M, C), Guard(M, 8)
    assert L.vkn_updator_gate_product_f32(P(c['p']), P(c['i']), G.ptr(), M, C, st) == 0
    assert L.vkn_updator_mix_fwd_f32(P(c['gt']), P(c['p']), P(c['i']), ctypes.byref(nw), EPS, Fo.ptr(), S.ptr(), M, C, st) == 0
    dGT, dP, dI = Guard(M, 2 * C), Guard(M, 2 * C), Guard(M, 2 * C)
    dn = [Guard(1, C) for _ in range(8)]
    if dn_null == 'all':
        gwp = None
    else:
        gw = lib.VknUpdatorNormGrads(*[None if k in dn_null else dn[k].v.data_ptr() for k in range(8)])
        gwp = ctypes.byref(gw)
    stats_in = S.v.contiguous()
    assert L.vkn_updator_mix_bwd_f32(P(c['dF']), P(c['gt']), P(c['p']), P(c['i']), ctypes.byref(nw), P(stats_in), dGT.ptr(), dP.ptr(), dI.ptr(),
                                     gwp, M, C, st) == 0
    torch.cuda.synchronize()
    G.check('gate_feats'), Fo.check('features'), S.check('stats'), dGT.check('d_gates')
    dP.check('d_params after the mix backward: second half only', C, 2 * C)
    dI.check('d_inputs after the mix backward: second half only', C, 2 * C)
    for k in range(8):
        dn[k].check(f'd_norms[{k}]', written=not (dn_null == 'all' or k in dn_null))
    second = (dP.bits.clone(), dI.bits.clone())
    assert L.vkn_updator_gate_product_bwd_f32(P(c['dG']), P(c['p']), P(c['i']), dP.ptr(), dI.ptr(), M, C, st) == 0
    torch.cuda.synchronize()
    dP.check('d_params'), dI.check('d_inputs')
    for gd, was, nm in ((dP, second[0], 'd_params'), (dI, second[1], 'd_inputs')):
        assert torch.equal(gd.bits[:, C:], was[:, C:]), f'{nm}: the gate-product backward touched the second half'
    return dict(G=G.v, F=Fo.v, stats=S.v, dgt=dGT.v, dp=dP.v, di=dI.v, dn=[d.v[0] for d in dn])


def one_multiply(got, ref):
    """ONE fp32 multiply per element: |got - ref| <= 2^-24 |ref| with the float64 product (exact: 48 bits) as ref"""
    return bool(((got.double() - ref).abs() <= 2.0 ** -24 * ref.abs()).all())


def core_errors(out, ref, C, dn_null=()):
    e = dict(F=rel(out['F'], ref['F']), dgt=rel(out['dgt'], ref['dgt']), dp2=rel(out['dp'][:, C:], ref['dp'][:, C:]),
             di2=rel(out['di'][:, C:], ref['di'][:, C:]),
             stats_mean=max(rel(out['stats'][:, 2 * j], ref['stats'][:, 2 * j]) for j in range(4)),
             stats_rstd=max(rel(out['stats'][:, 2 * j + 1], ref['stats'][:, 2 * j + 1]) for j in range(4)))
    dn = [rel(out['dn'][k], ref['dn'][k]) for k in range(8) if dn_null != 'all' and k not in dn_null]
    e['dn'] = max(dn) if dn else 0.0
    return e


def assert_core(out, ref, C, e):
    assert one_multiply(out['G'], ref['G']), 'gate product forward'
    assert one_multiply(out['dp'][:, :C], ref['dp'][:, :C]) and one_multiply(out['di'][:, :C], ref['di'][:, :C]), 'gate product backward'
    assert e['F'] < LIM['core_F'], e
    assert e['stats_mean'] < LIM['core_mean'] and e['stats_rstd'] < LIM['core_rstd'], e
    assert e['dgt'] < LIM['core_dgt'] and e['dp2'] < LIM['core_dpi'] and e['di2'] < LIM['core_dpi'], e
    assert e['dn'] < LIM['core_dn'], e


@pytest.mark.parametrize('M,C', CORE_SHAPES, ids=lambda v: str(v))
def test_updator_core_every_element_vs_fp64(vkn, M, C):
    c = core_case(M, C, 1000 + 7 * M + C)
    ref = core_reference(c)
    out = run_core(vkn, c, M, C)
    e = core_errors(out, ref, C)
    record_margins(f'chain_blocks.core[{M}x{C}]', e)
    assert_core(out, ref, C, e)


@pytest.mark.parametrize('use_bi,use_bu', [(True, False), (False, True), (False, False)], ids=['bias_i', 'bias_u', 'no_bias'])
def test_updator_core_gate_bias_options(vkn, use_bi, use_bu):
    M, C = 117, 100
    c = core_case(M, C, 77)
    ref = core_reference(c, use_bi, use_bu)
    out = run_core(vkn, c, M, C, use_bi, use_bu)
    e = core_errors(out, ref, C)
    record_margins(f'chain_blocks.core_bias[{int(use_bi)}{int(use_bu)}]', e)
    assert_core(out, ref, C, e)
    both = core_reference(c)
    assert rel(both['F'], ref['F']) > 1e-3        # (the case exists: the biases matter at this input)


@pytest.mark.parametrize('dn_null', ['all'] + [(k,) for k in range(8)], ids=lambda v: 'dn_' + (v if isinstance(v, str) else str(v[0])))
def test_updator_mix_backward_with_null_norm_gradients(vkn, dn_null):
    """d_norms NULL, and each of its eight members NULL on its own: the NULL one is not written, the others are still right"""
    M, C = 129, 100
    c = core_case(M, C, 78)
    ref = core_reference(c)
    out = run_core(vkn, c, M, C, dn_null=dn_null)
    e = core_errors(out, ref, C, dn_null)
    record_margins(f'chain_blocks.core_null[{dn_null if isinstance(dn_null, str) else dn_null[0]}]', e)
    assert_core(out, ref, C, e)


def test_updator_mix_takes_any_width_up_to_256(vkn):
    """the mix kernels read and write element-wise: C need not be a multiple of 4 (the gate product does need it: VKN_E_SHAPE, and
    16-byte aligned operands: VKN_E_ALIGN — both before anything is launched), C = 257 is VKN_E_SHAPE"""
    L, lib = vkn._lib.lib(), vkn._lib
    M, C = 19, 7
    c = core_case(M, C, 79)
    ref = core_reference(c)
    st = stream()
    nw = lib.VknUpdatorNorms(*[t.data_ptr() for t in c['norms']], c['bi'].data_ptr(), c['bu'].data_ptr())
    Fo, S, dGT, dP, dI = Guard(M, C), Guard(M, 8), Guard(M, 2 * C), Guard(M, 2 * C), Guard(M, 2 * C)
    dn = [Guard(1, C) for _ in range(8)]
    gw = lib.VknUpdatorNormGrads(*[d.v.data_ptr() for d in dn])
    assert L.vkn_updator_mix_fwd_f32(P(c['gt']), P(c['p']), P(c['i']), ctypes.byref(nw), EPS, Fo.ptr(), S.ptr(), M, C, st) == 0
    stats_in = S.v.contiguous()
    assert L.vkn_updator_mix_bwd_f32(P(c['dF']), P(c['gt']), P(c['p']), P(c['i']), ctypes.byref(nw), P(stats_in), dGT.ptr(), dP.ptr(), dI.ptr(),
                                     ctypes.byref(gw), M, C, st) == 0
    torch.cuda.synchronize()
    Fo.check('features'), S.check('stats'), dGT.check('d_gates'), dP.check('d_params', C, 2 * C), dI.check('d_inputs', C, 2 * C)
    out = dict(F=Fo.v, stats=S.v, dgt=dGT.v, dp=dP.v, di=dI.v, dn=[d.v[0] for d in dn])
    e = core_errors(out, ref, C)
    record_margins('chain_blocks.core_mix_only[19x7]', e)
    assert e['F'] < LIM['core_F'] and e['dgt'] < LIM['core_dgt'] and max(e['dp2'], e['di2']) < LIM['core_dpi'] and e['dn'] < LIM['core_dn'], e
    # ---- the gates
    G = Guard(M, 8)
    assert L.vkn_updator_gate_product_f32(P(c['p']), P(c['i']), G.ptr(), M, C, st) == E(vkn, 'VKN_E_SHAPE')
    assert L.vkn_updator_gate_product_bwd_f32(P(c['dG']), P(c['p']), P(c['i']), dP.ptr(), dI.ptr(), M, C, st) == E(vkn, 'VKN_E_SHAPE')
    big = core_case(4, 260, 80)               # (buffers of the size C = 257 would need, and more)
    F2, S2 = Guard(4, 260), Guard(4, 8)
    nw2 = lib.VknUpdatorNorms(*[t.data_ptr() for t in big['norms']], None, None)
    assert L.vkn_updator_mix_fwd_f32(P(big['gt']), P(big['p']), P(big['i']), ctypes.byref(nw2), EPS, F2.ptr(), S2.ptr(), 4, 257, st) == E(vkn, 'VKN_E_SHAPE')
    # 16-byte alignment of the float4 gate product: the same buffers one float further on (each view lies inside a longer buffer)
    a8 = core_case(6, 8, 81)
    off = lambda t: ctypes.c_void_p(t.data_ptr() + 4)      # noqa: E731
    G8 = Guard(6, 8)
    assert L.vkn_updator_gate_product_f32(off(a8['p']), P(a8['i']), G8.ptr(), 5, 8, st) == E(vkn, 'VKN_E_ALIGN')
    assert L.vkn_updator_gate_product_f32(P(a8['p']), off(a8['i']), G8.ptr(), 5, 8, st) == E(vkn, 'VKN_E_ALIGN')
    assert L.vkn_updator_gate_product_f32(P(a8['p']), P(a8['i']), G8.ptr(1), 5, 8, st) == E(vkn, 'VKN_E_ALIGN')
    d8p, d8i = Guard(6, 16), Guard(6, 16)
    assert L.vkn_updator_gate_product_bwd_f32(off(a8['dG']), P(a8['p']), P(a8['i']), d8p.ptr(), d8i.ptr(), 5, 8, st) == E(vkn, 'VKN_E_ALIGN')
    assert L.vkn_updator_gate_product_bwd_f32(P(a8['dG']), P(a8['p']), P(a8['i']), d8p.ptr(1), d8i.ptr(), 5, 8, st) == E(vkn, 'VKN_E_ALIGN')
    torch.cuda.synchronize()
    for gd, nm in ((G, 'G'), (F2, 'F2'), (S2, 'S2'), (G8, 'G8'), (d8p, 'd8p'), (d8i, 'd8i')):
        gd.check(nm, written=False)


def test_updator_core_with_saturated_gates(vkn):
    """norm_in / input_norm_in weights x 100: the gates' pre-activations reach several hundred.  Everything stays finite (expf overflows
    to inf, 1 / inf = 0), gradients match float64; with norm_out = (0, 1) and input_norm_out = (0, 0) the output IS the update gate (and
    the reverse for the input gate): exactly 0 / 1 wherever float64's sigmoid rounds to that in fp32."""
    M, C = 117, 256
    c = core_case(M, C, 90, gate_scale=100.0)
    ref = core_reference(c)
    assert float(ref['zu'].abs().max()) > 300 and float(ref['zi'].abs().max()) > 300
    out = run_core(vkn, c, M, C)
    for k, v in out.items():
        for t in (v if isinstance(v, list) else [v]):
            assert bool(torch.isfinite(t).all()), k
    e = core_errors(out, ref, C)
    record_margins('chain_blocks.core_saturated', e)
    assert one_multiply(out['G'], ref['G'])
    # the project's single-op tolerances (measured: F 1.1e-7, d_gates 2.4e-7, d_params / d_inputs 1.4e-7, parameter gradients 1.7e-6)
    assert e['F'] < 2e-5 and max(e['dgt'], e['dp2'], e['di2'], e['dn']) < 5e-5, e
    assert e['stats_mean'] < LIM['core_mean'] and e['stats_rstd'] < LIM['core_rstd'], e
    for which in (0, 1):          # the output IS the update gate (0) / the input gate (1)
        o = core_case(M, C, 90, gate_scale=100.0)
        ones, zeros = torch.ones(C, device=DEV), torch.zeros(C, device=DEV)
        o['norms'][2], o['norms'][3] = zeros, (ones if which == 0 else zeros)
        o['norms'][6], o['norms'][7] = zeros.clone(), (zeros.clone() if which == 0 else ones.clone())
        r = core_reference(o)
        got = run_core(vkn, o, M, C)['F']
        want32 = r['F'].float()
        sat0, sat1 = want32 == 0.0, want32 == 1.0
        assert int(sat0.sum()) > 100 and int(sat1.sum()) > 1000, (int(sat0.sum()), int(sat1.sum()))
        assert bool((got[sat0] == 0.0).all()) and bool((got[sat1] == 1.0).all()), which
        assert bool(((got >= 0) & (got <= 1)).all()) and rel(got, r['F']) < 2e-5


def _ku(vkn, C, seed):
    torch.manual_seed(seed)
    ku = vkn.kernel_updator.KernelUpdator(in_channels=C, feat_channels=C).to(DEV)
    g = gen(seed)
    with torch.no_grad():
        for n, p in ku.named_parameters():
            if 'norm' in n:
                p.copy_(randn(g, *p.shape, std=0.5 if n.endswith('weight') else 0.3, mean=1.0 if n.endswith('weight') else 0.0))
            elif n.endswith('bias'):
                p.copy_(randn(g, *p.shape, std=0.3))
    return ku


@pytest.mark.parametrize('route', ['queue', 'no_queue'])
def test_updator_core_fn_vs_fp64(vkn, route):
    """`UpdatorCoreFn` built the way `chain_train.kernel_updator` builds it (`WeightImages.pair`: ONE GEMM for both gate layers), the
    gate-weight gradients through the `DwQueue` and computed in its own backward."""
    ct = vkn.chain_train
    M, C = 117, 256
    ku = _ku(vkn, C, 11)
    g = gen(12)
    p0, i0, dF = randn(g, M, 2 * C), randn(g, M, 2 * C), randn(g, M, C, std=1e-2)
    wig, big, wug, bug = ku.input_gate.weight, ku.input_gate.bias, ku.update_gate.weight, ku.update_gate.bias
    norms = [t for n in R.NORM_NAMES for t in (getattr(ku, n).weight, getattr(ku, n).bias)]
    leaves = [wig, big, wug, bug] + norms
    queue = ct.DwQueue() if route == 'queue' else None
    imgs = ct.WeightImages([wig, wug], queue)
    img_n, img_t = imgs.pair(wig, wug)
    assert img_n is not None and img_t is not None
    p, i = p0.clone().requires_grad_(True), i0.clone().requires_grad_(True)
    pe, ie = ct.ChainEntryFn.apply(queue, 2, p, i, wig, big, wug, bug) if queue is not None else (p, i)
    feats = ct.UpdatorCoreFn.apply(pe, ie, wig, big, wug, bug, ku.norm_in.eps, img_n, img_t, queue, *norms)
    feats.backward(dF)
    torch.cuda.synchronize()
    got = [p.grad, i.grad] + [t.grad for t in leaves]
    assert all(t is not None for t in got)
    d = lambda t: t.detach().double().requires_grad_(True)      # noqa: E731
    pd, idd = d(p0), d(i0)
    ld = [d(t) for t in leaves]
    fr = R.updator_core(pd, idd, ld[0], ld[2], ld[4:], ld[1], ld[3], ku.norm_in.eps)
    want = torch.autograd.grad((fr * dF.double()).sum(), [pd, idd] + ld)
    names = ['params', 'inputs', 'input_gate.weight', 'input_gate.bias', 'update_gate.weight', 'update_gate.bias'] + [f'norm{k}' for k in range(8)]
    e = {n: rel(a, b) for n, a, b in zip(names, got, want)}
    e['F'] = rel(feats, fr)
    record_margins(f'chain_blocks.core_fn[{route}]', e)
    # the project's tolerances (a bf16x3 GEMM sits inside).  Measured: F 7.1e-8, largest gradient error 3.8e-7 (the gate weights through
    # the queue's batch kernel; 1.8e-7 through the single form)
    assert e['F'] < 2e-5, e
    assert max(v for k, v in e.items() if k != 'F') < 5e-5, e
    for t in leaves:
        t.grad = None


def test_kernel_updator_unfused_branch_vs_fp64(vkn):
    """`chain_train.kernel_updator` without weight images: the branch that composes LinearFn / LayerNormActFn and torch's element-wise
    ops — against the float64 reference, not against the fused branch.  The closing ReLU(fc_norm(.)) has a kink: elements whose float64
    pre-activation lies within 1e-4 of zero get no upstream gradient (fp32 may take the other branch there)."""
    ct = vkn.chain_train
    M, C = 117, 256
    ku = _ku(vkn, C, 13)
    g = gen(14)
    u0, k0, dy = randn(g, M, C), randn(g, M, C), randn(g, M, C, std=1e-2)
    d = lambda t: t.detach().double().requires_grad_(True)      # noqa: E731
    ud, kd = d(u0), d(k0)
    sd = {n: d(t) for n, t in ku.named_parameters()}
    z = R.kernel_updator(sd, ud, kd, ku.norm_in.eps, pre_relu=True)
    near = z.detach().abs() < 1e-4
    assert float(near.double().mean()) < 1e-3
    dy = dy * (~near).float()
    want = torch.autograd.grad((torch.relu(z) * dy.double()).sum(), [ud, kd] + list(sd.values()))
    u, k = u0.clone().requires_grad_(True), k0.clone().requires_grad_(True)
    y = ct.kernel_updator(ku, u, k, imgs=None)
    y.backward(dy)
    torch.cuda.synchronize()
    got = [u.grad, k.grad] + [t.grad for t in ku.parameters()]
    e = {n: rel(a, b) for n, a, b in zip(['update_feature', 'input_feature'] + list(sd), got, want)}
    e['out'] = rel(y, torch.relu(z))
    e['out_far_from_kink'] = rel(y * (~near).float(), torch.relu(z) * (~near).double())
    record_margins('chain_blocks.kernel_updator_unfused', e)
    # four layers deep (three bf16x3 GEMMs, five LayerNorms): the project's single-op tolerances.  Measured: out 2.0e-7,
    # largest gradient error 4.6e-7 (input_norm_in.bias)
    assert e['out'] < 2e-5, e
    assert max(v for n, v in e.items() if not n.startswith('out')) < 5e-5, e
    ku.zero_grad(set_to_none=True)


# ====================================================================================================================== 2. attention
def arms_of(names):
    """the attention-backward arms among kernel names: 'valu<HD,TQ>' / 'mfma<HD>' (demangled or mangled names)"""
    out = set()
    for n in names:
        s = n.replace(' ', '')
        for m in re.finditer(r'k_attn_bwd_mfma<(\d+)>|k_attn_bwd_mfmaILi(\d+)E', s):
            out.add(f'mfma<{m.group(1) or m.group(2)}>')
        for m in re.finditer(r'k_attn_bwd<(\d+),(\d+)>|k_attn_bwdILi(\d+)ELi(\d+)E', s):
            out.add(f'valu<{m.group(1) or m.group(3)},{m.group(2) or m.group(4)}>')
    return out


def attn_case(B, Nq, Nk, heads, hd, packed, seed, std=0.7):
    """Q / K / V as column slices of one packed buffer (packed: [B N, 3C + 4]; cross: q [B Nq, C + 4], kv [B Nk, 2C + 8]); dO with a
    row stride of its own"""
    C = heads * hd
    g = gen(seed)
    if packed:
        assert Nq == Nk
        buf = randn(g, B * Nq, 3 * C + 4, std=std)
        q, k, v = buf[:, :C], buf[:, C:2 * C], buf[:, 2 * C:3 * C]
    else:
        qb, kvb = randn(g, B * Nq, C + 4, std=std), randn(g, B * Nk, 2 * C + 8, std=std)
        q, k, v = qb[:, :C], kvb[:, :C], kvb[:, C:2 * C]
    do = randn(g, B * Nq, C + 12, std=1e-2)[:, :C]
    return q, k, v, do


def run_attention(vkn, B, Nq, Nk, heads, hd, packed, seed, std=0.7):
    """forward + backward on guarded, strided outputs -> (errors, arms that ran, float64 scores)"""
    L = vkn._lib.lib()
    C = heads * hd
    q, k, v, do = attn_case(B, Nq, Nk, heads, hd, packed, seed, std)
    st = stream()
    out = Guard(B * Nq, C, C + 8)
    assert L.vkn_attention_f32(P(q), q.stride(0), P(k), P(v), k.stride(0), out.ptr(), out.ld, B, Nq, Nk, heads, hd, st) == 0
    torch.cuda.synchronize()
    out.check('out')
    dq, dkv = Guard(B * Nq, C, C + 12), Guard(B * Nk, 2 * C, 2 * C + 8)        # dK | dV share one row stride (the ABI has one lddkv)

    def bwd():
        return L.vkn_attention_bwd_f32(P(q), q.stride(0), P(k), P(v), k.stride(0), out.ptr(), out.ld, P(do), do.stride(0), dq.ptr(), dq.ld,
                                       dkv.ptr(0), dkv.ptr(C), dkv.ld, B, Nq, Nk, heads, hd, st)
    rc, names = run_and_kernels(bwd)
    assert rc == 0
    dq.check('dQ'), dkv.check('dK | dV')
    d = lambda t: t.double().requires_grad_(True)      # noqa: E731
    qd, kd, vd = d(q), d(k), d(v)
    ref, scores = R.attention(qd, kd, vd, B, heads, with_scores=True)
    gq, gk, gv = torch.autograd.grad((ref * do.double()).sum(), [qd, kd, vd])
    for t in (out.v, dq.v, dkv.v):
        assert bool(torch.isfinite(t).all())
    e = dict(out=rel(out.v, ref), dq=rel(dq.v, gq), dk=rel(dkv.v[:, :C], gk), dv=rel(dkv.v[:, C:], gv))
    if Nk == 1:
        # one key: the softmax is 1, dS = P (dO . v - D) scale with D = dO . O = dO . v, so dQ and dK are exactly ZERO in exact arithmetic
        # and there is no max-abs to measure against.  In fp32 the two dot products are summed in different orders: what is left is
        # their rounding, relative to the size of the terms that cancel — sum_d |dO_d v_d| scale max(|q|, |k|) — which is the scale here
        assert float(gq.abs().max()) < 1e-15 and float(gk.abs().max()) < 1e-15
        terms = (do.double().abs().reshape(B, Nq, heads, hd) * v.double().abs().reshape(B, 1, heads, hd)).sum(-1).max()
        scale = float(terms) / hd ** 0.5 * max(float(q.abs().max()), float(k.abs().max()))
        e['dq'], e['dk'] = float(dq.v.abs().max()) / scale, float(dkv.v[:, :C].abs().max()) / scale
    return e, arms_of(names), scores


# lds_of(TQ) of attn_bwd_launch<HD> = 4 (2 Nk (HD + 1) + 2 TQ (HD + 1) + TQ (Nk + 1) + TQ) bytes against the cap of 160 KiB = 163 840 B:
#   hd 64, Nk 130: TQ 64 -> 4 (16 900 + 8 320 + 8 384 + 64) = 134 672 B                                            -> k_attn_bwd<64, 64>
#   hd 64, Nk 200: TQ 64 -> 4 (26 000 + 8 320 + 12 864 + 64) = 188 992 B (over), TQ 32 -> 4 (26 000 + 4 160 + 6 432 + 32) = 146 496 B
#                                                                                                                   -> k_attn_bwd<64, 32>
#   hd 64, Nk 256: TQ 64 -> 232 448 B, TQ 32 -> 4 (33 280 + 4 160 + 8 224 + 32) = 182 784 B (both over),
#                  TQ 16 -> 4 (33 280 + 2 080 + 4 112 + 16) = 157 952 B                                             -> k_attn_bwd<64, 16>
# The matrix-core launcher declines all three on its own sum 4 (2 KB 32 (HD + 1) + 2 QB 32 (HD + 1) + 2 KB 32 HD + NW 32 33 + QB 32):
# with KB = 5 key blocks at hd 64 the K / V tiles and accumulators alone are 4 (20 800 + 20 480) = 165 120 B.
#   hd 32, N 166 packed (QB = KB = 6): 4 (12 672 + 12 672 + 12 288 + 6 336 + 192) = 176 640 B (over) -> VALU, lds_of(64) = 103 728 B
#   hd 32, N 256 (QB = KB = 8): over as well -> VALU, lds_of(64) = 4 (16 896 + 4 224 + 16 448 + 64) = 150 528 B       -> k_attn_bwd<32, 64>
#   hd 16, N 256 (QB = KB = 8): 4 (8 704 + 8 704 + 8 192 + 8 448 + 256) = 137 216 B: stays on the matrix cores       -> k_attn_bwd_mfma<16>
#   hd 64, (Nq, Nk) = (33, 96): QB 2, KB 3: 4 (12 480 + 8 320 + 12 288 + 3 168 + 64) = 145 280 B                      -> k_attn_bwd_mfma<64>
ATTN_CASES = [
    # (B, Nq, Nk, heads, hd, packed, arm)
    (2, 117, 117, 8, 4, True, 'valu<4,64>'), (1, 33, 256, 4, 4, False, 'valu<4,64>'),
    (2, 117, 117, 4, 8, True, 'valu<8,64>'), (2, 50, 131, 8, 8, False, 'valu<8,64>'),
    (1, 70, 130, 4, 64, False, 'valu<64,64>'), (1, 50, 200, 2, 64, False, 'valu<64,32>'), (1, 9, 256, 2, 64, False, 'valu<64,16>'),
    (1, 37, 256, 2, 64, False, 'valu<64,16>'),
    (1, 166, 166, 8, 32, True, 'valu<32,64>'), (1, 256, 256, 4, 32, True, 'valu<32,64>'), (1, 256, 256, 8, 16, True, 'mfma<16>'),
    (2, 33, 128, 8, 32, False, 'mfma<32>'), (2, 117, 20, 8, 32, False, 'mfma<32>'),
    (2, 33, 128, 8, 16, False, 'mfma<16>'), (2, 117, 20, 8, 16, False, 'mfma<16>'),
    (2, 33, 96, 4, 64, False, 'mfma<64>'), (2, 96, 20, 4, 64, False, 'mfma<64>'),
    (2, 1, 117, 8, 32, False, 'mfma<32>'), (2, 117, 1, 8, 32, False, 'mfma<32>'), (1, 1, 1, 4, 16, True, 'mfma<16>'),
    (3, 1, 1, 2, 64, False, 'mfma<64>'),
    (1, 32, 33, 8, 32, False, 'mfma<32>'), (1, 33, 32, 8, 32, False, 'mfma<32>'), (2, 32, 33, 4, 16, False, 'mfma<16>'),
    (2, 33, 32, 4, 64, False, 'mfma<64>'), (2, 117, 117, 8, 32, True, 'mfma<32>'),
]


@pytest.mark.parametrize('B,Nq,Nk,heads,hd,packed,arm', ATTN_CASES, ids=lambda v: str(v))
def test_attention_every_backward_arm_vs_fp64(vkn, B, Nq, Nk, heads, hd, packed, arm):
    e, arms, _ = run_attention(vkn, B, Nq, Nk, heads, hd, packed, 2000 + Nq + 3 * Nk + hd)
    e['arm'] = ','.join(sorted(arms))
    record_margins(f'chain_blocks.attn[{B}x{Nq}x{Nk}x{heads}x{hd}{"p" if packed else "c"}]', e)
    assert arms == {arm}, f'the backward ran {sorted(arms)}, this case was written for {arm}'
    assert e['out'] < LIM['attn_out'], e
    assert e['dq'] < LIM['attn_dq'] and e['dk'] < LIM['attn_dk'] and e['dv'] < LIM['attn_dv'], e


@pytest.mark.parametrize('heads,hd,arm', [(8, 32, 'mfma<32>'), (8, 8, 'valu<8,64>')], ids=['mfma', 'valu'])
def test_attention_with_a_wide_score_spread(vkn, heads, hd, arm):
    """q, k ~ N(0, 5.6^2): the scaled scores span about +-150.  The forward and the softmax each backward kernel recomputes stay finite
    and match float64.  A score of 150 carries an absolute fp32 error of ~ hd 2^-24 150 in ANY fp32 evaluation, which the softmax turns
    into a relative error of its weights: the project's tolerances (2e-5 / 5e-5) are the limit here, not the tightened ones."""
    e, arms, scores = run_attention(vkn, 2, 117, 117, heads, hd, True, 2500 + hd, std=5.6)
    e['score_min'], e['score_max'], e['arm'] = float(scores.min()), float(scores.max()), ','.join(sorted(arms))
    record_margins(f'chain_blocks.attn_wide[{hd}]', e)
    assert e['score_max'] > 120 and e['score_min'] < -120
    assert arms == {arm}
    # measured (matrix cores / VALU): out 3.7e-6 / 2.2e-6, dq 7.3e-6 / 7.0e-6, dk 8.5e-6 / 7.7e-6, dv 2.9e-6 / 1.1e-6
    assert e['out'] < 2e-5 and max(e['dq'], e['dk'], e['dv']) < 5e-5, e


def test_attention_gates_return_before_any_launch(vkn):
    L = vkn._lib.lib()
    SHAPE = E(vkn, 'VKN_E_SHAPE')
    st = stream()
    B, heads = 1, 4
    g = gen(5)
    # Nk = 257 in the backward (real buffers of that size)
    hd, C, Nq, Nk = 16, 64, 20, 257
    q, kv, o, do = randn(g, Nq, C), randn(g, Nk, 2 * C), randn(g, Nq, C), randn(g, Nq, C)
    dq, dkv = Guard(Nq, C), Guard(Nk, 2 * C)
    assert L.vkn_attention_bwd_f32(P(q), C, P(kv), ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, P(o), C, P(do), C, dq.ptr(), C, dkv.ptr(0),
                                   dkv.ptr(C), 2 * C, B, Nq, Nk, heads, hd, st) == SHAPE
    # hd = 12, forward and backward
    hd, C, Nq, Nk = 12, 48, 20, 30
    q, kv, o, do = randn(g, Nq, C), randn(g, Nk, 2 * C), randn(g, Nq, C), randn(g, Nq, C)
    out2, dq2, dkv2 = Guard(Nq, C), Guard(Nq, C), Guard(Nk, 2 * C)
    assert L.vkn_attention_f32(P(q), C, P(kv), ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, out2.ptr(), C, B, Nq, Nk, heads, hd, st) == SHAPE
    assert L.vkn_attention_bwd_f32(P(q), C, P(kv), ctypes.c_void_p(kv.data_ptr() + 4 * C), 2 * C, P(o), C, P(do), C, dq2.ptr(), C, dkv2.ptr(0),
                                   dkv2.ptr(C), 2 * C, B, Nq, Nk, heads, hd, st) == SHAPE
    # a row stride that is not a multiple of 4 in the forward (q, then k / v, then out)
    hd, C, Nq, Nk = 16, 64, 20, 30
    q, kv = randn(g, Nq, C + 2), randn(g, Nk, 2 * C + 2)
    out3 = Guard(Nq, C, C + 6)
    kp, vp = P(kv), ctypes.c_void_p(kv.data_ptr() + 4 * C)
    assert L.vkn_attention_f32(P(q), C + 2, kp, vp, 2 * C, out3.ptr(), C + 4, B, Nq, Nk, heads, hd, st) == SHAPE
    assert L.vkn_attention_f32(P(q), C, kp, vp, 2 * C + 2, out3.ptr(), C + 4, B, Nq, Nk, heads, hd, st) == SHAPE
    assert L.vkn_attention_f32(P(q), C, kp, vp, 2 * C, out3.ptr(), C + 6, B, Nq, Nk, heads, hd, st) == SHAPE
    torch.cuda.synchronize()
    for gd in (dq, dkv, out2, dq2, dkv2, out3):
        gd.check('gated output', written=False)


# ====================================================================================================================== 3. LayerNorm
LN_SHAPES = [(1, 1, 0, False), (15, 7, 1, True), (17, 31, 2, False), (255, 32, 0, True), (256, 33, 1, False), (257, 63, 2, True),
             (3744, 65, 0, False), (17, 100, 1, True), (257, 200, 2, False), (255, 255, 0, True), (3744, 256, 1, True), (1, 256, 2, True),
             (15, 256, 0, False), (256, 100, 2, True)]


def run_layernorm(vkn, M, C, act, resid, seed, gamma=True, beta=True, dgamma=True, dbeta=True, stats=True, x=None):
    """forward + backward with every row stride larger than C and different from the others -> (errors, outputs)"""
    L = vkn._lib.lib()
    st = stream()
    g = gen(seed)
    xin = randn(g, M, C + 4, std=2.0)[:, :C] if x is None else x
    r = randn(g, M, C + 8)[:, :C] if resid else None
    gm = randn(g, C, std=0.5, mean=1.0) if gamma else None
    bt = randn(g, C, std=0.3) if beta else None
    dy = randn(g, M, C + 12, std=1e-2)[:, :C]
    out, S = Guard(M, C, C + 16), Guard(M, 2)
    assert L.vkn_layernorm_act_fwd_f32(P(xin), xin.stride(0), P(r), r.stride(0) if resid else 0, P(gm), P(bt), EPS, act, out.ptr(), out.ld,
                                       S.ptr() if stats else None, M, C, st) == 0
    torch.cuda.synchronize()
    out.check('out'), S.check('stats', written=stats)
    d = lambda t: t.double().requires_grad_(True) if t is not None else None      # noqa: E731
    xd, rd, gd, bd = d(xin), d(r), d(gm), d(bt)
    ref = R.layernorm_act(xd, rd, gd, bd, EPS, act)
    leaves = [t for t in (xd, rd, gd, bd) if t is not None]
    grads = dict(zip([n for n, t in zip('xrgb', (xd, rd, gd, bd)) if t is not None], torch.autograd.grad((ref * dy.double()).sum(), leaves)))
    mean, rstd = R.ln_stats(xd.detach() + rd.detach() if resid else xd.detach(), EPS)
    e = dict(out=rel(out.v, ref))
    if stats:
        e['mean'], e['rstd'] = rel(S.v[:, 0], mean), rel(S.v[:, 1], rstd)
        stats_in = S.v.contiguous()
    else:                      # (the backward needs them: the float64 ones, rounded)
        stats_in = torch.stack([mean, rstd], 1).float().contiguous()
    dx, dg, db = Guard(M, C, C + 20), Guard(1, C), Guard(1, C)
    assert L.vkn_layernorm_act_bwd_f32(P(dy), dy.stride(0), P(xin), xin.stride(0), P(r), r.stride(0) if resid else 0, P(gm), P(bt), P(stats_in),
                                       act, dx.ptr(), dx.ld, dg.ptr() if dgamma else None, db.ptr() if dbeta else None, M, C, st) == 0
    torch.cuda.synchronize()
    dx.check('dx'), dg.check('dgamma', written=dgamma), db.check('dbeta', written=dbeta)
    e['dx'] = rel(dx.v, grads['x'])
    if resid:
        assert torch.equal(grads['x'], grads['r'])          # (one tensor is the gradient of both)
    # gamma / beta NULL: the kernel still reports the gradient w.r.t. an implicit gamma = 1 / beta = 0
    if dgamma or dbeta:
        ones = torch.ones(C, dtype=torch.float64, device=DEV, requires_grad=True)
        zeros = torch.zeros(C, dtype=torch.float64, device=DEV, requires_grad=True)
        gg, bb = (gd.detach().requires_grad_(True) if gamma else ones), (bd.detach().requires_grad_(True) if beta else zeros)
        full = R.layernorm_act(xd.detach(), rd.detach() if resid else None, gg, bb, EPS, act)
        wg, wb = torch.autograd.grad((full * dy.double()).sum(), [gg, bb])
        if dgamma:
            e['dgamma'] = rel(dg.v[0], wg)
        if dbeta:
            e['dbeta'] = rel(db.v[0], wb)
    return e, dict(out=out.v, dx=dx.v, dg=dg.v[0], db=db.v[0], x=xin, dy=dy, gm=gm, bt=bt, ref=ref.detach(), grads=grads)


def assert_layernorm(e):
    assert e['out'] < LIM['ln_out'], e
    assert e.get('mean', 0) < LIM['ln_mean'] and e.get('rstd', 0) < LIM['ln_rstd'], e
    assert e['dx'] < LIM['ln_dx'], e
    assert e.get('dgamma', 0) < LIM['ln_dgamma'] and e.get('dbeta', 0) < LIM['ln_dbeta'], e


@pytest.mark.parametrize('M,C,act,resid', LN_SHAPES, ids=lambda v: str(v))
def test_layernorm_ragged_widths_and_row_counts_vs_fp64(vkn, M, C, act, resid):
    e, _ = run_layernorm(vkn, M, C, act, resid, 3000 + M + 5 * C)
    record_margins(f'chain_blocks.ln[{M}x{C}a{act}r{int(resid)}]', e)
    assert_layernorm(e)


@pytest.mark.parametrize('opts', [dict(gamma=False), dict(beta=False), dict(gamma=False, beta=False), dict(dgamma=False), dict(dbeta=False),
                                  dict(dgamma=False, dbeta=False), dict(stats=False), dict(gamma=False, beta=False, dgamma=False, dbeta=False)],
                         ids=lambda o: '_'.join(f'no_{k}' for k in o))
@pytest.mark.parametrize('act', [0, 1, 2])
def test_layernorm_null_parameters(vkn, opts, act):
    M, C = 257, 100
    e, _ = run_layernorm(vkn, M, C, act, act != 1, 3100 + act, **opts)
    record_margins(f'chain_blocks.ln_null[{"_".join(opts)}a{act}]', e)
    assert_layernorm(e)


def test_layernorm_refuses_257_columns(vkn):
    L = vkn._lib.lib()
    st = stream()
    M, C = 9, 257
    g = gen(7)
    x, gm, bt, dy, stt = randn(g, M, C), randn(g, C), randn(g, C), randn(g, M, C), randn(g, M, 2)
    out, S, dx, dg, db = Guard(M, C), Guard(M, 2), Guard(M, C), Guard(1, C), Guard(1, C)
    assert L.vkn_layernorm_act_fwd_f32(P(x), C, None, 0, P(gm), P(bt), EPS, 0, out.ptr(), C, S.ptr(), M, C, st) == E(vkn, 'VKN_E_SHAPE')
    assert L.vkn_layernorm_act_bwd_f32(P(dy), C, P(x), C, None, 0, P(gm), P(bt), P(stt), 0, dx.ptr(), C, dg.ptr(), db.ptr(), M, C,
                                       st) == E(vkn, 'VKN_E_SHAPE')
    torch.cuda.synchronize()
    for gd in (out, S, dx, dg, db):
        gd.check('gated output', written=False)


def test_layernorm_badly_conditioned_rows(vkn):
    """rows with |mean| / std ~ 1e3: fp32 cannot hold the base tolerance (x - mean loses ten bits).  The yardstick is torch's own fp32
    `F.layer_norm` (and its autograd) on the same input: the kernel's error against float64 must be at most 4 x torch's, per quantity
    that the conditioning reaches (out, dx, dgamma); dbeta is a plain column sum and keeps the base tolerance."""
    M, C = 257, 200
    g = gen(9)
    s = torch.rand(M, 1, generator=g) * 4 + 0.5
    x = ((1000.0 * s * torch.where(torch.rand(M, 1, generator=g) > 0.5, 1.0, -1.0)) + s * torch.randn(M, C, generator=g)).to(DEV)
    xw = torch.zeros(M, C + 4, device=DEV)
    xw[:, :C] = x
    e, o = run_layernorm(vkn, M, C, 0, False, 3200, x=xw[:, :C])
    ratio = (o['x'].double().mean(1).abs() / o['x'].double().std(1)).median()
    assert 500 < float(ratio) < 2000
    xt, gt_, bt_ = o['x'].clone().requires_grad_(True), o['gm'].clone().requires_grad_(True), o['bt'].clone().requires_grad_(True)
    yt = F.layer_norm(xt, (C,), gt_, bt_, EPS)
    yt.backward(o['dy'].contiguous())
    # the reference gradients w.r.t. gamma / beta
    t = dict(out=rel(yt, o['ref']), dx=rel(xt.grad, o['grads']['x']), dgamma=rel(gt_.grad, o['grads']['g']), dbeta=rel(bt_.grad, o['grads']['b']))
    record_margins('chain_blocks.ln_conditioned', {**{f'kernel_{k}': v for k, v in e.items()}, **{f'torch_{k}': v for k, v in t.items()}})
    for k in ('out', 'dx', 'dgamma'):
        assert e[k] <= 4 * t[k], (k, e[k], t[k])
    assert e['dbeta'] < LIM['ln_dbeta'], e


# ============================================================================================================================= 4. dW
def run_dw(vkn, dy, A, ldy, lda, with_db=True, old=None):
    """vkn_linear_dw_f32 on operands re-laid with row strides ldy / lda; old = (dW, db) pre-fill -> accumulate = 1"""
    L = vkn._lib.lib()
    M, Nout = dy.shape
    K = A.shape[1]
    dyw, Aw = torch.full((M, ldy), 7.0, device=DEV), torch.full((M, lda), -5.0, device=DEV)      # (the gaps hold values that would show)
    dyw[:, :Nout], Aw[:, :K] = dy.to(DEV), A.to(DEV)
    dW, db = Guard(Nout, K), Guard(1, Nout)
    if old is not None:
        dW.v.copy_(old[0].to(DEV))
        db.v[0].copy_(old[1].to(DEV))
    assert L.vkn_linear_dw_f32(P(dyw), ldy, P(Aw), lda, dW.ptr(), db.ptr() if with_db else None, M, K, Nout, int(old is not None), stream()) == 0
    torch.cuda.synchronize()
    dW.check('dW')
    if with_db:
        db.check('db')
    elif old is None:
        db.check('db', written=False)
    else:
        assert torch.equal(db.v[0].cpu(), old[1]), 'db = NULL: the pre-filled db was touched'
    return dW.v, db.v[0]


@pytest.mark.parametrize('M,K,Nout', ec.DW_SHAPES, ids=lambda v: str(v))
def test_linear_dw_bit_for_bit_on_integer_operands(vkn, M, K, Nout):
    """strides (ldy > Nout, lda > K: the column slices `UpdatorCoreFn` passes), db NULL, accumulate on integer old values: equal to
    float64 bit for bit (exact-fp32 MFMA; premise: tests/test_exact_premise.py::test_dw_fp32_equals_integer_reference)"""
    dy, A, old_w, old_b, dW, db = ec.dw_case(M, K, Nout, 1500 + ec.DW_SHAPES.index((M, K, Nout)))
    same = lambda got, want: torch.equal(got.double().cpu(), want)      # noqa: E731
    for ldy, lda in ((Nout, K), (2 * Nout + 3, K + 5), (Nout + 1, 2 * K)):
        gw, gb = run_dw(vkn, dy, A, ldy, lda)
        assert same(gw, dW) and same(gb, db), (ldy, lda)
    gw, _ = run_dw(vkn, dy, A, Nout + 4, K + 4, with_db=False)
    assert same(gw, dW)
    gw, gb = run_dw(vkn, dy, A, Nout + 4, K + 4, old=(old_w, old_b))
    assert same(gw, old_w.double() + dW) and same(gb, old_b.double() + db), 'accumulate = 1: old value + gradient'
    gw, gb = run_dw(vkn, dy, A, Nout, K, with_db=False, old=(old_w, old_b))
    assert same(gw, old_w.double() + dW)


@pytest.mark.parametrize('M,K,Nout', ec.DW_SHAPES, ids=lambda v: str(v))
def test_linear_dw_float_operands_vs_fp64(vkn, M, K, Nout):
    g = gen(4000 + M + K)
    dy, A = torch.randn(M, Nout, generator=g) * 1e-2, torch.randn(M, K, generator=g)
    old = (torch.randn(Nout, K, generator=g), torch.randn(Nout, generator=g))
    dW, db = R.linear_dw(dy.double(), A.double())
    gw, gb = run_dw(vkn, dy, A, Nout + 4, K + 8)
    aw, ab = run_dw(vkn, dy, A, Nout + 4, K + 8, old=old)
    e = dict(dW=rel(gw.cpu(), dW), db=rel(gb.cpu(), db), dW_acc=rel(aw.cpu(), old[0].double() + dW), db_acc=rel(ab.cpu(), old[1].double() + db))
    record_margins(f'chain_blocks.dw[{M}x{K}x{Nout}]', e)
    assert max(e['dW'], e['dW_acc']) < LIM['dw'] and max(e['db'], e['db_acc']) < LIM['db'], e


def _dw_batch(vkn, nitems, integer, seed):
    lib = vkn._lib
    M = ec.DW_BATCH_M
    keep, items, outs, refs = [], [], [], []
    for j, (K, Nout) in enumerate(ec.dw_batch_shapes(nitems)):
        if integer:
            dy, A, _, _, dW, db = ec.dw_case(M, K, Nout, 1600 + j)
        else:
            g = gen(seed + j)
            dy, A = torch.randn(M, Nout, generator=g), torch.randn(M, K, generator=g)
            dW, db = R.linear_dw(dy.double(), A.double())
        ldy, lda = Nout + (j % 3), K + 2 * (j % 2)
        dyw, Aw = torch.full((M, ldy), 7.0, device=DEV), torch.full((M, lda), -5.0, device=DEV)
        dyw[:, :Nout], Aw[:, :K] = dy.to(DEV), A.to(DEV)
        gW, gb = Guard(Nout, K), Guard(1, Nout)
        with_db = j % 4 != 3
        keep += [dyw, Aw]
        items.append(lib.VknDwItem(dyw.data_ptr(), Aw.data_ptr(), gW.v.data_ptr(), gb.v.data_ptr() if with_db else None, ldy, lda, Nout, K))
        outs.append((gW, gb, with_db))
        refs.append((dW, db))
    arr = (lib.VknDwItem * nitems)(*items)
    assert lib.lib().vkn_linear_dw_batch_f32(arr, nitems, M, stream()) == 0
    torch.cuda.synchronize()
    for gW, gb, with_db in outs:
        gW.check('dW'), gb.check('db', written=with_db)
    return outs, refs


@pytest.mark.parametrize('nitems', ec.DW_BATCH_ITEMS)
def test_linear_dw_batch_bit_for_bit_and_deterministic(vkn, nitems):
    """the batch launch at 1, 3 and VKN_DW_MAX_ITEMS items (mixed shapes and strides, db NULL in every fourth): on integer operands
    equal to float64 bit for bit — hence to the single calls, which `test_linear_dw_bit_for_bit_on_integer_operands` pins the same way;
    on float operands two runs give the same bits, and float64 to the single form's tolerance"""
    assert max(ec.DW_BATCH_ITEMS) == vkn._lib.CONSTS['VKN_DW_MAX_ITEMS']
    outs, refs = _dw_batch(vkn, nitems, True, 0)
    for j, ((gW, gb, with_db), (dW, db)) in enumerate(zip(outs, refs)):
        assert torch.equal(gW.v.double().cpu(), dW), j
        assert not with_db or torch.equal(gb.v[0].double().cpu(), db), j
        K, Nout = ec.dw_batch_shapes(nitems)[j]
        if j < 7:          # the single form on the same operands: the same bits
            dy, A = ec.dw_case(ec.DW_BATCH_M, K, Nout, 1600 + j)[:2]
            sw, sb = run_dw(vkn, dy, A, Nout, K)
            assert torch.equal(sw, gW.v) and (not with_db or torch.equal(sb, gb.v[0])), j
    a, refs = _dw_batch(vkn, nitems, False, 4100)
    b, _ = _dw_batch(vkn, nitems, False, 4100)
    worst = 0.0
    for (aw, ab, with_db), (bw, bb, _), (dW, db) in zip(a, b, refs):
        assert torch.equal(aw.bits, bw.bits) and torch.equal(ab.bits, bb.bits), 'two runs differ'
        worst = max(worst, rel(aw.v.cpu(), dW), rel(ab.v[0].cpu(), db) if with_db else 0.0)
    record_margins(f'chain_blocks.dw_batch[{nitems}]', dict(worst=worst))
    assert worst < LIM['dw_batch']


def test_linear_dw_batch_refuses_too_many_items(vkn):
    lib = vkn._lib
    n = lib.CONSTS['VKN_DW_MAX_ITEMS'] + 1
    dy, A = torch.ones(4, 4, device=DEV), torch.ones(4, 4, device=DEV)
    gs = [Guard(4, 4) for _ in range(n)]
    arr = (lib.VknDwItem * n)(*[lib.VknDwItem(dy.data_ptr(), A.data_ptr(), g_.v.data_ptr(), None, 4, 4, 4, 4) for g_ in gs])
    assert lib.lib().vkn_linear_dw_batch_f32(arr, n, 4, stream()) == E(vkn, 'VKN_E_ARG')
    torch.cuda.synchronize()
    for g_ in gs:
        g_.check('dW', written=False)
