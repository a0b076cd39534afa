"""GPU: the sampling core `vkn_msda_sample_f32` (include/vkn_msda.h) and `MSDeformAttnPixelDecoder`'s fused forward.

References, bound and cases are those of tests/msda_ref.py (tests/test_msda_refs.py proves their premises on the CPU).  Per tensor:
max-abs error against float64 <= max(8 x the error of torch's fp32 composition against that float64, 4 fp32 ulps of the tensor's
largest magnitude).  The ratios err / bound go to the margins record (profiles/msda_margins.json holds a run's).

Measured on an MI355X (that file): the largest ratio err / bound is 0.129 for the core (the shipped point on the 2x3 / 4x5 / 7x9
levels) and 0.129 for the module (the 4 x 6 level at 64 channels; 0.122 at the shipped width, 0.131 in another run of it); every ratio
lies between 0.07 and 0.13, that is the kernel's error equals torch's own fp32 error: both are dominated by the rounding of
loc = ref + off / W, which the two compute alike.
"""
import ctypes

import pytest
import torch

import msda_ref as R
from abi_arena import Arena, frozen
from helpers import record_margins
from test_msdeform_decoder import BASE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_SHAPE, E_ALIGN = -2, -5


def _cuda(*ts):
    return [t.to(DEV).contiguous() for t in ts]


def _run(vkn, case_shapes, value, off, logits, ref, M, P):
    """the wrapper on the layouts of the ABI: offsets and logits as the column ranges of ONE [B Q][3 M L P] buffer, as the module has them"""
    B, Q = off.shape[0], off.shape[1]
    both = torch.cat([off.reshape(B * Q, -1), logits.reshape(B * Q, -1)], 1).contiguous()
    n_off = off[0, 0].numel()
    return vkn.ops.msda_sample(value.flatten(2), case_shapes, both[:, :n_off], both[:, n_off:], ref, M, P)


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_core_per_element(vkn, name):
    case = R.CORE_CASES[name]
    value, off, logits, ref = R.draw_core(case, 4100 + list(R.CORE_CASES).index(name))
    want = R.core_f64(value, case.shapes, off, logits, ref)
    yard = R.core_grid_sample(value, case.shapes, off, logits, ref, torch.float32)
    g = _cuda(value, off, logits, ref)
    with frozen(*g):
        got = _run(vkn, case.shapes, *g, case.M, case.P)
        plain = vkn.ops.msda_sample(g[0].flatten(2), case.shapes, g[1].flatten(2).flatten(0, 1), g[2].flatten(2).flatten(0, 1), g[3], case.M, case.P)
    assert got.shape == want.shape and torch.equal(got, plain)                    # the row strides change nothing
    err, bound, ratio, yard_err = R.judge(got, want, yard)
    record_margins(f'msda_core[{name}]', dict(err=err, bound=bound, ratio=ratio, torch_fp32_err=yard_err))
    assert torch.isfinite(got).all() and err <= bound, (name, err, bound)


@pytest.mark.parametrize('name', list(R.EXACT_CASES))
def test_core_bit_for_bit(vkn, name):
    """integer values, power-of-two levels, quarter-pixel offsets, equal logits: every product and sum is exact in fp32, in any order"""
    case = R.EXACT_CASES[name]
    value, off, logits, ref = R.draw_exact(case, 4200 + list(R.EXACT_CASES).index(name))
    want = R.exact_premise(case, value, off, logits, ref)
    got = _run(vkn, case.shapes, *_cuda(value, off, logits, ref), case.M, case.P)
    assert torch.equal(got.cpu().double(), want), (name, float((got.cpu().double() - want).abs().max()))


def test_core_safety_and_determinism(vkn):
    """NaN, +-inf and +-1e30 offsets at a few points leave every other (b, q, m) bit-identical, the poisoned points read nothing and add
    nothing (the poisoned heads equal the float64 reference with those points dropped), and two runs are bitwise equal"""
    case = R.CORE_CASES['shipped-89']
    value, off, logits, ref = R.draw_core(case, 4100)
    spots = [(0, 0, 0, 0, 0, 0), (0, 17, 3, 1, 2, 1), (1, 88, 7, 2, 3, 0), (1, 40, 5, 0, 1, 1), (0, 60, 2, 2, 0, 0), (1, 5, 1, 1, 1, 0)]
    for spot in spots:
        off[spot[:-1]] = 0.0                                                      # clean: the point sits on its reference point, inside
    bad = off.clone()
    for spot, v in zip(spots, (float('nan'), float('inf'), float('-inf'), 1e30, -1e30, float('nan'))):
        bad[spot] = v
    hit = torch.zeros(case.B, case.Q, case.M, dtype=torch.bool)
    for b, q, m, *_ in spots:
        hit[b, q, m] = True
    g = _cuda(value, off, logits, ref)
    clean = _run(vkn, case.shapes, *g, case.M, case.P)
    dirty = _run(vkn, case.shapes, g[0], bad.to(DEV), g[2], g[3], case.M, case.P)
    again = _run(vkn, case.shapes, g[0], bad.to(DEV), g[2], g[3], case.M, case.P)
    torch.cuda.synchronize()
    assert torch.isfinite(dirty).all() and torch.equal(dirty, again)
    c, d = clean.view(case.B, case.Q, case.M, case.D).cpu(), dirty.view(case.B, case.Q, case.M, case.D).cpu()
    assert torch.equal(c[~hit], d[~hit]) and int(hit.sum()) == len(spots)
    # a poisoned point is a point outside: the reference with the offset moved far out (finite) gives the poisoned heads
    far = torch.where(torch.isfinite(bad) & (bad.abs() < 1e29), bad, torch.full_like(bad, 1e6))
    want = R.core_f64(value, case.shapes, far, logits, ref).view(case.B, case.Q, case.M, case.D)
    yard = R.core_grid_sample(value, case.shapes, far, logits, ref, torch.float32).view(case.B, case.Q, case.M, case.D)
    err, bound, ratio, _ = R.judge(d[hit], want[hit], yard[hit])
    record_margins('msda_core[poisoned heads]', dict(err=err, bound=bound, ratio=ratio))
    assert err <= bound and float((want[hit] - R.core_f64(value, case.shapes, off, logits, ref).view_as(want)[hit]).abs().max()) > 1e-3


def test_core_buffer_contract(vkn):
    """raw ctypes out of an arena: the output at its exact size between sentinel guards, inputs unchanged, a misaligned pointer and a
    shape outside the envelope refused with nothing written, two runs bitwise equal"""
    L = vkn._lib.lib()
    case = R.CORE_CASES['shipped-89']
    value, off, logits, ref = _cuda(*R.draw_core(case, 4100))
    B, Q, M, D, P, nl = case.B, case.Q, case.M, case.D, case.P, len(case.shapes)
    shapes = (ctypes.c_int * (2 * nl))(*[v for hw in case.shapes for v in hw])
    A = Arena(DEV)
    out, out2 = A.out((B, Q, M * D), name='out'), A.out((B, Q, M * D), name='out2')
    refused = A.out((B, Q, M * D), name='refused', full=False)
    p = lambda t: ctypes.c_void_p(t.data_ptr())                                # noqa: E731

    def call(o, d=D, value_ptr=None):
        return L.vkn_msda_sample_f32(value_ptr or p(value), p(off), 2 * M * nl * P, p(logits), M * nl * P, p(ref), shapes, o, B, Q, M, d, nl, P, None)
    with torch.cuda.device(DEV), frozen(value, off, logits, ref):
        assert call(out.ptr) == 0 and call(out2.ptr) == 0
        assert call(ctypes.c_void_p(refused.addr + 4)) == E_ALIGN and call(refused.ptr, value_ptr=ctypes.c_void_p(value.data_ptr() + 8)) == E_ALIGN
        assert call(refused.ptr, d=24) == E_SHAPE
    A.check('msda_sample')
    assert torch.equal(out.t, out2.t)
    assert bool((refused.bytes.view(torch.int32) == 0x7FC0BEEF).all())          # the refusals wrote nothing
    want = R.core_f64(value.cpu(), case.shapes, off.cpu(), logits.cpu(), ref.cpu())
    yard = R.core_grid_sample(value.cpu(), case.shapes, off.cpu(), logits.cpu(), ref.cpu(), torch.float32)
    err, bound, ratio, _ = R.judge(out.t, want, yard)
    assert err <= bound


# ---------------------------------------------------------------------------------------------------------------- the module
class _Counter:
    def __init__(self, ops):
        self.ops, self.fn, self.calls = ops, ops.msda_sample, 0

    def __enter__(self):
        def counted(*a, **k):
            self.calls += 1
            return self.fn(*a, **k)
        self.ops.msda_sample = counted
        return self

    def __exit__(self, *exc):
        self.ops.msda_sample = self.fn


@pytest.fixture(scope='module')
def necks(vkn):
    """per module case: (the module on the GPU in eval mode, inputs on the CPU, the float64 decoder's outputs) — computed once"""
    made = {}
    for name, case in R.MODULE_CASES.items():
        torch.manual_seed(11)
        neck = vkn.build_neck(R.module_cfg(case, BASE))
        neck.init_weights()
        R.randomise(neck, 12)
        neck.eval()
        feats = R.module_inputs(case, 13)
        want = R.decoder_f64(neck.state_dict(), feats, num_heads=case['num_heads'])
        made[name] = (neck.to(DEV), feats, want)
    return made


@pytest.mark.parametrize('name', list(R.MODULE_CASES))
def test_module_fused_forward(vkn, necks, name):
    neck, feats, want = necks[name]
    case = R.MODULE_CASES[name]
    ins = [f.to(DEV) for f in feats]
    with torch.no_grad(), _Counter(vkn.ops) as n:
        assert neck.fused_ok(ins)
        got = neck(ins)
        assert n.calls == case['num_layers']                                     # torch.no_grad(): the kernel, once per layer
        yard = neck.forward_torch(ins)
        assert n.calls == case['num_layers']
    assert isinstance(got, tuple) and [tuple(g.shape) for g in got] == [tuple(w.shape) for w in want]
    vals = {}
    for i, (g, y, w) in enumerate(zip(got, yard, want)):
        err, bound, ratio, yard_err = R.judge(g, w, y)
        vals.update({f'out{i}_err': err, f'out{i}_bound': bound, f'out{i}_ratio': ratio, f'out{i}_torch_fp32_err': yard_err})
    record_margins(f'msda_module[{name}]', vals)
    for i in range(len(got)):
        assert vals[f'out{i}_err'] <= vals[f'out{i}_bound'], (name, i, vals)


def test_module_path_choices(vkn, necks):
    neck, feats, _ = necks['narrow']
    ins = [f.to(DEV) for f in feats]
    with _Counter(vkn.ops) as n:
        out = neck(ins)                                                          # grad enabled, parameters require it: forward_torch
        assert n.calls == 0 and all(o.requires_grad for o in out)
        with torch.no_grad():
            neck(ins)
            assert n.calls == 2
            # outside the envelope: D = 64 / 8 heads = 8 channels per head, and nine points
            for edit in (dict(num_heads=8), dict(num_points=9)):
                cfg = R.module_cfg(R.MODULE_CASES['narrow'], BASE)
                cfg['encoder']['transformerlayers']['attn_cfgs'].update(edit)
                other = vkn.build_neck(cfg).to(DEV).eval()
                assert not other.fused_ok(ins)
                res = other(ins)
                assert n.calls == 2 and all(torch.isfinite(r).all() for r in res)
            # fused=False keeps a module on the torch composition
            cfg = R.module_cfg(R.MODULE_CASES['narrow'], BASE)
            off = vkn.build_neck(dict(cfg, fused=False)).to(DEV).eval()
            off(ins)
            assert n.calls == 2
        # a changed weight is seen: the prepared images are rebuilt
        with torch.no_grad():
            weight = neck.encoder.layers[0].attentions[0].value_proj.weight
            before, saved = neck(ins), weight.clone()
            weight.mul_(1.5)
            after = neck(ins)
            weight.copy_(saved)
            assert n.calls == 6 and float((before[1] - after[1]).abs().max()) > 1e-3
