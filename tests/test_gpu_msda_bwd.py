"""GPU: the backward of the sampling core, `vkn_msda_sample_bwd_f32` (include/vkn_msda_train.h), and `MSDeformAttnPixelDecoder`'s
training path with `fused_backward=True`.

References, draws and premises are those of tests/msda_bwd_ref.py (tests/test_msda_bwd_refs.py proves them on the CPU): reference =
float64 autograd through the explicit-corner core, yardstick = torch's fp32 autograd through its `grid_sample` composition, bound per
tensor = `msda_ref.judge`: max-abs error <= max(8 x the yardstick's error, 4 fp32 ulps of the tensor's largest magnitude).  The ratios
err / bound go to the margins record (profiles/msda_bwd_margins.json holds a run's)."""
import contextlib
import ctypes
import functools

import pytest
import torch

import msda_bwd_ref as RB
import msda_ref as R
from abi_arena import SENT, Arena, frozen
from helpers import record_margins
from test_msda_bwd_refs import PER_ELEMENT
from test_msdeform_decoder import BASE

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
STATUS_RANGE = 1
ONE_PIXEL = ((1, 1),)


def _cuda(*ts):
    return [t.to(DEV).contiguous() for t in ts]


@functools.lru_cache(maxsize=None)
def _core_case(name):
    """(operands, float64 gradients, fp32 yardstick gradients) of a per-element case: computed once, never modified"""
    case = R.CORE_CASES[name]
    ops = RB.draw_core_bwd(case, 5100 + list(R.CORE_CASES).index(name))
    want = RB.reference(case, *ops)
    RB.premises(name, case, ops[1], ops[3], want)
    return ops, want, RB.yardstick(case, *ops)


def _bwd(vkn, shapes, value, off, logits, ref, dout, M, P, grad_rows=None):
    """the binding on the layouts of the ABI -> (dvalue [B, S, M, D], doff like off, dlogits like logits)"""
    B, Q = off.shape[0], off.shape[1]
    dv, do, dl = vkn.ops.msda_sample_bwd(value.flatten(2), shapes, off.reshape(B * Q, -1), logits.reshape(B * Q, -1), ref, dout, M, P,
                                         grad_rows=grad_rows)
    return dv.view_as(value), do.reshape(off.shape), dl.reshape(logits.shape)


def _judge_all(label, got, want, yard):
    vals = {}
    for k, g, w, y in zip(('dvalue', 'doff', 'dlogits'), got, want, yard):
        err, bound, ratio, yard_err = R.judge(g, w, y)
        vals.update({f'{k}_err': err, f'{k}_bound': bound, f'{k}_ratio': ratio, f'{k}_torch_fp32_err': yard_err})
    record_margins(label, vals)
    for k, g in zip(('dvalue', 'doff', 'dlogits'), got):
        assert torch.isfinite(g).all() and vals[f'{k}_err'] <= vals[f'{k}_bound'], (label, k, vals)


@pytest.mark.parametrize('name', PER_ELEMENT)
def test_core_backward_per_element(vkn, name):
    case = R.CORE_CASES[name]
    ops, want, yard = _core_case(name)
    g = _cuda(*ops)
    with frozen(*g):
        got = _bwd(vkn, case.shapes, *g, case.M, case.P)
    vkn.ops.workspace_status(DEV)                                                # clean operands: no range flag
    _judge_all(f'msda_bwd_core[{name}]', got, want, yard)
    if len(case.shapes) * case.P == 1:
        assert not bool(got[2].any())                                            # L P = 1: exactly zero


@pytest.mark.parametrize('name', list(R.EXACT_CASES))
def test_core_backward_bit_for_bit(vkn, name):
    """integer values and dout, power-of-two levels, quarter-pixel offsets, equal logits: every product and sum is exact in fp32 in any
    order, and the fixed-point scatter is exact as well"""
    case = R.EXACT_CASES[name]
    ops = RB.draw_exact_bwd(case, 5200 + list(R.EXACT_CASES).index(name))
    want = RB.exact_premise_bwd(name, case, *ops)
    got = _bwd(vkn, case.shapes, *_cuda(*ops), case.M, case.P)
    for k, g, w in zip(('dvalue', 'doff', 'dlogits'), got, want):
        assert torch.equal(g.cpu().double(), w), (name, k, float((g.cpu().double() - w).abs().max()))


def test_headroom_at_its_limit(vkn):
    """every contribution the largest possible, |c| = max |dout|, and all Q P of them on ONE cell: the sum is Q max |dout| exactly"""
    B, M, D, Q = 1, 8, 16, 4096
    value = torch.randn(B, 1, M, D)
    off, logits = torch.zeros(B, Q, M, 1, 1, 2), torch.zeros(B, Q, M, 1)
    ref = torch.full((Q, 1, 2), 0.5)
    dout = torch.full((B, Q, M * D), 3.0)
    dv, do, dl = _bwd(vkn, ONE_PIXEL, *_cuda(value, off, logits, ref, dout), M, 1)
    vkn.ops.workspace_status(DEV)
    assert torch.equal(dv, torch.full_like(dv, 4096 * 3.0))
    assert not bool(dl.any()) and torch.isfinite(do).all()                       # one point: dlogits is exactly zero


def test_determinism_where_arrival_order_would_show(vkn):
    """32 768 contributions per cell of a one-pixel level: a float-atomic sum would differ from run to run in its last bits"""
    case = R.CoreCase(1, 4096, 8, 32, 8, ONE_PIXEL, 2.0)
    gen = torch.Generator().manual_seed(5300)
    value = torch.randn((1, 1, case.M, case.D), generator=gen)
    logits = (torch.rand((1, case.Q, case.M, case.P), generator=gen) * 2 - 1) * case.spread
    ref = torch.full((case.Q, 1, 2), 0.5)
    off = RB.nudge(case.shapes, (torch.rand((1, case.Q, case.M, 1, case.P, 2), generator=gen) * 2 - 1) * 0.9, ref)    # x = off.x in (-1, 1): in range
    dout = torch.randn((1, case.Q, case.M * case.D), generator=gen)
    ops = (value, off, logits, ref, dout)
    assert float(RB.integer_distance(case.shapes, off, ref).min()) >= RB.NEAR and R.band_shares(case.shapes, off, ref)['fail'] == 0.0
    g = _cuda(*ops)
    first = _bwd(vkn, case.shapes, *g, case.M, case.P)
    second = _bwd(vkn, case.shapes, *g, case.M, case.P)
    vkn.ops.workspace_status(DEV)
    for a, b in zip(first, second):
        assert torch.equal(a, b)
    _judge_all('msda_bwd_core[one cell, 32768 terms]', first, RB.reference(case, *ops), RB.yardstick(case, *ops))


# ---------------------------------------------------------------------------------------------------------------- raw ABI
class _Raw:
    """the entry through ctypes, outputs and workspace carved from an arena"""

    def __init__(self, vkn, case, ops):
        self.L, self.case = vkn._lib.lib(), case
        self.g = _cuda(*ops)
        B, Q, M, D, P, nl = case.B, case.Q, case.M, case.D, case.P, len(case.shapes)
        self.mlp = M * nl * P
        self.shapes = (ctypes.c_int * (2 * nl))(*[v for hw in case.shapes for v in hw])
        self.nb = self.L.vkn_msda_bwd_workspace_bytes(self.shapes, B, Q, M, D, nl, P)
        assert self.nb > 0
        self.A = Arena(DEV)
        self.sets = []

    def outputs(self, tag):
        c = self.case
        S = sum(h * w for h, w in c.shapes)
        o = dict(dvalue=self.A.out((c.B, S, c.M, c.D), name=f'dvalue{tag}'), doff=self.A.out((c.B * c.Q, 2 * self.mlp), name=f'doff{tag}'),
                 dlogits=self.A.out((c.B * c.Q, self.mlp), name=f'dlogits{tag}'), ws=self.A.ws(self.nb, name=f'ws{tag}'))
        self.sets.append(o)
        return o

    def call(self, o, off=None, dout=None, doff=None, dlogits=None, ld_doff=None, ld_dlogits=None):
        c, p = self.case, lambda t: ctypes.c_void_p(t.data_ptr())               # noqa: E731
        value, off0, logits, ref, dout0 = self.g
        o['ws'].bytes[:256].zero_()                                              # the caller's part: a clear status header
        with torch.cuda.device(DEV):
            return self.L.vkn_msda_sample_bwd_f32(
                p(value), p(off0 if off is None else off), 2 * self.mlp, p(logits), self.mlp, p(ref), self.shapes, p(dout0 if dout is None else dout),
                o['dvalue'].ptr, doff or o['doff'].ptr, ld_doff or 2 * self.mlp, dlogits or o['dlogits'].ptr, ld_dlogits or self.mlp,
                c.B, c.Q, c.M, c.D, len(c.shapes), c.P, o['ws'].ptr, self.nb, None)

    @staticmethod
    def status(o):
        torch.cuda.synchronize()
        return int(o['ws'].bytes[:4].view(torch.int32)[0])


def test_poisoned_offsets_write_nothing_outside_and_change_nothing_else(vkn):
    """NaN / +inf / -inf / +-1e30 in the offsets of points that the clean draw already places OUT: the guards around the three outputs
    and the workspace stay intact, the poisoned points' doff is exactly 0 and every output is bit-identical to the clean run"""
    name = 'shipped-89'
    case = R.CORE_CASES[name]
    (value, off, logits, ref, dout), want, yard = _core_case(name)
    x, y = R.pixel_coords(case.shapes, off.double(), ref.double())
    W = torch.tensor([w for _, w in case.shapes], dtype=torch.float64).view(1, 1, 1, -1, 1)
    far_out = ((x < -1.1) | (x > W + 0.1)).nonzero().tolist()                      # OUT in x by a margin no rounding crosses
    spots, seen = [], set()
    for b, q, m, l, p in far_out:
        if (b, q, m) not in seen and (b, q) not in {(s[0], s[1]) for s in spots}:
            seen.add((b, q, m))
            spots.append((b, q, m, l, p))
        if len(spots) == 6:
            break
    assert len(spots) == 6
    bad = off.clone()
    for (b, q, m, l, p), (axis, v) in zip(spots, ((0, float('nan')), (1, float('inf')), (0, float('-inf')), (1, 1e30), (0, -1e30), (1, float('nan')))):
        bad[b, q, m, l, p, axis] = v
    raw = _Raw(vkn, case, (value, off, logits, ref, dout))
    clean, dirty = raw.outputs('_clean'), raw.outputs('_dirty')
    with frozen(*raw.g):
        assert raw.call(clean) == 0 and raw.status(clean) == 0
        assert raw.call(dirty, off=bad.to(DEV)) == 0 and raw.status(dirty) == 0    # a point that fails the test is no range error
    raw.A.check('msda_sample_bwd')
    for k in ('dvalue', 'doff', 'dlogits'):
        assert torch.equal(clean[k].t, dirty[k].t), k
    doff = dirty['doff'].t.view(off.shape).cpu()
    for b, q, m, l, p in spots:
        assert not bool(doff[b, q, m, l, p].any())
    got = (clean['dvalue'].t, clean['doff'].t.view(off.shape), clean['dlogits'].t.view(logits.shape))
    for g, w, yd in zip(got, want, yard):
        err, bound, _, _ = R.judge(g, w, yd)
        assert err <= bound


def test_status_word(vkn):
    name = 'q5-of-89'
    case = R.CORE_CASES[name]
    ops, _, _ = _core_case(name)
    raw = _Raw(vkn, case, ops)
    a, b, c = raw.outputs('_a'), raw.outputs('_b'), raw.outputs('_c')
    nan_dout = ops[4].clone()
    nan_dout[1, 3, 17] = float('nan')
    nan_logit = ops[2].clone()
    nan_logit[0, 2, 5, 1] = float('nan')
    assert raw.call(a) == 0 and raw.status(a) == 0                                 # a clean call leaves the word 0
    assert raw.call(b, dout=nan_dout.to(DEV)) == 0 and raw.status(b) & STATUS_RANGE
    raw.g[2] = nan_logit.to(DEV)                                                   # a NaN logit: a non-finite contribution, never converted
    assert raw.call(c) == 0 and raw.status(c) & STATUS_RANGE
    raw.A.check('msda_sample_bwd status')
    # through the binding: `workspace_status` raises once and is clear afterwards
    g = _cuda(*ops)
    vkn.ops.workspace_status(DEV)
    _bwd(vkn, case.shapes, g[0], g[1], g[2], g[3], nan_dout.to(DEV), case.M, case.P)
    with pytest.raises(vkn.VknError):
        vkn.ops.workspace_status(DEV)
    vkn.ops.workspace_status(DEV)


def test_strides_both_gradients_in_one_buffer(vkn):
    """doff | dlogits written into ONE [B Q][3 M L P] buffer equal the separately written ones bit for bit; a guard column behind the
    rows proves nothing else is touched"""
    name = 'l4-p8'
    case = R.CORE_CASES[name]
    ops, _, _ = _core_case(name)
    raw = _Raw(vkn, case, ops)
    sep, joint = raw.outputs('_sep'), raw.outputs('_joint')
    rows, mlp, guard = case.B * case.Q, raw.mlp, 4
    both = torch.full((rows, 3 * mlp + guard), SENT, dtype=torch.int32, device=DEV)
    assert raw.call(sep) == 0
    assert raw.call(joint, doff=ctypes.c_void_p(both.data_ptr()), dlogits=ctypes.c_void_p(both.data_ptr() + 8 * mlp), ld_doff=3 * mlp + guard,
                    ld_dlogits=3 * mlp + guard) == 0
    torch.cuda.synchronize()
    assert bool((both[:, 3 * mlp:] == SENT).all()) and not bool((both[:, :3 * mlp] == SENT).any())
    assert torch.equal(both[:, :2 * mlp].view(torch.float32), sep['doff'].t) and torch.equal(both[:, 2 * mlp:3 * mlp].view(torch.float32), sep['dlogits'].t)
    assert torch.equal(joint['dvalue'].t, sep['dvalue'].t)
    assert bool((joint['doff'].bytes.view(torch.int32) == SENT).all()) and bool((joint['dlogits'].bytes.view(torch.int32) == SENT).all())
    # the binding's `grad_rows`: the same bits
    g = _cuda(*ops)
    rows_buf = torch.empty((rows, 3 * mlp), dtype=torch.float32, device=DEV)
    dv, do, dl = _bwd(vkn, case.shapes, *g, case.M, case.P, grad_rows=rows_buf)
    assert do.data_ptr() == rows_buf.data_ptr() and dl.data_ptr() == rows_buf.data_ptr() + 8 * mlp
    assert torch.equal(rows_buf[:, :2 * mlp], sep['doff'].t) and torch.equal(rows_buf[:, 2 * mlp:], sep['dlogits'].t) and torch.equal(dv.flatten(), sep['dvalue'].t.flatten())


# ---------------------------------------------------------------------------------------------------------------- the module
@contextlib.contextmanager
def _torch_deterministic():
    """torch's own ops around the core (the convs above all) repeat their bits from run to run only in torch's deterministic mode: on an
    MI355X even the module's FORWARD output differs between two runs without it, flag on or off.  In that mode the whole backward is
    reproducible with the flag on; with it off, `grid_sample`'s backward still is not (torch says so itself)."""
    before = (torch.are_deterministic_algorithms_enabled(), torch.is_deterministic_algorithms_warn_only_enabled())
    torch.use_deterministic_algorithms(True, warn_only=True)
    try:
        yield
    finally:
        torch.use_deterministic_algorithms(before[0], warn_only=before[1])


def _set_flag(neck, on):
    neck.fused_backward = on
    for layer in neck.encoder.layers:
        layer.attentions[0].fused_backward = on


def _grads(neck, feats, weights):
    ins = [f.detach().clone().requires_grad_(True) for f in feats]
    params = [p for _, p in neck.named_parameters()]
    outs = neck(ins)
    loss = sum((o * w).sum() for o, w in zip(outs, weights))
    g = torch.autograd.grad(loss, params + ins)
    return outs, dict(zip([k for k, _ in neck.named_parameters()], g[:len(params)])), list(g[len(params):])


def _nodes(outs):
    seen, stack = set(), [o.grad_fn for o in outs]
    while stack:
        fn = stack.pop()
        if fn is None or fn in seen:
            continue
        seen.add(fn)
        stack += [f for f, _ in fn.next_functions]
    return [type(fn).__name__ for fn in seen]


@pytest.fixture(scope='module')
def necks(vkn):
    """per module case: (the module on the GPU with the flag on, inputs, loss weights, float64 gradients) — computed once"""
    made = {}
    for name, case in R.MODULE_CASES.items():
        torch.manual_seed(31)
        neck = vkn.build_neck(dict(R.module_cfg(case, BASE), fused_backward=True))
        neck.init_weights()
        R.randomise(neck, 32)
        feats = R.module_inputs(case, 33)
        with torch.no_grad():
            shapes = [tuple(o.shape) for o in neck(feats)]
        gen = torch.Generator().manual_seed(34)
        weights = [torch.randn(s, generator=gen) for s in shapes]
        want_p, want_x = RB.decoder_grads_f64(neck.state_dict(), feats, weights, case['num_heads'])
        made[name] = (neck.to(DEV), [f.to(DEV) for f in feats], [w.to(DEV) for w in weights], want_p, want_x)
    return made


@pytest.mark.parametrize('name', list(R.MODULE_CASES))
def test_module_fused_backward(vkn, necks, name):
    neck, feats, weights, want_p, want_x = necks[name]
    case = R.MODULE_CASES[name]
    _set_flag(neck, True)
    with _torch_deterministic():
        outs, gp, gx = _grads(neck, feats, weights)
        assert _nodes(outs).count('MSDASampleFnBackward') == case['num_layers']
        _, gp2, gx2 = _grads(neck, feats, weights)
    assert all(torch.equal(gp[k], gp2[k]) for k in gp) and all(torch.equal(a, b) for a, b in zip(gx, gx2))      # two backward passes: the same bits
    vkn.ops.workspace_status(DEV)
    _set_flag(neck, False)
    try:
        outs_t, yp, yx = _grads(neck, feats, weights)
        assert 'MSDASampleFnBackward' not in _nodes(outs_t)                      # flag off: torch's composition, as before
    finally:
        _set_flag(neck, True)
    assert set(gp) == set(want_p) and all(want_p[k] is not None for k in gp)
    vals, worst = {}, ('', 0.0)
    for k, g, w, y in [(k, gp[k], want_p[k], yp[k]) for k in gp] + [(f'input{i}', gx[i], want_x[i], yx[i]) for i in range(len(gx))]:
        err, bound, ratio, yard_err = R.judge(g, w, y)
        vals[k] = (err, bound, ratio, yard_err)
        worst = max(worst, (k, ratio), key=lambda t: t[1])
    record_margins(f'msda_bwd_module[{name}]', dict(tensors=len(vals), worst_ratio=worst[1], worst_tensor=worst[0],
                                                     worst_err=vals[worst[0]][0], worst_bound=vals[worst[0]][1]))
    for k, (err, bound, ratio, _) in vals.items():
        assert err <= bound, (name, k, err, bound)


def test_module_graph_capture_and_replay(vkn, necks):
    """one torch.cuda.graph capture of forward + backward, replayed: the eager gradients bit for bit"""
    neck, feats, weights, _, _ = necks['narrow']
    _set_flag(neck, True)
    with _torch_deterministic():
        _, gp, gx = _grads(neck, feats, weights)
        side = torch.cuda.Stream()
        side.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(side):
            for _ in range(2):
                _grads(neck, feats, weights)
        torch.cuda.current_stream().wait_stream(side)
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            _, cp, cx = _grads(neck, feats, weights)
        for t in list(cp.values()) + cx:
            t.zero_()
        graph.replay()
        torch.cuda.synchronize()
    assert all(torch.equal(gp[k], cp[k]) for k in gp) and all(torch.equal(a, b) for a, b in zip(gx, cx))
