"""GPU: the HIP backward of the Swin window-attention core (include/vkn_wattn_train.h, csrc/vkn_swin_bwd.hip), its autograd function and the
modules that take it with `fused='train'` (video-k-net_amd/swin.py), against float64 autograd of the restatement tests/swin_ref.py
(premises: tests/test_swin_refs.py, tests/test_swin_bwd_refs.py).

The accuracy bound is the project's, `swin_ref.bound`, per gradient tensor: max-abs error against float64 autograd on the CPU <= max(8 x the
error of the SAME composition run in fp32 on the device with torch autograd, 4 fp32 ulps of that gradient's largest magnitude).  The bound
is measured on the torch arm, never on the kernel.  `dout` is a seeded randn.  The ratios err / limit go to `helpers.record_margins` (one
run: profiles/swin_bwd_margins.json).

The addressing test catches a wrong token, window or mask outright: on the single-offset selector cases with dout zeroed on undecided and
pad-won queries every softmax is exactly one-hot in fp32, so the v third of dqkv is a pure scatter of dout rows, bit for bit."""
import ctypes

import pytest
import torch

import swin_bwd_ref as G
import swin_ref as R
from abi_arena import Arena, frozen
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
_REFS = {}


def _ref(name):
    """a core case, its dout, float64 autograd of the restatement, and the fp32 torch arm on the device: computed once, shared, never modified"""
    if name not in _REFS:
        case = R.core_case(name)
        dout = G.seeded_dout(case)
        _REFS[name] = case, dout, G.autograd_grads(case, dout, torch.float64, 'cpu'), G.autograd_grads(case, dout, torch.float32, DEV)
    return _REFS[name]


def _run(vkn, case, dout):
    dev = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    out = vkn.ops.swin_window_attention_bwd(dev(case['qkv']), dev(case['qkv_bias']), dev(case['table']), dev(dout), case['H'], case['W'], case['heads'],
                                            case['window'], case['shift'], case['scale'])
    torch.cuda.synchronize()
    return out


def _judge(test_id, got, want64, own):
    """got: the kernel arm; own: the fp32 torch arm (both anywhere, any float dtype); want64: float64 on the CPU"""
    want64 = want64.reshape(got.shape)
    err = (got.detach().double().cpu() - want64).abs().max().item()
    ref_err = (own.detach().double().cpu().reshape(got.shape) - want64).abs().max().item()
    limit, ratio = R.bound(err, ref_err, want64.abs().max().item())
    record_margins(test_id, dict(err=err, torch_fp32_err=ref_err, limit=limit, ratio=ratio))
    assert err <= limit, f'{test_id}: error {err:.3e} over the limit {limit:.3e} (torch fp32 {ref_err:.3e})'


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_core_per_element(vkn, name):
    case, dout, want, own = _ref(name)
    assert case['B'] * case['H'] * case['W'] <= 2 * 14 * 21
    dqkv, dbias, dtable = _run(vkn, case, dout)
    assert dqkv.shape == case['qkv'].shape and dtable.shape == case['table'].shape and all(bool(torch.isfinite(t).all()) for t in (dqkv, dtable))
    _judge(f'swin_bwd_core[{name}: dqkv]', dqkv, want['dqkv'], own['dqkv'])
    _judge(f'swin_bwd_core[{name}: dbias_table]', dtable, want['dtable'], own['dtable'])
    C = case['heads'] * R.HD
    rows = dqkv.double().reshape(-1, 3 * C).sum(0)                              # the real tokens' part: the qkv Linear's own backward
    if case['qkv_bias'] is None:
        assert dbias is None
        return
    assert dbias.shape == (3 * C,) and not bool(dbias[:C].any())                 # the q third: exactly zero
    _judge(f'swin_bwd_core[{name}: whole bias gradient]', dbias.double() + rows, want['dbias_total'], own['dbias_total'])
    pad64 = G.run_formulas(case, dout)['dbias_pad']                             # the pad part alone, against the written-out formulas
    if bool(pad64.any()):
        _judge(f'swin_bwd_core[{name}: pad part of the bias gradient]', dbias, pad64, own['dbias_pad'])
    else:
        assert not bool(dbias.any()), f'{name}: no pad token, yet a pad part'


@pytest.mark.parametrize('name', G.ADDRESSING_CASES)
def test_addressing_bit_for_bit(vkn, name):
    case, dout = G.addressing_case(name)
    want = G.autograd_grads(case, dout)['dqkv'][:, :, :, 2].float()             # zero or exactly one dout row each (tests/test_swin_bwd_refs.py)
    dqkv, _, _ = _run(vkn, case, dout)
    got = dqkv.view(case['B'], case['H'], case['W'], 3, case['heads'], R.HD)[:, :, :, 2].cpu()
    live = int((want.abs().amax(-1) > 0).sum())
    assert live == G.ADDRESSING_ROWS[name]
    wrong = got != want
    assert torch.equal(got, want), f'{name}: {int(wrong.sum())} elements of dv are not the scatter of dout, the first at {wrong.nonzero()[0].tolist()}'


def test_buffer_contract_and_gates(vkn):
    """the three outputs and the workspace of exactly their sizes between guards, on a padded shifted shape; the inputs are `const`; every
    refusal comes before a launch, in the stated order"""
    L = vkn._lib.lib()
    case, dout, want, own = _ref('pad_both_shift')
    B, H, W, heads, ws, shift = (case[k] for k in ('B', 'H', 'W', 'heads', 'window', 'shift'))
    qkv, bias, table, do = case['qkv'].to(DEV), case['qkv_bias'].to(DEV), case['table'].to(DEV), dout.to(DEV)
    assert all(t.data_ptr() % 16 == 0 for t in (qkv, bias, table, do))
    need = L.vkn_wattn_bwd_workspace_bytes(B, H, W, heads, ws)
    assert need == (4 * 6 * heads * 169 + 255) // 256 * 256 + 4 * 6 * heads * 64
    A = Arena(DEV)
    dqkv = A.out((B, H, W, 3, heads, R.HD), torch.float32, name='dqkv')
    dbias = A.out((3 * heads * R.HD,), torch.float32, name='dqkv_bias')
    dtable = A.out((169, heads), torch.float32, name='dbias_table')
    wsp = A.ws(need, name='workspace')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(qkv=qkv.data_ptr(), qkv_bias=bias.data_ptr(), table=table.data_ptr(), dout=do.data_ptr(), dqkv=dqkv.addr, dqkv_bias=dbias.addr,
                 dtable=dtable.addr, B=B, H=H, W=W, heads=heads, window=ws, shift=shift, ws=wsp.addr, ws_bytes=need)
        a.update(kw)
        p = lambda k: ctypes.c_void_p(a[k])                                     # noqa: E731
        return L.vkn_wattn_bwd_f32(p('qkv'), p('qkv_bias'), p('table'), p('dout'), p('dqkv'), p('dqkv_bias'), p('dtable'), a['B'], a['H'], a['W'],
                                   a['heads'], a['window'], a['shift'], case['scale'], p('ws'), a['ws_bytes'], stream)
    with torch.cuda.device(DEV), frozen(qkv=qkv, qkv_bias=bias, table=table, dout=do):
        # refused: nothing is written (the arena still holds its sentinel everywhere, the outputs included)
        for kw in (dict(qkv=None), dict(table=None), dict(dout=None), dict(dqkv=None), dict(dtable=None), dict(B=0), dict(H=0), dict(W=-1), dict(heads=0),
                   dict(qkv_bias=None), dict(dqkv_bias=None)):
            assert call(**kw) == E_ARG, kw
        for kw in (dict(heads=65), dict(window=0), dict(window=9), dict(shift=ws), dict(shift=-1), dict(window=3, shift=3), dict(B=1 << 20, H=64, W=64)):
            assert call(**kw) == E_SHAPE, kw
        assert call(ws_bytes=need - 1) == call(ws=None) == call(ws_bytes=0) == E_WORKSPACE
        for k, p in dict(qkv=qkv.data_ptr(), qkv_bias=bias.data_ptr(), table=table.data_ptr(), dout=do.data_ptr(), dqkv=dqkv.addr, dqkv_bias=dbias.addr,
                         dtable=dtable.addr, ws=wsp.addr).items():
            assert call(**{k: p + 4}) == call(**{k: p + 8}) == E_ALIGN, k
        # the order of the refusals
        assert call(qkv=None, heads=65) == call(dqkv_bias=None, shift=ws) == E_ARG and call(shift=ws, ws_bytes=0) == call(shift=ws, dqkv=dqkv.addr + 4) == E_SHAPE
        assert call(ws_bytes=need - 1, dqkv=dqkv.addr + 4) == E_WORKSPACE
        torch.cuda.synchronize()
        assert bool((A.words == 0x7FC0BEEF).all())
        assert call() == 0
        A.check('wattn_bwd_f32 on 10 x 17, window 7, shift 3')
    _judge('swin_bwd_arena[dqkv]', dqkv.t, want['dqkv'], own['dqkv'])
    _judge('swin_bwd_arena[dbias_table]', dtable.t, want['dtable'], own['dtable'])
    _judge('swin_bwd_arena[pad part of the bias gradient]', dbias.t, want['dbias_pad'], own['dbias_pad'])
    # without a bias: the same workspace size, dqkv_bias NULL
    A2 = Arena(DEV)
    dqkv2, dtable2, wsp2 = A2.out((B, H, W, 3, heads, R.HD), name='dqkv'), A2.out((169, heads), name='dbias_table'), A2.ws(need, name='workspace')
    with torch.cuda.device(DEV), frozen(qkv=qkv, table=table, dout=do):
        rc = L.vkn_wattn_bwd_f32(ctypes.c_void_p(qkv.data_ptr()), None, ctypes.c_void_p(table.data_ptr()), ctypes.c_void_p(do.data_ptr()), dqkv2.ptr, None,
                                 dtable2.ptr, B, H, W, heads, ws, shift, case['scale'], wsp2.ptr, need, stream)
        assert rc == 0
        A2.check('wattn_bwd_f32 without a bias')
    # the envelope query says what the entry says
    sup = vkn.ops.swin_window_attention_bwd_supported
    assert sup(B, H, W, heads, ws, shift) and sup(2, 200, 336, 4, 7, 3) and sup(1, 7, 7, 64, 8, 7)
    assert not sup(B, H, W, 65, ws, shift) and not sup(B, H, W, heads, 9, 0) and not sup(B, H, W, heads, ws, ws) and not sup(B, H, W, heads, ws, shift, head_dim=16)


@pytest.mark.parametrize('name', ('pad_both_shift', 'max_tokens'))
def test_two_runs_give_the_same_bits(vkn, name):
    case, dout, _, _ = _ref(name)
    a, b = _run(vkn, case, dout), _run(vkn, case, dout)
    assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_a_graph_replay_gives_the_same_bits(vkn):
    case, dout, _, _ = _ref('pad_both_shift')
    qkv, bias, table, do = case['qkv'].to(DEV), case['qkv_bias'].to(DEV), case['table'].to(DEV), dout.to(DEV)
    run = lambda: vkn.ops.swin_window_attention_bwd(qkv, bias, table, do, case['H'], case['W'], case['heads'], case['window'], case['shift'], case['scale'])      # noqa: E731
    first = run()
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                  # (the code objects are loaded and the workspace allocated before the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run()
    for t in cap:
        t.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert all(torch.equal(x, y) for x, y in zip(cap, first))


# ------------------------------------------------------------------------------------------------ modules
def _blocks(m):
    from video_k_net_amd import swin
    return [b for b in m.modules() if isinstance(b, swin.SwinTransformerBlock)]


def _arms(make, seed):
    """the same module twice in fp32 on the device, `fused='train'` and `fused=False`, and its state dict in float64 as leaves"""
    nets = []
    for fused in ('train', False):
        m = make(fused).eval()                                 # (eval: no stochastic depth; gradients flow all the same)
        m.load_state_dict(R.random_state(m, seed), strict=True)
        nets.append(m.to(DEV))
    sd64 = {k: (v.double().requires_grad_() if v.dtype.is_floating_point else v) for k, v in R.random_state(make(False), seed).items()}
    return nets[0], nets[1], sd64


def _functional(outs, seed):
    """a seeded linear functional of the outputs (the same weights for every arm)"""
    total = 0
    for i, o in enumerate(outs):
        w = torch.randn(o.shape, generator=torch.Generator().manual_seed(seed + i))
        total = total + (o * w.to(device=o.device, dtype=o.dtype)).sum()
    return total


def _judge_grads(tag, train, plain, sd64, x_grads):
    for k, p in train.named_parameters():
        assert p.grad is not None and sd64[k].grad is not None, k
        _judge(f'{tag}[{k}]', p.grad, sd64[k].grad, dict(plain.named_parameters())[k].grad)
    _judge(f'{tag}[input]', *x_grads)


def _layer_case(with_cp, seed):
    from video_k_net_amd import swin
    train, plain, sd = _arms(lambda f: swin.BasicLayer(dim=64, depth=2, num_heads=2, window_size=7, downsample=swin.PatchMerging, with_cp=with_cp, fused=f), seed)
    x = torch.randn((2, 10 * 17, 64), generator=torch.Generator().manual_seed(seed + 100))
    grads = []
    for m in (train, plain):
        xi = x.to(DEV).requires_grad_()
        out = m(xi, 10, 17)
        _functional((out[0], out[3]), 77).backward()
        grads.append(xi.grad)
    x64 = x.double().requires_grad_()
    want = R.layer(sd, '', x64, 10, 17, 2, 2, 7, True)
    _functional(want[:2], 77).backward()
    assert [b.last_path for b in _blocks(train)] == ['fused_train'] * 2 and [b.last_path for b in _blocks(plain)] == ['torch'] * 2
    return train, plain, sd, (grads[0], x64.grad, grads[1]), x


def test_basic_layer_gradients(vkn):
    train, plain, sd, xg, x = _layer_case(False, 41)
    _judge_grads('swin_bwd_layer', train, plain, sd, xg)
    # a second backward pass: the same bits where the kernel's sums land
    names = ('attn.qkv.weight', 'attn.qkv.bias', 'attn.relative_position_bias_table')
    first = {k: p.grad.clone() for k, p in train.named_parameters() if k.endswith(names)}
    assert len(first) == 6
    train.zero_grad(set_to_none=True)
    out = train(x.to(DEV).requires_grad_(), 10, 17)
    _functional((out[0], out[3]), 77).backward()
    assert all(torch.equal(p.grad, first[k]) for k, p in train.named_parameters() if k in first)


def test_basic_layer_gradients_with_checkpointing(vkn):
    train, plain, sd, xg, _ = _layer_case(True, 43)
    _judge_grads('swin_bwd_layer_cp', train, plain, sd, xg)


def test_whole_backbone_gradients(vkn):
    from video_k_net_amd import swin
    cfg = dict(embed_dims=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])
    train, plain, sd = _arms(lambda f: swin.SwinTransformerDIY(fused=f, **cfg), 45)
    img = torch.randn((2, 3, 61, 90), generator=torch.Generator().manual_seed(47))
    grads = []
    for m in (train, plain):
        xi = img.to(DEV).requires_grad_()
        _functional(m(xi), 79).backward()
        grads.append(xi.grad)
    x64 = img.double().requires_grad_()
    _functional(R.backbone(sd, x64, 32, cfg['depths'], cfg['num_heads']), 79).backward()
    assert [b.last_path for b in _blocks(train)] == ['fused_train'] * 8 and [b.last_path for b in _blocks(plain)] == ['torch'] * 8
    _judge_grads('swin_bwd_backbone', train, plain, sd, (grads[0], x64.grad, grads[1]))


def test_path_choice(vkn):
    from video_k_net_amd import swin
    mask = R.painted_mask(10, 17, 7, 3, torch.float32).to(DEV)
    x = torch.randn((1, 170, 64), device=DEV)

    def path(blk, grad=True):
        blk.H, blk.W = 10, 17
        for p in blk.parameters():
            p.requires_grad = grad
        out = blk(x, mask)
        assert out.requires_grad == grad
        return blk.last_path
    train = swin.SwinTransformerBlock(dim=64, num_heads=2, window_size=7, shift_size=3, fused='train').to(DEV).eval()
    assert path(train) == 'fused_train'
    assert path(train, grad=False) == 'fused'                                   # nothing requires a gradient: the forward kernel alone
    with torch.no_grad():
        for p in train.parameters():
            p.requires_grad = True
        train(x, mask)
        assert train.last_path == 'fused'
    assert path(train.train()) == 'fused_train'                                 # attn_drop = 0: training mode alone changes nothing
    odd = swin.SwinTransformerBlock(dim=64, num_heads=4, window_size=7, shift_size=3, fused='train').to(DEV).eval()      # head_dim 16
    assert path(odd) == 'torch'
    drop = swin.SwinTransformerBlock(dim=64, num_heads=2, window_size=7, shift_size=3, attn_drop=0.1, fused='train').to(DEV)
    assert path(drop.train()) == 'torch' and path(drop.eval()) == 'fused_train'
    plain = swin.SwinTransformerBlock(dim=64, num_heads=2, window_size=7, shift_size=3).to(DEV).eval()
    assert plain.fused is swin.FUSED_DEFAULT and path(plain) == 'torch'        # a default block with a gradient: the composition, as before
    with torch.autocast('cuda', dtype=torch.float16):
        assert path(train.eval()) == 'torch'
