"""GPU: the fused (shifted-)window attention of the Swin backbone (include/vkn_swin.h, csrc/vkn_swin.hip) and the modules on top of it
(video-k-net_amd/swin.py), against the float64 restatement of tests/swin_ref.py (its premises: tests/test_swin_refs.py).

The accuracy bound is the project's: max-abs error against float64 <= max(8 x the error of the torch composition in fp32 against that
float64, 4 fp32 ulps of the tensor's largest magnitude).  The bound is measured on the torch composition, never on the kernel.  For the
core cases, which start from the rows of the qkv Linear, the torch composition is the restatement itself run in fp32 on the device from the
same rows (tests/test_swin_refs.py pins it against `forward_torch` to 1e-12 in float64); for the module cases it is the module's own
`forward_torch` (fused=False) in fp32.  The ratios err / limit go to `helpers.record_margins` (one run: profiles/swin_margins.json).

The selector cases catch an addressing or mask error outright: q = 0 and a bias table of -400 but at one or two offsets make the softmax of
most queries exactly one-hot in fp32, so their output must be the winner's v row (the v part of qkv_bias for a pad winner) bit for bit."""
import ctypes

import pytest
import torch

import swin_ref as R
from abi_arena import Arena, frozen
from helpers import record_margins

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -5
_REFS = {}


def _ref(kind, name):
    """the float64 restatement of a case, its details, and the fp32 torch composition's error: computed once, shared, never modified"""
    key = (kind, name)
    if key not in _REFS:
        case = (R.core_case if kind == 'core' else R.selector_case)(name)
        out64, det = R.run_core(case, torch.float64, 'cpu', details=True)
        out32 = R.run_core(case, torch.float32, DEV).double().cpu()
        _REFS[key] = case, out64, det, (out32 - out64).abs().max().item()
    return _REFS[key]


def _run(vkn, case):
    dev = lambda t: None if t is None else t.to(DEV)      # noqa: E731
    out = vkn.ops.swin_window_attention(dev(case['qkv']), dev(case['qkv_bias']), dev(case['table']), case['H'], case['W'], case['heads'],
                                        case['window'], case['shift'], case['scale'])
    torch.cuda.synchronize()
    return out.view(case['B'], case['H'], case['W'], -1)


def _judge(test_id, got, want64, ref_err, extra=None):
    err = (got.double().cpu() - want64).abs().max().item()
    limit, ratio = R.bound(err, ref_err, want64.abs().max().item())
    record_margins(test_id, dict(err=err, torch_fp32_err=ref_err, limit=limit, ratio=ratio, **(extra or {})))
    assert err <= limit, f'{test_id}: error {err:.3e} over the limit {limit:.3e} (torch fp32 {ref_err:.3e})'


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_core_per_element(vkn, name):
    case, out64, _, ref_err = _ref('core', name)
    assert case['B'] * case['H'] * case['W'] <= 2 * 14 * 21
    got = _run(vkn, case)
    assert got.shape == out64.shape and bool(torch.isfinite(got).all())
    _judge(f'swin_core[{name}]', got, out64, ref_err)


@pytest.mark.parametrize('name', list(R.SELECTOR_CASES))
def test_selector_cases_bit_for_bit(vkn, name):
    case, out64, det, ref_err = _ref('selector', name)
    got = _run(vkn, case).cpu()
    heads = case['heads']
    decided = (det['lead'] >= R.DECIDED_LEAD).unsqueeze(-1).expand(-1, -1, -1, -1, R.HD).reshape(got.shape)
    want = det['winner_v'].float()                                    # fp32 inputs: the float64 v row converts back exactly
    assert torch.equal(want.double(), det['winner_v'])
    wrong = decided & (got != want)
    assert not bool(wrong.any()), f'{name}: {int(wrong.sum())} elements of decided queries are not their winner\'s v row, the first at {wrong.nonzero()[0].tolist()}'
    assert decided.float().mean().item() >= (0.25 if name == 'sel_two_offsets' else 0.5)      # (tests/test_swin_refs.py: why that case cannot reach one half)
    # the rest (ties, no such key in the window, a lead of 50): by the bound
    rest = ~decided
    err = ((got.double() - out64).abs() * rest).max().item()
    limit, ratio = R.bound(err, ref_err, out64.abs().max().item())
    record_margins(f'swin_selector[{name}]', dict(err=err, torch_fp32_err=ref_err, limit=limit, ratio=ratio, decided=decided.float().mean().item(), heads=heads))
    assert err <= limit


def test_buffer_contract_and_gates(vkn):
    """`out` of exactly its size between guards, on a padded shifted shape; the inputs are `const`; every refusal comes before a launch"""
    L = vkn._lib.lib()
    case = R.core_case('pad_both_shift')
    B, H, W, heads, ws, shift = (case[k] for k in ('B', 'H', 'W', 'heads', 'window', 'shift'))
    qkv, bias, table = case['qkv'].to(DEV), case['qkv_bias'].to(DEV), case['table'].to(DEV)
    assert all(t.data_ptr() % 16 == 0 for t in (qkv, bias, table))
    A = Arena(DEV)
    out = A.out((B, H, W, heads * R.HD), torch.float32, name='out')
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)

    def call(**kw):
        a = dict(qkv=qkv.data_ptr(), qkv_bias=bias.data_ptr(), table=table.data_ptr(), out=out.addr, B=B, H=H, W=W, heads=heads, window=ws, shift=shift)
        a.update(kw)
        return L.vkn_swin_window_attn_f32(ctypes.c_void_p(a['qkv']), ctypes.c_void_p(a['qkv_bias']), ctypes.c_void_p(a['table']), ctypes.c_void_p(a['out']),
                                          a['B'], a['H'], a['W'], a['heads'], a['window'], a['shift'], case['scale'], stream)
    with torch.cuda.device(DEV), frozen(qkv=qkv, qkv_bias=bias, table=table):
        # refused: nothing is written (the arena still holds its sentinel everywhere, `out` included)
        for kw in (dict(qkv=None), dict(table=None), dict(out=None), dict(B=0), dict(H=0), dict(W=-1), dict(heads=0)):
            assert call(**kw) == E_ARG, kw
        for kw in (dict(heads=65), dict(window=0), dict(window=9), dict(shift=ws), dict(shift=-1), dict(window=3, shift=3), dict(B=1 << 20, H=64, W=64)):
            assert call(**kw) == E_SHAPE, kw
        for k, p in dict(qkv=qkv.data_ptr(), qkv_bias=bias.data_ptr(), table=table.data_ptr(), out=out.addr).items():
            assert call(**{k: p + 4}) == call(**{k: p + 8}) == E_ALIGN, k
        assert call(shift=ws, out=out.addr + 4) == E_SHAPE and call(qkv=None, heads=65) == E_ARG          # the order of the refusals
        torch.cuda.synchronize()
        assert bool((A.words == 0x7FC0BEEF).all())
        assert call() == 0
        A.check('swin_window_attn_f32 on 10 x 17, window 7, shift 3')
    _, out64, _, ref_err = _ref('core', 'pad_both_shift')
    err = (out.t.double().cpu() - out64).abs().max().item()
    assert err <= R.bound(err, ref_err, out64.abs().max().item())[0]
    # the envelope query says what the entry says
    sup = vkn.ops.swin_window_attention_supported
    assert sup(B, H, W, heads, ws, shift) and sup(2, 200, 336, 4, 7, 3) and sup(1, 7, 7, 64, 8, 7)
    assert not sup(B, H, W, 65, ws, shift) and not sup(B, H, W, heads, 9, 0) and not sup(B, H, W, heads, ws, ws) and not sup(B, H, W, heads, ws, shift, head_dim=16)


def test_two_runs_and_a_graph_replay_give_the_same_bits(vkn):
    case = R.core_case('pad_both_shift')
    qkv, bias, table = case['qkv'].to(DEV), case['qkv_bias'].to(DEV), case['table'].to(DEV)
    run = lambda: vkn.ops.swin_window_attention(qkv, bias, table, case['H'], case['W'], case['heads'], case['window'], case['shift'], case['scale'])      # noqa: E731
    a, b = run(), run()
    torch.cuda.synchronize()
    assert torch.equal(a, b)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        run()                                                  # (the code object is loaded before the capture)
    torch.cuda.current_stream().wait_stream(s)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        cap = run()
    cap.zero_()
    g.replay()
    torch.cuda.synchronize()
    assert torch.equal(cap, a)


def _net_arms(vkn, make, seed):
    """the same module three times: fused fp32 on the device, forward_torch fp32 on the device, and its state dict in float64"""
    nets = []
    for fused in (True, False):
        m = make(fused).eval()
        m.load_state_dict(R.random_state(m, seed), strict=True)
        nets.append(m.to(DEV))
    sd64 = {k: v.double() for k, v in R.random_state(make(False), seed).items()}
    return nets[0], nets[1], sd64


def _paths(m):
    from video_k_net_amd import swin
    return [b.last_path for b in m.modules() if isinstance(b, swin.SwinTransformerBlock)]


@pytest.mark.parametrize('shift', (0, 3))
def test_block(vkn, shift):
    from video_k_net_amd import swin
    fused, plain, sd = _net_arms(vkn, lambda f: swin.SwinTransformerBlock(dim=64, num_heads=2, window_size=7, shift_size=shift, fused=f), 21 + shift)
    x = torch.randn((2, 170, 64), generator=torch.Generator().manual_seed(31))
    mask = R.painted_mask(10, 17, 7, 3, torch.float32).to(DEV)
    with torch.no_grad():
        for m in (fused, plain):
            m.H, m.W = 10, 17
        got, own = fused(x.to(DEV), mask), plain(x.to(DEV), mask)
        want = R.block(sd, '', x.double(), 10, 17, 2, 7, shift, mask.double().cpu())
    assert fused.last_path == 'fused' and plain.last_path == 'torch'
    _judge(f'swin_block[shift={shift}]', got, want, (own.double().cpu() - want).abs().max().item())


def test_basic_layer_with_patch_merging(vkn):
    from video_k_net_amd import swin
    fused, plain, sd = _net_arms(vkn, lambda f: swin.BasicLayer(dim=64, depth=2, num_heads=2, window_size=7, downsample=swin.PatchMerging, fused=f), 23)
    x = torch.randn((2, 11 * 15, 64), generator=torch.Generator().manual_seed(33))
    with torch.no_grad():
        got, own = fused(x.to(DEV), 11, 15), plain(x.to(DEV), 11, 15)
        want_out, want_down, wh, ww = R.layer(sd, '', x.double(), 11, 15, 2, 2, 7, True)
    assert _paths(fused) == ['fused', 'fused'] and _paths(plain) == ['torch', 'torch'] and got[1:3] == (11, 15) and got[4:] == (6, 8) == (wh, ww)
    _judge('swin_layer[out]', got[0], want_out, (own[0].double().cpu() - want_out).abs().max().item())
    _judge('swin_layer[down]', got[3], want_down, (own[3].double().cpu() - want_down).abs().max().item())


def test_whole_backbone(vkn):
    from video_k_net_amd import swin
    cfg = dict(embed_dims=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8])
    fused, plain, sd = _net_arms(vkn, lambda f: swin.SwinTransformerDIY(fused=f, **cfg), 25)
    img = torch.randn((2, 3, 61, 90), generator=torch.Generator().manual_seed(35))
    with torch.no_grad():
        got, own = fused(img.to(DEV)), plain(img.to(DEV))
        want = R.backbone(sd, img.double(), 32, cfg['depths'], cfg['num_heads'])
    assert _paths(fused) == ['fused'] * 8 and _paths(plain) == ['torch'] * 8 and len(got) == 4
    for i, (g, o, w) in enumerate(zip(got, own, want)):
        assert g.shape == w.shape
        _judge(f'swin_backbone[level {i}]', g, w, (o.double().cpu() - w).abs().max().item())


def test_path_choice(vkn):
    from video_k_net_amd import swin
    blk = swin.SwinTransformerBlock(dim=64, num_heads=2, window_size=7, shift_size=3, fused=True).to(DEV).eval()
    blk.H, blk.W = 10, 17
    x = torch.randn((1, 170, 64), device=DEV)
    mask = R.painted_mask(10, 17, 7, 3, torch.float32).to(DEV)
    with torch.no_grad():
        blk(x, mask)
        assert blk.last_path == 'fused'
        assert blk(x, None) is not None and blk.last_path == 'fused'           # the kernel computes the regions: no mask tensor is needed
    b = blk(x, mask)                                                            # parameters that need a gradient: the composition
    assert blk.last_path == 'torch' and b.requires_grad
    with torch.no_grad():
        blk.fused = False
        blk(x, mask)
        assert blk.last_path == 'torch'
        blk.fused = True
        odd = swin.SwinTransformerBlock(dim=64, num_heads=4, window_size=7, shift_size=3, fused=True).to(DEV).eval()      # head_dim 16
        odd.H, odd.W = 10, 17
        odd(x, mask)
        assert odd.last_path == 'torch'
        blk.train()
        blk(x, mask)
        assert blk.last_path == 'fused'                                         # attn_drop = 0: training mode alone changes nothing
        drop = swin.SwinTransformerBlock(dim=64, num_heads=2, window_size=7, shift_size=3, attn_drop=0.1, fused=True).to(DEV)
        drop.H, drop.W = 10, 17
        drop.train()
        drop(x, mask)
        assert drop.last_path == 'torch'
        drop.eval()
        drop(x, mask)
        assert drop.last_path == 'fused'


def test_a_shifted_block_behind_a_fused_one_keeps_its_mask(vkn):
    """Gradients enabled, everything frozen but block 0's MLP: the layer's input needs no gradient, so block 0 takes the kernel, its output
    needs one, so the shifted block 1 takes `forward_torch` — with the painted mask, decided on the `x` that reaches it."""
    from video_k_net_amd import swin
    fused, plain, sd = _net_arms(vkn, lambda f: swin.BasicLayer(dim=64, depth=2, num_heads=2, window_size=7, fused=f), 27)
    for m in (fused, plain):
        for p in m.parameters():
            p.requires_grad = False
        for p in m.blocks[0].mlp.parameters():
            p.requires_grad = True
    x = torch.randn((2, 10 * 17, 64), generator=torch.Generator().manual_seed(37))
    got, own = fused(x.to(DEV), 10, 17)[0], plain(x.to(DEV), 10, 17)[0]
    assert _paths(fused) == ['fused', 'torch'] and _paths(plain) == ['torch', 'torch'] and got.requires_grad
    want = R.layer(sd, '', x.double(), 10, 17, 2, 2, 7, False)[0]
    _judge('swin_layer[fused then torch, with a gradient]', got.detach(), want, (own.detach().double().cpu() - want).abs().max().item())
    got.square().mean().backward()
    assert fused.blocks[0].mlp.fc1.weight.grad is not None and bool(torch.isfinite(fused.blocks[0].mlp.fc1.weight.grad).all())
