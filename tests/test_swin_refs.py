"""CPU: the premises of tests/swin_ref.py, the float64 restatement that tests/test_gpu_swin.py judges the Swin kernel and modules by.
  * the package's `forward_torch` (video-k-net_amd/swin.py) and the restatement are two independent writings of the reference's lines:
    in float64 they agree to 1e-12, on a block of every core case's geometry, on the module cases, and from the rows of the qkv Linear
    (a pad token's row is that Linear's bias);
  * the arithmetic of include/vkn_swin.h (the region rule, rel(i, j)) equals the tensors the reference paints and gathers;
  * the selector cases decide what tests/test_gpu_swin.py takes them to decide."""
import pytest
import torch

import swin_ref as R


def _block(vkn, dim, heads, ws, shift, seed, **kw):
    from video_k_net_amd import swin
    blk = swin.SwinTransformerBlock(dim=dim, num_heads=heads, window_size=ws, shift_size=shift, **kw).eval()
    blk.load_state_dict(R.random_state(blk, seed), strict=True)
    return blk


@pytest.mark.parametrize('name', list(R.CORE_CASES))
def test_forward_torch_is_the_restatement_on_every_core_geometry(vkn, name):
    from video_k_net_amd import swin
    B, H, W, ws, shift, heads, _ = R.CORE_CASES[name]
    dim = heads * R.HD
    blk = _block(vkn, dim, heads, ws, shift, 7, mlp_ratio=1.).double()
    sd = blk.state_dict()
    x = torch.randn((B, H * W, dim), dtype=torch.float64, generator=torch.Generator().manual_seed(3))
    blk.H, blk.W = H, W
    mask = swin.shift_attention_mask(H, W, ws, max(shift, 1), dtype=torch.float64)
    ref_mask = R.painted_mask(H, W, ws, max(shift, 1), torch.float64)
    assert torch.equal(mask, ref_mask)
    with torch.no_grad():
        own = blk.forward_torch(x, mask)
        assert blk.last_path == 'torch'
        ref = R.block(sd, '', x, H, W, heads, ws, shift, ref_mask)
        assert (own - ref).abs().max().item() <= 1e-12
        # from the Linear's rows on the tokens as they are: what the kernel is given
        n1 = blk.norm1(x)
        qkv = blk.attn.qkv(n1).view(B, H, W, 3, heads, R.HD)
        core = R.core(qkv, sd['attn.qkv.bias'], sd['attn.relative_position_bias_table'], heads, ws, shift, blk.attn.scale)
        span = blk.attention_torch(n1, mask)
        assert (blk.attn.proj(core.view(B, H * W, dim)) - span).abs().max().item() <= 1e-12


def test_forward_torch_is_the_restatement_on_the_module_cases(vkn):
    from video_k_net_amd import swin
    g = torch.Generator().manual_seed(5)
    with torch.no_grad():
        for shift in (0, 3):                                   # a block, dim 64, 2 heads, 10 x 17: both arms
            blk = _block(vkn, 64, 2, 7, shift, 11 + shift).double()
            blk.H, blk.W = 10, 17
            x = torch.randn((2, 170, 64), dtype=torch.float64, generator=g)
            mask = R.painted_mask(10, 17, 7, 3, torch.float64)
            assert (blk.forward_torch(x, mask) - R.block(blk.state_dict(), '', x, 10, 17, 2, 7, shift, mask)).abs().max().item() <= 1e-12
        lay = swin.BasicLayer(dim=64, depth=2, num_heads=2, window_size=7, downsample=swin.PatchMerging).eval()
        lay.load_state_dict(R.random_state(lay, 13), strict=True)
        lay = lay.double()
        x = torch.randn((2, 11 * 15, 64), dtype=torch.float64, generator=g)
        x_out, H, W, x_down, Wh, Ww = lay(x, 11, 15)
        r_out, r_down, rh, rw = R.layer(lay.state_dict(), '', x, 11, 15, 2, 2, 7, True)
        assert (H, W, Wh, Ww) == (11, 15, 6, 8) == (11, 15, rh, rw) and x_down.shape == (2, 48, 128)
        assert (x_out - r_out).abs().max().item() <= 1e-12 and (x_down - r_down).abs().max().item() <= 1e-12
        net = swin.SwinTransformerDIY(embed_dims=32, depths=[2, 2, 2, 2], num_heads=[1, 2, 4, 8]).eval()
        net.load_state_dict(R.random_state(net, 17), strict=True)
        net = net.double()
        img = torch.randn((2, 3, 61, 90), dtype=torch.float64, generator=g)
        outs, refs = net(img), R.backbone(net.state_dict(), img, 32, [2, 2, 2, 2], [1, 2, 4, 8])
        assert [tuple(o.shape) for o in outs] == [(2, 32, 16, 23), (2, 64, 8, 12), (2, 128, 4, 6), (2, 256, 2, 3)] == [tuple(o.shape) for o in refs]
        for o, r in zip(outs, refs):
            assert (o - r).abs().max().item() <= 1e-12 * max(1.0, r.abs().max().item())


def _r(s, E, ws, shift):
    """include/vkn_swin.h: the slice of a rolled axis of extent E that position s falls in"""
    return 0 if s < E - ws else (1 if s < E - shift else 2)


def test_the_region_rule_is_the_painted_mask():
    n = 0
    for ws in range(2, 9):
        for shift in range(1, ws):
            for nh in (1, 2, 3):
                for nw in (1, 2, 3):
                    Hp, Wp = nh * ws, nw * ws
                    painted = R.painted_regions(Hp, Wp, ws, shift)[0, :, :, 0].long()
                    rule = torch.tensor([[3 * _r(y, Hp, ws, shift) + _r(x, Wp, ws, shift) for x in range(Wp)] for y in range(Hp)])
                    assert torch.equal(painted, rule), (ws, shift, Hp, Wp)
                    n += 1
    assert n == sum(ws - 1 for ws in range(2, 9)) * 9
    # one window along an axis: region 0 of that axis is empty
    assert set(R.painted_regions(7, 14, 7, 3)[0, :, :, 0].long().flatten().tolist()) == {3, 4, 5, 6, 7, 8}


def test_rel_is_relative_position_index(vkn):
    from video_k_net_amd import swin
    for ws in range(1, 9):
        idx = R.rel_index(ws)
        rule = torch.tensor([[(i // ws - j // ws + ws - 1) * (2 * ws - 1) + (i % ws - j % ws + ws - 1) for j in range(ws * ws)] for i in range(ws * ws)])
        assert torch.equal(idx, rule) and torch.equal(swin.relative_position_index((ws, ws)), rule), ws
        assert int(idx.min()) == 0 and int(idx.max()) == (2 * ws - 1) ** 2 - 1


def test_scores80_has_scores_of_that_magnitude():
    case = R.core_case('scores80')
    q, k = case['qkv'][:, :, :, 0].double(), case['qkv'][:, :, :, 1].double()
    s = torch.einsum('bhwmd,bhwmd->bhwm', q, k) * case['scale']            # a token with itself: a lower bound on the window's largest
    assert 80 <= s.abs().max().item() <= 2000
    plain = R.core_case('pad_both_shift')
    assert plain['qkv'].abs().max().item() < 6


@pytest.mark.parametrize('name', list(R.SELECTOR_CASES))
def test_selector_cases_decide_as_claimed(name):
    """On the float64 restatement alone.  A query is DECIDED when its best score leads the second by >= 150: exp(-150) is 0 in fp32, so
    its fp32 softmax is exactly one-hot and its output is the winner's v row, bit for bit."""
    case = R.selector_case(name)
    out, d = R.run_core(case, details=True)
    decided = d['lead'] >= R.DECIDED_LEAD
    B, H, W, ws, shift, heads, offsets = R.SELECTOR_CASES[name]
    frac = decided.double().mean().item()
    print(f'{name}: decided {frac:.3f} of {decided.numel()} queries, pad winners {int((decided & d["winner_pad"]).sum())}')
    # a decided query's float64 output IS the winner's row to rounding: the restatement's own softmax agrees with the claim
    sel = decided.unsqueeze(-1).expand(-1, -1, -1, -1, R.HD).reshape(out.shape)
    assert (out - d['winner_v'])[sel].abs().max().item() <= 1e-12
    if len(offsets) == 1:
        # the key is the query's right (in one case left) neighbour in its window: every query but those of a window's last (first) column has one, and it
        # leads by 300 (masked) or 400
        assert frac >= 0.5
        assert frac == pytest.approx((ws - 1) / ws, abs=0.2)
    else:
        # two offsets, 0 at (0, +1) and -50 at (+1, 0): where both keys are present and unmasked the lead is 50 and nothing is decided
        # bit for bit (such a query is judged by the bound).  The mask decides the rest: a masked lower neighbour (-150) leaves the right
        # one leading by 150, and without the -100 NONE of these queries would be decided.
        # Only at window 2, where half of a window's queries have just one of the two keys, is half of the case decided.
        assert (frac >= 0.5) if ws == 2 else (0 < frac < 0.5)
        slot = d['slot'].unsqueeze(-1).expand_as(decided)
        inner = (slot // ws < ws - 1) & (slot % ws < ws - 1)                               # both neighbours lie in the query's window
        by_mask = decided & inner
        assert bool(by_mask.any()) and bool((d['winner_slot'][by_mask] == slot[by_mask] + 1).all())
        # ... and the mask turns the winner: a masked right neighbour (-100) loses to the lower one (-50); without the -100 it would win
        turned = inner & (d['winner_slot'] == slot + ws) & (d['lead'] == 50)
        assert bool(turned.any()) and bool((d['winner_region'][turned] == d['region'].unsqueeze(-1).expand_as(turned)[turned]).all())
    if 'pad' in name or 'small' in name:
        assert bool((decided & d['winner_pad']).any()), 'no decided query is won by a pad token'
    if name == 'sel_nine_regions':
        # winners in ANOTHER region than the query's, for every region that holds a query whose right neighbour in the window lies across
        # a region border INSIDE a window: the rolled map is cut at columns 7 and 11, 7 is a window's edge, so those are regions 1, 4, 7
        cross = decided & (d['winner_region'] != d['region'].unsqueeze(-1))
        assert set(d['region'].unsqueeze(-1).expand_as(cross)[cross].tolist()) == {1, 4, 7}
        assert set(d['region'].flatten().tolist()) == set(range(9))


@pytest.mark.parametrize('ws,shift,H,W', [(7, 3, 10, 17), (4, 2, 8, 12), (2, 1, 5, 6)])
def test_a_shifted_block_is_never_attended_without_its_mask(vkn, ws, shift, H, W):
    """`forward_torch(x, None)` on a shifted block paints the mask itself: it equals `forward_torch(x, mask)`, and differs from the
    unmasked attention (which a `None` once meant)."""
    from video_k_net_amd import swin
    blk = _block(vkn, 64, 2, ws, shift, 41).double()
    blk.H, blk.W = H, W
    x = torch.randn((2, H * W, 64), dtype=torch.float64, generator=torch.Generator().manual_seed(9))
    mask = R.painted_mask(H, W, ws, shift, torch.float64)
    with torch.no_grad():
        with_mask, without = blk.forward_torch(x, mask), blk.forward_torch(x, None)
        assert torch.equal(with_mask, without)
        assert (with_mask - blk.forward_torch(x, torch.zeros_like(mask))).abs().max().item() > 1e-6
    # a layer whose first block's output needs a gradient where its input did not: the shifted block gets its mask all the same
    lay = swin.BasicLayer(dim=64, depth=2, num_heads=2, window_size=ws, fused=True).eval()
    lay.load_state_dict(R.random_state(lay, 43), strict=True)
    lay = lay.double()
    for p in lay.parameters():
        p.requires_grad = False
    for p in lay.blocks[0].mlp.parameters():
        p.requires_grad = True
    out = lay(x, H, W)[0]
    ref = R.layer(lay.state_dict(), '', x, H, W, 2, 2, ws, False)[0]
    assert out.requires_grad and (out - ref).abs().max().item() <= 1e-12
