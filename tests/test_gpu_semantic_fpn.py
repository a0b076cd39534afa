"""The localization FPN on the MI355X (video-k-net_amd/csrc/vkn_fpn.hip, include/vkn.h: vkn_conv_gn_f32 / vkn_localization_fpn_f32).

Oracle: a float64 torch restatement written here (knet/det/semantic_fpn_wrapper.py:197-237 with mmcv ConvModule = conv -> GN -> ReLU,
knet/det/kernel_head.py:207-230 for the loc / seg convs).  Accuracy rule for every output:
    max|hip - ref64| <= max(4 * max|torch32 - ref64|, 2e-5 * max|ref64|)
where torch32 is the same module's torch composition on the GPU in fp32."""
import copy
import math

import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

SHIPPED = dict(type='SemanticFPNWrapper', in_channels=256, feat_channels=256, out_channels=256, start_level=0, end_level=3,
               upsample_times=2, num_aux_convs=1, cat_coors=False, fuse_by_cat=False,
               positional_encoding=dict(type='SinePositionalEncoding', num_feats=128, normalize=True),
               norm_cfg=dict(type='GN', num_groups=32, requires_grad=True))
KITTI = [(96, 312), (48, 156), (24, 78), (12, 39)]          # P2..P5 of a 384 x 1248 frame
CITY = [(256, 512), (128, 256), (64, 128), (32, 64)]        # P2..P5 of a 1024 x 2048 frame
DEV = 'cuda:0'
MARGINS = {}


def _rule(name, hip, t32, r64):
    e_hip = (hip.double() - r64).abs().max().item()
    e_t32 = (t32.double() - r64).abs().max().item()
    bound = max(4 * e_t32, 2e-5 * r64.abs().max().item())
    MARGINS[name] = (e_hip, e_t32, bound)
    print(f'{name}: hip {e_hip:.3e}  torch32 {e_t32:.3e}  bound {bound:.3e}')
    assert e_hip <= bound, (name, e_hip, e_t32, bound)


def _pos64(num_feats, H, W, dev):
    y = torch.arange(1, H + 1, dtype=torch.float64, device=dev)[:, None].expand(H, W) / (H + 1e-6) * 2 * math.pi
    x = torch.arange(1, W + 1, dtype=torch.float64, device=dev)[None, :].expand(H, W) / (W + 1e-6) * 2 * math.pi
    k = torch.arange(num_feats, dtype=torch.float64, device=dev)
    dim_t = 10000 ** (2 * torch.div(k, 2, rounding_mode='floor') / num_feats)
    py, px = y[None] / dim_t[:, None, None], x[None] / dim_t[:, None, None]
    even = (torch.arange(num_feats, device=dev) % 2 == 0)[:, None, None]
    return torch.cat([torch.where(even, py.sin(), py.cos()), torch.where(even, px.sin(), px.cos())], 0)


def _cm64(mod, x, stride=1):
    k = mod.conv.kernel_size[0]
    y = F.conv2d(x, mod.conv.weight.detach().double(), stride=stride, padding=k // 2)
    y = F.group_norm(y, mod.gn.num_groups, mod.gn.weight.detach().double(), mod.gn.bias.detach().double(), 1e-5)
    return y.clamp_min(0)


def _up(x):
    return F.interpolate(x, scale_factor=2, mode='bilinear', align_corners=False)


def fpn_ref64(m, inputs):
    p2, p3, p4, p5 = [t.double() for t in inputs]
    L = m.convs_all_levels
    l0 = _cm64(L[0].conv0, p2, 2)
    l1 = _cm64(L[1].conv0, p3)
    l2 = _cm64(L[2].conv1, _up(_cm64(L[2].conv0, p4)))
    x5 = p5 + _pos64(m.positional_encoding.num_feats, p5.shape[-2], p5.shape[-1], p5.device)
    l3 = _cm64(L[3].conv2, _up(_cm64(L[3].conv1, _up(_cm64(L[3].conv0, x5)))))
    s = ((l0 + l1) + l2) + l3
    return _cm64(m.conv_pred, s), _cm64(m.aux_convs[0], s)


def _module(vkn, C=256, seed=0):
    torch.manual_seed(seed)
    cfg = copy.deepcopy(SHIPPED)
    cfg.update(in_channels=C, feat_channels=C, out_channels=C)
    m = vkn.registry.HEADS.build(cfg)
    m.init_weights()
    with torch.no_grad():
        for mod in m.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
    return m.to(DEV).eval()


def _loc_seg(vkn, C=256, seed=1):
    torch.manual_seed(seed)
    from importlib import import_module
    kh = import_module('video_k_net_amd.kernel_head')
    convs = [kh._ConvGNReLU(C, C, 1, norm_cfg=dict(type='GN', num_groups=32)) for _ in range(2)]
    for c in convs:
        torch.nn.init.normal_(c.conv.weight, 0, 0.05)
        with torch.no_grad():
            c.gn.weight.uniform_(0.5, 1.5)
            c.gn.bias.uniform_(-0.3, 0.3)
    return [c.to(DEV).eval() for c in convs]


def _levels(B, C, shapes, seed=2, scale=1.0):
    g = torch.Generator(device='cpu').manual_seed(seed)
    return [(torch.randn(B, C, h, w, generator=g) * scale).to(DEV) for h, w in shapes]


# ---------------------------------------------------------------------------------------------------------- building block
def _block_case(vkn, C, H, W, stride, mode, seed):
    g = torch.Generator(device='cpu').manual_seed(seed)
    B, G = 2, 32
    x = torch.randn(B, C, H, W, generator=g).to(DEV)
    w = (torch.randn(C, C, 3, 3, generator=g) * 0.01).to(DEV)
    img = vkn.ops.conv_prepare(w)
    pos = ins = gam = bet = None
    x64 = x.double()
    if mode == 'pos':
        pos = torch.randn(C, H, W, generator=g).to(DEV)
        x32 = x + pos
        x64 = x64 + pos.double()
    elif mode in ('norm', 'up'):
        xr = x * 3 + 1                                  # a "previous raw output" and its GroupNorm statistics
        x = xr
        gam = torch.rand(C, generator=g).to(DEV) + 0.5
        bet = (torch.rand(C, generator=g).to(DEV) - 0.5) * 0.6
        v = xr.view(B, G, -1)
        mean = v.mean(-1)
        rstd = (v.var(-1, unbiased=False) + 1e-5).rsqrt()
        ins = torch.stack([mean, rstd], -1).contiguous()
        cpg = C // G
        m64, r64 = mean.double().repeat_interleave(cpg, 1)[..., None, None], rstd.double().repeat_interleave(cpg, 1)[..., None, None]
        x64 = ((xr.double() - m64) * r64 * gam.double()[None, :, None, None] + bet.double()[None, :, None, None]).clamp_min(0)
        m32, r32 = mean.repeat_interleave(cpg, 1)[..., None, None], rstd.repeat_interleave(cpg, 1)[..., None, None]
        x32 = ((xr - m32) * r32 * gam[None, :, None, None] + bet[None, :, None, None]).clamp_min(0)
        if mode == 'up':
            x64, x32 = _up(x64), _up(x32)
    else:
        x32 = x
    out, st = vkn.ops.conv_gn(x, img, C, 3, stride, G, pos=pos, in_stats=ins, in_gamma=gam, in_beta=bet, upsample=(mode == 'up'))
    r64 = F.conv2d(x64, w.double(), stride=stride, padding=1)
    t32 = F.conv2d(x32, w, stride=stride, padding=1)
    _rule(f'block C{C} {H}x{W} s{stride} {mode}', out, t32, r64)
    v64 = r64.view(B, G, -1)
    mean64, var64 = v64.mean(-1), v64.var(-1, unbiased=False)
    rstd64 = (var64 + 1e-5).rsqrt()
    v32 = t32.view(B, G, -1)
    _rule(f'block C{C} {H}x{W} s{stride} {mode} mean', st[..., 0], v32.mean(-1), mean64)
    _rule(f'block C{C} {H}x{W} s{stride} {mode} rstd', st[..., 1], (v32.var(-1, unbiased=False) + 1e-5).rsqrt(), rstd64)


@pytest.mark.parametrize('C', [64, 256])
@pytest.mark.parametrize('mode', ['raw', 'pos', 'norm', 'up'])
def test_conv_gn_block(vkn, C, mode):
    with torch.no_grad():
        for i, (H, W) in enumerate([(1, 1), (3, 5), (12, 39), (24, 78), (47, 155), (48, 156)]):
            for stride in (1, 2):
                if mode == 'up' and H * W > 24 * 78:
                    continue                                 # the conv input is (2H, 2W): the two largest sizes are covered above
                _block_case(vkn, C, H, W, stride, mode, seed=100 * i + stride)
    vkn.ops.workspace_status()


# ---------------------------------------------------------------------------------------------------------- whole module
def _whole(vkn, B, shapes, with_ls=True):
    m = _module(vkn)
    ls = _loc_seg(vkn) if with_ls else None
    x = _levels(B, 256, shapes)
    with torch.no_grad():
        hip = m.forward_fused(x, *ls) if with_ls else m(x)
        t_out, t_aux = m.forward_torch(x)
        r_out, r_aux = fpn_ref64(m, x)
        if with_ls:
            t = (ls[0](t_out), ls[1](t_aux))
            r = (_cm64(ls[0], r_out), _cm64(ls[1], r_aux))
        else:
            t, r = (t_out, t_aux), (r_out, r_aux)
    vkn.ops.workspace_status()
    names = ('loc', 'sem') if with_ls else ('out', 'aux')
    for n, h, tt, rr in zip(names, hip, t, r):
        assert h.shape == rr.shape
        _rule(f'fpn B{B} {shapes[1]} {n}', h, tt, rr)
    return m, ls, x, hip


@pytest.mark.parametrize('B', [1, 2])
def test_fpn_kitti_levels(vkn, B):
    _whole(vkn, B, KITTI)


def test_fpn_module_outputs_kitti(vkn):
    _whole(vkn, 1, KITTI, with_ls=False)


def test_fpn_cityscapes_levels(vkn):
    _whole(vkn, 1, CITY)


def test_fpn_deterministic_and_graph_replay(vkn):
    m, ls, x, hip = _whole(vkn, 2, KITTI)
    with torch.no_grad():
        again = m.forward_fused(x, *ls)
        for a, b in zip(hip, again):
            assert torch.equal(a, b)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            m.forward_fused(x, *ls)                         # warm-up on the capture stream: workspace and weight images exist
        torch.cuda.current_stream().wait_stream(s)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=s):
            cap = m.forward_fused(x, *ls)
        graph.replay()
        torch.cuda.synchronize()
        for a, b in zip(hip, cap):
            assert torch.equal(a, b)


def test_fpn_out_of_range_is_flagged_not_silent(vkn):
    m = _module(vkn)
    ls = _loc_seg(vkn)
    for kind in ('scaled', 'nan'):
        x = _levels(1, 256, KITTI, scale=1e5 if kind == 'scaled' else 1.0)
        if kind == 'nan':
            x[1][0, 7, 5, 9] = float('nan')
        with torch.no_grad():
            hip = m.forward_fused(x, *ls)
            try:
                vkn.ops.workspace_status()
                flagged = False
            except vkn.VknError as e:
                assert e.code == -6
                flagged = True
            if not flagged:
                r_out, r_aux = fpn_ref64(m, x)
                r = (_cm64(ls[0], r_out), _cm64(ls[1], r_aux))
                for h, rr in zip(hip, r):
                    assert (h.double() - rr).abs().max().item() <= 2e-5 * rr.abs().max().item(), kind
        print(kind, 'flagged' if flagged else 'correct')
        if kind == 'nan':
            assert flagged


def test_fpn_inconsistent_levels_raise(vkn):
    m = _module(vkn)
    x = _levels(1, 256, [(96, 312), (48, 156), (24, 78), (13, 39)])
    with torch.no_grad(), pytest.raises(vkn.VknError) as e:
        m(x)
    assert e.value.code == -2


# ---------------------------------------------------------------------------------------------------------- the head's RPN
def test_simple_test_rpn_from_p2_p5(vkn):
    from test_semantic_fpn_surface import RPN
    cfg = copy.deepcopy(RPN[sorted(RPN)[0]])
    torch.manual_seed(3)
    head = vkn.build_head(cfg)
    head.init_weights()
    with torch.no_grad():
        for mod in head.modules():
            if isinstance(mod, torch.nn.GroupNorm):
                mod.weight.uniform_(0.5, 1.5)
                mod.bias.uniform_(-0.3, 0.3)
        for c in list(head.loc_convs) + list(head.seg_convs):
            torch.nn.init.normal_(c.conv.weight, 0, 0.05)
    head = head.to(DEV).eval()
    x = _levels(1, 256, KITTI)
    prop, xf, masks, _, seg = head.simple_test_rpn(x, [dict()])
    vkn.ops.workspace_status()                                  # the fused call's range flag (VKN_STATUS_RANGE) is clear
    fpn = head.localization_fpn
    with torch.no_grad():
        t_out, t_aux = fpn.forward_torch(x)
        t_loc, t_sem = head.loc_convs[0](t_out), head.seg_convs[0](t_aux)
        tprop, txf, tmasks, _, tseg = head.decode_init_proposals_from_feats(t_loc, t_sem)
        r_out, r_aux = fpn_ref64(fpn, x)
        r_loc, r_sem = _cm64(head.loc_convs[0], r_out), _cm64(head.seg_convs[0], r_aux)
        rprop, _, rmasks, _, _ = head.decode_init_proposals_from_feats(r_loc.float(), r_sem.float())
    _rule('rpn x_feats', xf, txf, r_loc + r_sem)
    flips = int(((masks >= 0) != (rmasks >= 0)).sum())
    tflips = int(((tmasks >= 0) != (rmasks >= 0)).sum())
    print(f'binarised-mask flips: hip {flips}, torch32 {tflips} of {masks.numel()}')
    assert flips <= max(4 * tflips, 1e-4 * masks.numel())
    if flips == 0:
        _rule('rpn proposal_feats', prop, tprop, rprop.double())
    else:    # a flipped pixel moves its row's sum by one x_feats value
        e = (prop.double() - rprop.double()).abs().max().item()
        assert e <= flips * (r_loc + r_sem).abs().max().item() + 2e-5 * rprop.abs().max().item()
