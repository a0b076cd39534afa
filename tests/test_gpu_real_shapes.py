"""GPU: the joint panoptic merge at the frame shapes the reference really hands it.

`KernelIterHead.get_panoptic` / `VideoKernelIterHead.get_panoptic` (knet/det/kernel_iter_head.py:332-370, knet/video/kernel_iter_head.py:
591-640) receive the ALREADY up-scaled masks (`scaled_mask_preds`, upsample_stride = 1): a KITTI-STEP frame (48 x 156 features x 4) gives
192 x 624 logits, a Cityscapes frame (128 x 256 x 4) 512 x 1024.  The suite's other panoptic tests feed low-res logits (Wm <= 256); these
pin the wide-map path (k_pan_bounds' strip of full-width column rows, vkn_panoptic.hip) at KITTI's and Cityscapes' widths and at the
width edges 512 / 513 / 1025 / 2048 / 4096, against the CPU oracle where its cost is modest and against the torch chain on the device
(which materialises K x Ho x Wo) where it is not."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from helpers import PAN_CFG, assert_pan_matches_oracle, run_and_kernels
from oracle import synth
from oracle.knet_oracle import panoptic_joint as oracle_panoptic_joint

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N, NP, T, NCLS = 117, 100, 2, 19          # KITTI-STEP / Cityscapes panoptic: 100 proposals, 2 thing + 17 stuff classes


def _inputs(Hm, Wm, seed, up_from=1):
    """cls probabilities [1, N, ncls] and mask logits [1, N, Hm, Wm] (synth.panoptic_inputs); with `up_from` > 1 the logits are the
    F.interpolate x`up_from` up-scaling of low-res ones — what `_mask_forward` hands `get_panoptic`."""
    cls, low = synth.panoptic_inputs(1, N, NP, NCLS, Hm // up_from, Wm // up_from, seed)
    m = torch.from_numpy(low)
    if up_from > 1:
        m = F.interpolate(m, scale_factor=up_from, mode='bilinear', align_corners=False)
    assert tuple(m.shape[-2:]) == (Hm, Wm)
    return torch.from_numpy(cls), m.contiguous()


def _meta(img, bis, ori):
    return dict(img_shape=(img[0], img[1], 3), batch_input_shape=bis, ori_shape=(ori[0], ori[1], 3))


def _gpu(vkn, cls, m, meta):
    seg, info, nseg = vkn.ops.panoptic_joint(cls.to(DEV), m.to(DEV), NP, T, NP, PAN_CFG['instance_score_thr'], PAN_CFG['overlap_thr'],
                                             meta['img_shape'][:2], meta['batch_input_shape'], meta['ori_shape'][:2], upsample_stride=1)
    torch.cuda.synchronize()
    return seg, info, nseg


# (Hm, Wm, up_from, img_shape, batch_input_shape, ori_shape): up-scaled masks, upsample_stride = 1
ORACLE_CASES = {
    'kitti_376x1241': (192, 624, 4, (376, 1241), (384, 1248), (376, 1241)),     # KITTI-STEP test frame, img_shape = ori_shape
    'kitti_370x1226': (192, 624, 4, (370, 1226), (384, 1248), (370, 1226)),
    'w512': (64, 512, 1, (124, 1000), (128, 1024), (124, 1000)),                 # the last width the merge accepted before
    'w513_rescaled': (48, 513, 1, (90, 1020), (96, 1026), (135, 1530)),          # ori_shape != img_shape: three resampling levels
}


@pytest.mark.parametrize('name', list(ORACLE_CASES))
def test_panoptic_joint_wide_maps_vs_oracle(vkn, name):
    Hm, Wm, upf, img, bis, ori = ORACLE_CASES[name]
    cls, m = _inputs(Hm, Wm, 11 + Wm, upf)
    meta = _meta(img, bis, ori)
    seg, info, nseg = _gpu(vkn, cls, m, meta)
    seg, info, nseg = seg[0].cpu().numpy(), info[0].cpu().numpy(), nseg.cpu().numpy()
    assert int(info[:, 3].sum()) == ori[0] * ori[1]                      # every pixel is won by exactly one kernel
    assert int(nseg[0]) > 3
    with torch.no_grad():
        r = oracle_panoptic_joint(cls[0], m[0], NP, T, NP, PAN_CFG['instance_score_thr'], PAN_CFG['overlap_thr'], meta, upsample_stride=1)
    assert_pan_matches_oracle(seg, info, nseg[0], r)


TORCH_CASES = {
    'cityscapes_1024x2048': (512, 1024, 4, (1024, 2048), (1024, 2048), (1024, 2048)),   # Cityscapes: 128 x 256 features x 4
    'w1025_rescaled': (64, 1025, 1, (120, 2000), (128, 2050), (200, 2600)),             # odd width, ori_shape != img_shape
    'w2048': (32, 2048, 1, (60, 4000), (64, 4096), (60, 4000)),
    'w4096': (16, 4096, 1, (16, 4096), (16, 4096), (16, 4096)),                         # the documented limit (include/vkn.h)
}


@pytest.mark.parametrize('name', list(TORCH_CASES))
def test_panoptic_joint_wide_maps_vs_torch_chain(vkn, name):
    """the chain of test_gpu_parity.py::test_panoptic_joint_cfg2_size (resampling + sigmoid + score-weighted arg-max in torch on the
    device) at widths whose K x Ho x Wo CPU oracle would be slow"""
    Hm, Wm, upf, img, bis, ori = TORCH_CASES[name]
    cls, m = _inputs(Hm, Wm, 23 + Wm, upf)
    seg, info, nseg = _gpu(vkn, cls, m, _meta(img, bis, ori))
    info = info[0].cpu().numpy()
    K = info.shape[0]
    assert int(nseg[0]) > 3 and int(nseg[0]) == int((info[:, 2] > 0).sum())
    assert int(info[:, 3].sum()) == ori[0] * ori[1]                      # every pixel is won by exactly one kernel
    rows = torch.from_numpy(info[:, 0]).long().to(DEV)
    scores = torch.from_numpy(info[:, 5].view(np.float32).copy()).to(DEV)
    md = m[0].to(DEV)
    tm = F.interpolate(md[rows][None].sigmoid(), size=bis, mode='bilinear', align_corners=False)[0][:, :img[0], :img[1]]
    if tuple(ori) != tuple(img):
        tm = F.interpolate(tm[None], size=ori, mode='bilinear', align_corners=False)[0]
    del md
    prob = scores.view(-1, 1, 1) * tm
    top2 = prob.topk(2, dim=0)
    del prob
    near = (top2.values[0] - top2.values[1]) < 1e-6
    ids = top2.indices[0]
    del top2
    want = torch.from_numpy(info[:, 2]).to(DEV)[ids].int()
    diff = seg[0] != want
    assert not bool((diff & ~near).any()) and float(near.float().mean()) < 2e-3
    area = torch.bincount(ids.flatten(), minlength=K).cpu().numpy()
    assert np.abs(area - info[:, 3]).sum() <= 2 * int(near.sum())
    orig = (tm >= 0.5).flatten(1).sum(1).cpu().numpy()
    assert np.abs(orig - info[:, 4]).sum() <= int(((tm - 0.5).abs() < 1e-6).sum())


def test_panoptic_joint_refuses_past_the_width_limit(vkn):
    """Wm = 4097: VKN_E_SHAPE from the launcher's gate, before anything is launched (include/vkn.h: vkn_panoptic_joint_f32)"""
    cls, m = _inputs(8, 4097, 5)
    with pytest.raises(vkn._lib.VknError) as e:
        _gpu(vkn, cls, m, _meta((8, 4097), (8, 4097), (8, 4097)))
    assert e.value.code == -2


_TEST_CFG = dict(max_per_img=NP, mask_thr=0.5, stuff_score_thr=0.05,
                 merge_stuff_thing=dict(overlap_thr=0.6, iou_thr=0.5, stuff_max_area=4096, instance_score_thr=0.25))


@pytest.mark.parametrize('video', [False, True], ids=['det', 'video'])
def test_get_panoptic_at_the_kitti_frame_shape(vkn, video):
    """The reference's own route at a KITTI-STEP frame: `get_panoptic(cls, scaled_mask_preds[img], test_cfg, img_meta)` on the x4
    up-scaling of 48 x 156 head logits (Wm = 624), against the oracle; the video head also returns the accepted things' tracking
    embeddings (`thing_obj_feat`, knet/video/kernel_iter_head.py:903).  The low-res route of `simple_test`
    (`_panoptic_results(..., upsample_stride=4)`: the merge resamples the 48 x 156 logits itself) agrees with it up to arg-max near-ties."""
    from test_gpu_parity import _pan_compare
    from test_host_logic import _cfg
    cfg = _cfg(video, C=32, heads=4, ffn=64, ncls=NCLS, n_thing=T, n_stuff=NCLS - T, S=1, up=4, nprop=NP)
    cfg.update(do_panoptic=True, merge_joint=True, test_cfg=_TEST_CFG)
    head = vkn.build_head(cfg).to(DEV).eval()
    cls_np, low_np = synth.panoptic_inputs(1, N, NP, NCLS, 48, 156, 31)
    cls, low = torch.from_numpy(cls_np)[0], torch.from_numpy(low_np)
    scaled = F.interpolate(low, scale_factor=4, mode='bilinear', align_corners=False)[0]       # `_mask_forward`'s x4 (reference :122-130)
    meta = _meta((376, 1241), (384, 1248), (376, 1241))
    with torch.no_grad():
        r = oracle_panoptic_joint(cls, scaled, NP, T, NP, 0.25, 0.6, meta, upsample_stride=1)
    obj_feat = torch.randn(N, 32, generator=torch.Generator().manual_seed(3)).to(DEV)
    if video:
        bbox, segm, thing_masks, (seg, info), tfeat = head.get_panoptic(cls.to(DEV), scaled.to(DEV), head.test_cfg, meta, obj_feat=obj_feat)
        assert bbox is None and segm is None and thing_masks is None
        thing_rows = [int(r['rows'][s['instance_id']]) for s in r['segments_info'] if s['isthing']]
        assert len(thing_rows) > 0 and torch.equal(tfeat, obj_feat[thing_rows])
    else:
        bbox, segm, (seg, info) = head.get_panoptic(cls.to(DEV), scaled.to(DEV), head.test_cfg, meta)
        assert bbox is None and segm is None
    assert seg.dtype == np.int32 and seg.shape == (376, 1241)
    _pan_compare(seg, info, r)
    seg_lr, info_lr, _ = head._panoptic_results(cls[None].to(DEV), low.to(DEV), [meta], 4)[0]
    near = r['margin'].numpy() < 1e-6
    assert not ((seg_lr != seg) & ~near).any()
    _pan_compare(seg_lr, info_lr, r)


# ---------------------------------------------------------------------------------------------------- the head at KITTI-STEP's frame shape
KITTI_HEAD = dict(C=256, heads=8, ffn=2048, ncls=19, n_thing=2, n_stuff=17, S=3, up=4, nprop=100, N=117, H=48, W=156, B=1, seed=13, video=1)


@pytest.mark.parametrize('chain', ['ksplit', 'launches', 'persistent', 'persistent_bf16x3'])
def test_kitti_frame_head_vs_oracle(vkn, chain):
    """The cfg3 video head (C = 256, 8 heads, ffn 2048, N = 117, S = 3, ffn link) on one 384 x 1248 KITTI-STEP frame: 48 x 156
    features, P = 7488, a width that is not a multiple of 32 (ragged gather / decode / decode -> gather / upsample tiles).  Every chain
    form, teacher-forced stage by stage against the oracle with test_cfg2_size_head_vs_oracle's tolerances, then the fused 3-stage call
    bit-identical to the GPU's own stage-by-stage path."""
    from test_gpu_parity import head_vs_oracle_teacher_forced
    assert vkn._lib.lib().vkn_decode_gather_supported(256, 48 * 156) != 0      # the fused decode -> gather pass takes P = 7488
    head_vs_oracle_teacher_forced(vkn, chain, KITTI_HEAD)


@pytest.mark.parametrize('S', [4, 2])
def test_kitti_frame_upsample_vs_float64(vkn, S):
    """`mask_upsample_stride` 4 (the video configs) and 2 (the image K-Net KITTI config) on 48 x 156 logits against F.interpolate
    (bilinear, align_corners=False) in float64"""
    low = torch.randn(2, 117, 48, 156, generator=torch.Generator().manual_seed(S)).mul_(4).to(DEV)
    out = vkn.ops.upsample_bilinear(low, S)
    ref = F.interpolate(low.double(), scale_factor=S, mode='bilinear', align_corners=False)
    assert out.shape == ref.shape and float((out.double() - ref).abs().max()) < 4e-6 * float(ref.abs().max())


def _has(names, kernel):
    return any(kernel in n for n in names)


# rows = 117 B: row tiles of 32 -> 4 / 8 (few-row chain up to 16 tiles) and 30 (persistent chain from 22 tiles: vkn_api.hip)
FORM_KERNEL = dict(ksplit='k_gemm_ks', persistent='k_chain_')


@pytest.mark.parametrize('B,form', [(1, 'ksplit'), (2, 'ksplit'), (8, 'persistent')], ids=['b1_117rows', 'b2_234rows', 'b8_936rows'])
def test_kitti_frame_default_policy(vkn, B, form):
    """The default chain policy at 1, 2 and 8 KITTI-STEP frames (48 x 156, P = 7488): teacher-forced stage by stage against the oracle
    (two distinct frames A B A B ..., every copy bit-identical to its twin; test_cfg2_size_batch_of_32_default_policy_vs_oracle's checks),
    the fused call bit-identical to the stage-by-stage path.  Then the fused default call
      * IS the chain form the row count selects (few-row at 117 / 234 rows, persistent at 936): the same bits as that form forced by its
        flag, and that form's kernels run;
      * runs the fused decode -> gather pass (k_fused_il), which this width is eligible for (P % 64 == 0);
      * gives the same bits with VKN_FLAG_BITS_HANDOFF and VKN_FLAG_LOGITS_HANDOFF (include/vkn.h: "same results"), which do not run it."""
    from test_gpu_parity import _chain_flags, batch_default_policy_vs_oracle
    ops = vkn.ops
    assert vkn._lib.lib().vkn_decode_gather_supported(256, 48 * 156) != 0
    head, ins, outs = batch_default_policy_vs_oracle(vkn, B, 48, 156)

    def same(a, b):
        return all((u is None and v is None) or torch.equal(u, v) for u, v in zip(a, b))
    with torch.no_grad():
        run = lambda flags=0: head._head_forward(*ins, want_track=True, flags=flags)     # noqa: E731
        a, names = run_and_kernels(run)
        assert same(a, outs)
        assert _has(names, 'k_fused_il'), sorted(n for n in names if n.startswith(('k_', 'void k_')))
        assert _has(names, FORM_KERNEL[form]), sorted(n for n in names if 'k_' in n)
        assert same(run(_chain_flags(vkn, form)), outs), f'the default call at {117 * B} rows is not the {form} chain'
        for fl in (ops.FLAG_BITS_HANDOFF, ops.FLAG_LOGITS_HANDOFF):
            c, cn = run_and_kernels(lambda: run(fl))
            assert same(c, outs), fl
            assert not _has(cn, 'k_fused_il'), fl
