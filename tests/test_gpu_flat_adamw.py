"""GPU (-m gpu): dist.FlatAdamW — AdamW behind a global L2 gradient clip over the flat gradient buckets (vkn_adamw_flat_f32) — against
a float64 restatement of clip + AdamW, against torch.optim.AdamW + clip_grad_norm_, through LR schedulers and checkpoints in both
directions, and on the real video head (train_video_c256)."""
import copy
import io
import math
from importlib import import_module

import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

# parameter indices of _net() per group: three groups, different lr, one without weight decay, per-group betas
GROUPS = [([0, 1], dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.05)),
          ([2, 3], dict(lr=3e-3, betas=(0.8, 0.99), eps=1e-6, weight_decay=0.0)),
          ([4, 5, 6], dict(lr=5e-4, betas=(0.95, 0.98), eps=1e-8, weight_decay=0.1))]


def _dist():
    return import_module('video_k_net_amd.dist')


def _net(seed=3):
    torch.manual_seed(seed)     # 37 x 300 = 11100 weights: one parameter spans two work items
    return torch.nn.Sequential(torch.nn.Linear(37, 300), torch.nn.LayerNorm(300), torch.nn.Linear(300, 11, bias=False),
                               torch.nn.Linear(11, 5)).to(DEV)


def _groups(net, spec=GROUPS):
    ps = list(net.parameters())
    return [dict(params=[ps[i] for i in idx], **hp) for idx, hp in spec]


def _flat(net, max_norm, spec=GROUPS, **kw):
    d = _dist()
    red = d.BucketedGradAllReducer(net, bucket_of=lambda name: 'a' if name.startswith(('0', '1')) else 'b')
    return red, d.FlatAdamW(red, _groups(net, spec), max_norm=max_norm, **kw)


def _torch(net, spec=GROUPS):
    return torch.optim.AdamW(_groups(net, spec))


def _grads(net, step, seed=11):
    g = torch.Generator(device='cpu').manual_seed(seed * 1000 + step)
    return [(torch.randn(tuple(p.shape), generator=g) * (0.05 * (i + 1))).to(DEV) for i, p in enumerate(net.parameters())]


def _step_flat(net, red, opt, grads, skip=()):
    red.zero_grad(set_to_none=True)
    for i, (p, g) in enumerate(zip(net.parameters(), grads)):
        if i not in skip:
            p.grad = g.clone()
    red.finalize()
    opt.step()


def _step_torch(net, opt, grads, max_norm, skip=()):
    for i, (p, g) in enumerate(zip(net.parameters(), grads)):
        p.grad = None if i in skip else g.clone()
    norm = torch.nn.utils.clip_grad_norm_([p for p in net.parameters() if p.grad is not None], max_norm) if max_norm else None
    opt.step()
    return norm


class _Ref64:
    """clip_grad_norm_ + torch.optim.AdamW restated in float64 (plain torch, no optimizer object)."""

    def __init__(self, net, spec=GROUPS):
        self.p = [p.detach().double().clone() for p in net.parameters()]
        self.m = [torch.zeros_like(p) for p in self.p]
        self.v = [torch.zeros_like(p) for p in self.p]
        self.t = [0] * len(self.p)
        self.hp = {i: hp for idx, hp in spec for i in idx}

    def step(self, grads, max_norm, skip=()):
        act = [i for i in range(len(self.p)) if i not in skip]
        g = {i: grads[i].double() for i in act}
        norm = math.sqrt(sum(float((g[i] ** 2).sum()) for i in act))
        if max_norm:
            coef = min(max_norm / (norm + 1e-6), 1.0)
            g = {i: g[i] * coef for i in act}
        for i in act:
            h = self.hp[i]
            (b1, b2), lr = h['betas'], h['lr']
            self.t[i] += 1
            self.p[i] *= 1 - lr * h['weight_decay']
            self.m[i] = b1 * self.m[i] + (1 - b1) * g[i]
            self.v[i] = b2 * self.v[i] + (1 - b2) * g[i] ** 2
            bc1, bc2 = 1 - b1 ** self.t[i], 1 - b2 ** self.t[i]
            self.p[i] -= lr / bc1 * self.m[i] / (self.v[i].sqrt() / math.sqrt(bc2) + h['eps'])
        return norm


def _assert_views(params, opt):
    """Every parameter is a view of its bucket's flat parameter buffer, on a 256-byte boundary."""
    ranges = [(st['param'].data_ptr(), st['param'].data_ptr() + 4 * st['param'].numel()) for st in opt.flat_state]
    for p in params:
        assert any(lo <= p.data_ptr() < hi for lo, hi in ranges) and p.data_ptr() % 256 == 0


def _close(a_net, b_net, rel=2e-6, what=''):
    for i, (a, b) in enumerate(zip(a_net.parameters(), b_net.parameters())):
        assert float((a - b).abs().max()) <= rel * max(1.0, float(b.abs().max())), (what, i, float((a - b).abs().max()))


@pytest.mark.parametrize('clip', ['active', 'inactive'])
def test_flat_adamw_vs_fp64_reference(vkn, clip):
    max_norm = 0.5 if clip == 'active' else 1e4
    net, tnet = _net(), _net()
    red, opt = _flat(net, max_norm)
    topt = _torch(tnet)
    ref = _Ref64(net)
    for step in range(6):
        grads = _grads(net, step)
        _step_flat(net, red, opt, grads)
        _step_torch(tnet, topt, grads, max_norm)
        norm64 = ref.step(grads, max_norm)
        assert (norm64 > max_norm) == (clip == 'active')
        assert abs(float(opt.last_grad_norm) - norm64) <= 1e-6 * norm64, step
        for i, (a, b, r) in enumerate(zip(net.parameters(), tnet.parameters(), ref.p)):
            err_flat, err_torch = float((a.detach().double() - r).abs().max()), float((b.detach().double() - r).abs().max())
            assert err_flat <= 2 * err_torch + 1e-7 * float(r.abs().max()), (step, i, err_flat, err_torch)
    _close(net, tnet, what='vs torch')
    _assert_views(net.parameters(), opt)


def test_flat_adamw_equals_torch_adamw_with_clip_and_backward(vkn):
    """Real backward passes through the reducer (hooks, finalize) against torch.optim.AdamW + clip_grad_norm_ on a deep copy."""
    net = _net()
    tnet = copy.deepcopy(net)
    red, opt = _flat(net, 0.3)
    topt = _torch(tnet)
    _assert_views(net.parameters(), opt)
    for a, b in zip(net.parameters(), tnet.parameters()):
        assert torch.equal(a, b)                               # moved into the flat buffers with their values unchanged
    for step in range(5):
        x = torch.randn(19, 37, device=DEV)
        red.zero_grad(set_to_none=True)
        topt.zero_grad(set_to_none=True)
        net(x).square().mean().backward()
        tnet(x).square().mean().backward()
        red.finalize()
        opt.step()
        tn = torch.nn.utils.clip_grad_norm_(tnet.parameters(), 0.3)
        topt.step()
        assert abs(float(opt.last_grad_norm) - float(tn)) <= 1e-5 * float(tn)
        _close(net, tnet, what=step)
    # the flat gradient keeps the reduced, UNCLIPPED gradient (clip_grad_norm_ scales .grad in place)
    assert float(torch.cat([p.grad.reshape(-1) for p in net.parameters()]).norm()) == pytest.approx(float(opt.last_grad_norm), rel=1e-5)
    _assert_views(net.parameters(), opt)


def test_unused_parameter_is_skipped_like_torch(vkn):
    net, tnet = _net(), _net()
    red, opt = _flat(net, 0.5)
    topt = _torch(tnet)
    for step in range(2):
        grads = _grads(net, step)
        _step_flat(net, red, opt, grads)
        _step_torch(tnet, topt, grads, 0.5)
    skip = (3, 5)                                              # LayerNorm bias, last weight: no gradient in this step
    before = [p.detach().clone() for p in net.parameters()]
    grads = _grads(net, 7)
    _step_flat(net, red, opt, grads, skip=skip)                # (their flat gradient slots still hold step 1's values)
    tn = _step_torch(tnet, topt, grads, 0.5, skip=skip)
    for i in skip:
        assert torch.equal(list(net.parameters())[i], before[i])
    assert float(opt.last_grad_norm) == pytest.approx(float(tn), rel=1e-5)
    assert float(opt.last_grad_norm) == pytest.approx(math.sqrt(sum(float((g.double() ** 2).sum()) for i, g in enumerate(grads)
                                                                    if i not in skip)), rel=1e-6)
    sd = opt.state_dict()
    for i in range(7):
        assert float(sd['state'][i]['step']) == (2 if i in skip else 3)
        assert float(sd['state'][i]['step']) == float(topt.state_dict()['state'][i]['step'])
    _close(net, tnet)
    # a parameter that never had a gradient has no state entry
    net2 = _net()
    red2, opt2 = _flat(net2, 0.5)
    _step_flat(net2, red2, opt2, _grads(net2, 0), skip=(6,))
    assert sorted(opt2.state_dict()['state']) == [0, 1, 2, 3, 4, 5]


def test_lr_scheduler_linear_warmup_drives_both_alike(vkn):
    """The shipped warm-up (warmup='linear', warmup_ratio=0.001) as a LambdaLR on both optimizers."""
    W, ratio = 4, 0.001

    def warm(it):
        return 1 - (1 - it / W) * (1 - ratio) if it < W else 1.0
    net, tnet = _net(), _net()
    red, opt = _flat(net, 0.5)
    topt = _torch(tnet)
    s1, s2 = torch.optim.lr_scheduler.LambdaLR(opt, warm), torch.optim.lr_scheduler.LambdaLR(topt, warm)
    for step in range(6):
        assert [g['lr'] for g in opt.param_groups] == [g['lr'] for g in topt.param_groups]
        grads = _grads(net, step)
        _step_flat(net, red, opt, grads)
        _step_torch(tnet, topt, grads, 0.5)
        s1.step()
        s2.step()
        _close(net, tnet, what=step)
    assert all('initial_lr' in g for g in opt.param_groups)


def _roundtrip(sd):
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


@pytest.mark.parametrize('direction', ['flat_to_torch', 'torch_to_flat'])
def test_checkpoint_moves_between_the_two_optimizers(vkn, direction):
    src_net = _net()
    if direction == 'flat_to_torch':
        red, src = _flat(src_net, 0.5)
        for step in range(3):
            _step_flat(src_net, red, src, _grads(src_net, step))
    else:
        src = _torch(src_net)
        for step in range(3):
            _step_torch(src_net, src, _grads(src_net, step), 0.5)
    sd = _roundtrip(src.state_dict())
    assert sorted(sd['state']) == list(range(7)) and all(float(s['step']) == 3.0 for s in sd['state'].values())
    dst_net = _net(seed=99)
    dst_net.load_state_dict(src_net.state_dict())
    if direction == 'flat_to_torch':
        dst = _torch(dst_net)
    else:
        red, dst = _flat(dst_net, 0.5)
    dst.load_state_dict(sd)
    assert [{k: v for k, v in g.items() if k != 'params'} for g in dst.param_groups] == \
           [{k: v for k, v in g.items() if k != 'params'} for g in src.param_groups]
    if direction == 'torch_to_flat':
        _assert_views(dst_net.parameters(), dst)
        flat_net, flat_red, flat_opt, t_net, t_opt = dst_net, red, dst, src_net, src
    else:
        flat_net, flat_red, flat_opt, t_net, t_opt = src_net, red, src, dst_net, dst
    for step in range(3, 6):
        grads = _grads(src_net, step)
        _step_flat(flat_net, flat_red, flat_opt, grads)
        _step_torch(t_net, t_opt, grads, 0.5)
        _close(flat_net, t_net, what=(direction, step))
    _assert_views(flat_net.parameters(), flat_opt)


def test_checkpoint_one_group_per_parameter(vkn):
    """mmcv's DefaultOptimizerConstructor makes one group per parameter: FlatAdamW -> checkpoint -> a fresh FlatAdamW and a torch
    AdamW, all three continuing alike."""
    spec = [([i], dict(lr=1e-3 * (1 + i % 3), betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0 if i % 2 else 0.05)) for i in range(7)]
    net = _net()
    red, opt = _flat(net, 0.5, spec=spec)
    for step in range(3):
        _step_flat(net, red, opt, _grads(net, step))
    sd = _roundtrip(opt.state_dict())
    assert len(sd['param_groups']) == 7
    net2, tnet = _net(seed=5), _net(seed=6)
    net2.load_state_dict(net.state_dict())
    tnet.load_state_dict(net.state_dict())
    red2, opt2 = _flat(net2, 0.5, spec=spec)
    opt2.load_state_dict(sd)
    topt = _torch(tnet, spec=spec)
    topt.load_state_dict(sd)
    _assert_views(net2.parameters(), opt2)
    for step in range(3, 6):
        grads = _grads(net, step)
        _step_flat(net, red, opt, grads)
        _step_flat(net2, red2, opt2, grads)
        _step_torch(tnet, topt, grads, 0.5)
        for a, b in zip(net.parameters(), net2.parameters()):
            assert torch.equal(a, b)
        _close(net, tnet, what=step)


def test_bitwise_deterministic(vkn):
    def run():
        net = _net()
        red, opt = _flat(net, 0.5)
        norms = []
        for step in range(4):
            _step_flat(net, red, opt, _grads(net, step))
            norms.append(opt.last_grad_norm.clone())
        return ([p.detach().clone() for p in net.parameters()], [st[k].clone() for st in opt.flat_state for k in ('exp_avg', 'exp_avg_sq')],
                torch.stack(norms))
    a, b = run(), run()
    for x, y in zip(a[0] + a[1] + [a[2]], b[0] + b[1] + [b[2]]):
        assert torch.equal(x, y)


@pytest.mark.parametrize('bad', ['inf', 'nan'])
def test_non_finite_gradient_pattern_matches_torch(vkn, bad):
    net, tnet = _net(), _net()
    red, opt = _flat(net, 0.5)
    topt = _torch(tnet)
    grads = _grads(net, 0)
    _step_flat(net, red, opt, grads)
    _step_torch(tnet, topt, grads, 0.5)
    grads = _grads(net, 1)
    grads[0][3, 5] = float(bad)
    _step_flat(net, red, opt, grads)
    tn = _step_torch(tnet, topt, grads, 0.5)
    assert (math.isinf(float(opt.last_grad_norm)) and math.isinf(float(tn))) if bad == 'inf' else \
        (math.isnan(float(opt.last_grad_norm)) and math.isnan(float(tn)))
    for a, b in zip(net.parameters(), tnet.parameters()):
        assert torch.equal(torch.isfinite(a), torch.isfinite(b))
        ok = torch.isfinite(b)
        if bool(ok.any()):
            assert float((a[ok] - b[ok]).abs().max()) <= 2e-6 * max(1.0, float(b[ok].abs().max()))


def test_step_never_synchronises_with_the_host(vkn):
    net = _net()
    red, opt = _flat(net, 0.5)
    sched = torch.optim.lr_scheduler.LambdaLR(opt, lambda it: 0.5 + 0.1 * it)
    for step in range(3):
        red.zero_grad(set_to_none=True)
        for i, (p, g) in enumerate(zip(net.parameters(), _grads(net, step))):
            if not (step == 1 and i == 2):                     # the active bytes change too
                p.grad = g
        red.finalize()
        torch.cuda.synchronize()
        torch.cuda.set_sync_debug_mode('error')
        try:
            opt.step()                                         # rows and active bytes re-uploaded (the LR changed every step)
        finally:
            torch.cuda.set_sync_debug_mode(0)
        sched.step()
    assert math.isfinite(float(opt.last_grad_norm))


def test_real_video_head_three_training_steps(vkn):
    """train_video_c256 (C = 256, N = 117, ffn link), forward_train_with_previous under the default policy: FlatAdamW(lr 1e-4,
    weight_decay 0.05, max_norm 1) — the shipped schedule — against torch's clip + AdamW on a cloned parameter set fed the same
    gradients; the chain kernels keep reading the moved parameter views."""
    from test_gpu_train import _train_case
    g, case, head, (x, pf, mp, prev), (gt_masks, gt_labels, gt_sem_seg, gt_sem_cls) = _train_case(vkn, 'train_video_c256')
    metas = [dict() for _ in range(case['B'])]
    d = _dist()
    red = d.BucketedGradAllReducer(head)
    opt = d.FlatAdamW(red, lr=1e-4, weight_decay=0.05, max_norm=1.0)
    params = list(opt.param_groups[0]['params'])
    clones = [torch.nn.Parameter(p.detach().clone()) for p in params]
    topt = torch.optim.AdamW(clones, lr=1e-4, weight_decay=0.05)
    for step in range(3):
        red.zero_grad(set_to_none=True)
        out = head.forward_train_with_previous(x.to(DEV), pf.to(DEV), mp.to(DEV), None, metas, gt_masks, gt_labels,
                                               gt_sem_seg=gt_sem_seg, gt_sem_cls=gt_sem_cls, previous_obj_feats=prev.to(DEV))
        losses = [v for k, v in out[0].items() if 'loss' in k]
        assert all(math.isfinite(float(v)) for v in losses), step
        (sum(losses) + 0.01 * (out[5] ** 2).sum()).backward()
        red.finalize()
        for c, p in zip(clones, params):
            c.grad = None if p.grad is None else p.grad.clone()
        tn = torch.nn.utils.clip_grad_norm_([c for c in clones if c.grad is not None], 1.0)
        topt.step()
        opt.step()
        assert float(opt.last_grad_norm) == pytest.approx(float(tn), rel=1e-5)
        for i, (p, c) in enumerate(zip(params, clones)):
            assert float((p - c).abs().max()) <= 2e-6 * max(1.0, float(c.abs().max())), (step, i)
    _assert_views(params, opt)
