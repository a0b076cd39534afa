"""Frame-sharded data parallelism for a clip (one process per GPU, `torch.distributed`; backend "nccl" = RCCL on ROCm).

Masks, class scores and kernels of frame t do not depend on frame t-1; only the tracking embedding of
the last stage does (knet/video/kernel_iter_head.py:544-546, knet/video/kernel_update_head.py:394-415).  So the frames of a clip
are split into contiguous blocks, every rank runs the whole head on its block with NO collective on the mask path, and a single
small exchange hands each rank the final kernels of the frame just before its block (120 KB for N=117, C=256).
"""
import torch
import torch.distributed as dist


def shard_bounds(num_frames: int, world: int, rank: int):
    """Contiguous block [begin, end) of a clip's frames owned by `rank` (sizes differ by at most 1)."""
    return (num_frames * rank) // world, (num_frames * (rank + 1)) // world


def exchange(send, recv, send_to=None, recv_from=None, group=None):
    """One batched point-to-point step: `send` -> group rank `send_to`, `recv` <- group rank `recv_from` (either may be None).
    P2POp peers are GLOBAL ranks: group-local ranks are translated (identical for the default group).  A rank may name itself
    (RCCL pairs a send and a receive posted in one group): that is how a 1-GPU box exercises this path."""
    peer = (lambda r: dist.get_global_rank(group, r)) if group is not None else (lambda r: r)
    ops = []
    if send_to is not None:
        ops.append(dist.P2POp(dist.isend, send, peer(send_to), group))
    if recv_from is not None:
        ops.append(dist.P2POp(dist.irecv, recv, peer(recv_from), group))
    for req in (dist.batch_isend_irecv(ops) if ops else []):
        req.wait()


def neighbour_last_kernels(block_kernels: torch.Tensor, group=None):
    """Every rank owns >= 1 frame: hand this rank's LAST frame's kernels [N, C] to rank + 1 and return the previous rank's
    ([1, N, C]; None on rank 0 or without a process group).  ONE point-to-point send / receive (120 KB at N = 117, C = 256) —
    xGMI is point-to-point, a single send rides one link, no ring, no host synchronisation."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    if world <= 1:
        return None
    N, C = block_kernels.shape[1:]
    last = block_kernels[-1].contiguous()
    recv = torch.empty_like(last)
    exchange(last, recv, rank + 1 if rank + 1 < world else None, rank - 1 if rank > 0 else None, group)
    return recv.reshape(1, N, C) if rank > 0 else None


def previous_kernels_for_block(block_kernels: torch.Tensor, first_previous=None, group=None, all_nonempty=False):
    """`block_kernels` [T_r, N, C] = final kernels of this rank's frames.  Returns prev [T_r, N, C] with
    prev[i] = kernels of the frame BEFORE frame i of the block: the previous rank's last frame for i = 0
    (rank 0: `first_previous` [1,N,C], or its own frame 0 when the clip starts the video), own frame i-1 otherwise.
    `all_nonempty=True` (every rank is known to own frames, e.g. an even split — what bench.py and training use): ONE
    point-to-point send to rank + 1 / receive from rank - 1, no host synchronisation.  Otherwise (uneven splits, ranks without
    frames): one all_gather of [N, C] + a has-frames flag per rank and one host read of the flags; ranks with an empty block are
    skipped by their successor."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    T = block_kernels.shape[0]
    N, C = block_kernels.shape[1:]
    if world > 1 and all_nonempty:
        p0 = neighbour_last_kernels(block_kernels, group)
    elif world > 1:
        last = block_kernels[-1].contiguous() if T > 0 else block_kernels.new_zeros(N, C)
        has = torch.tensor([1.0 if T > 0 else 0.0], device=block_kernels.device)
        payload = torch.cat([last.reshape(-1), has])             # one message per rank: [N*C kernels | has-frames flag]
        got = [torch.empty_like(payload) for _ in range(world)]
        dist.all_gather(got, payload, group=group)
        p0 = None
        flags = torch.stack([g_[-1] for g_ in got]).cpu()   # ONE device -> host read for all flags (uneven splits only)
        for r in range(rank - 1, -1, -1):        # nearest predecessor that owns at least one frame
            if float(flags[r]) > 0:
                p0 = got[r][:-1].reshape(1, N, C)
                break
    else:
        p0 = None
    if p0 is None:
        p0 = first_previous if first_previous is not None else block_kernels[:1]
    if T == 0:
        return block_kernels
    return torch.cat([p0.reshape(1, N, C), block_kernels[:-1]], dim=0)


def linked_block_forward(run_phase, first_previous, group=None):
    """One rank's share of a clip for the heads whose LAST stage rewrites its incoming kernels from the previous frame's final
    kernels (`previous_link = "update_dynamic_cov" | "link_atten"`, knet/video/kernel_update_head.py:324-372,
    knet/video/kernel_iter_head.py:454-456).  There the masks of frame t depend on frame t-1 — through [N x C]-sized state only,
    and only in the last stage — so a rank cannot simply run its block and patch frame 0 afterwards (`neighbour_last_kernels`
    does that for the heads without previous_link).  The block runs in three phases around ONE receive and ONE send:

        A  `run_phase('A', None)`     stages 0 .. S-2 and the last stage's gather for all frames of the block: no cross-frame input,
                                      every rank runs it at once (the x-streaming work);
           receive the final kernels of the frame before the block from rank - 1 (rank 0: `first_previous`);
        B  `run_phase('B', prev)`     the last stage's [N x C] chains, frame by frame, frame 0 linked to `prev` -> returns the
                                      block's final kernels [T_r, N, C];
           send the LAST frame's kernels to rank + 1 — before the HBM-bound tail, so the next rank's chains start while this
           rank decodes and upsamples;
        C  `run_phase('C', prev)`     the batched last decode, the upsample, the tracking link -> the block's outputs.

    The last-stage chains of a clip therefore serialise across the ranks (~0.13 ms per frame at one frame per launch) while
    phases A and C of all ranks overlap; the cross-rank traffic is one 120 KB point-to-point message per rank boundary.
    `run_phase(name, prev)` is `VideoKernelIterHead.linked_block_phases(...)` on the GPU, any callable with that contract in tests.
    Every rank must own at least one frame.  -> what phase C returns."""
    world = dist.get_world_size(group) if dist.is_initialized() else 1
    rank = dist.get_rank(group) if dist.is_initialized() else 0
    run_phase('A', None)
    prev = first_previous
    if world > 1 and rank > 0:
        prev = torch.empty_like(first_previous)
        exchange(None, prev, None, rank - 1, group)
    kernels = run_phase('B', prev)
    if world > 1 and rank + 1 < world:
        exchange(kernels[-1:].contiguous().reshape(first_previous.shape), None, rank + 1, None, group)
    return run_phase('C', prev)


class BucketedGradAllReducer:
    """Data-parallel gradient averaging for the head (BASELINE cfg3: frames of a clip sharded over the GPUs of a node, RCCL
    all-reduce over xGMI; the reference gets this from mmcv's `MMDistributedDataParallel`, external/train.py:53-61).

    Parameters are grouped into buckets (default: one per `mask_head.{s}` stage + one for the rest).  Every parameter's `.grad` is
    a VIEW into its bucket's flat fp32 buffer, so a bucket is reduced in place with ONE collective and nothing is copied.  A
    post-accumulate-grad hook marks the bucket's parameters as backward produces them; the bucket's `all_reduce(async_op=True)`
    is launched the moment the last gradient it EXPECTS has landed — backward runs the stages in reverse, so stage S-1's 13 MB
    travel while stages S-2 .. 0 are still being differentiated.  `finalize()` launches what is left, waits, and divides by the
    world size.  xGMI is point-to-point (7 links x ~153 GB/s per GPU): a few large buckets keep every link busy with long
    messages instead of hundreds of per-tensor rings.  With world_size 1 everything degenerates to plain local gradients.

    Contract (the DDP one):
    * one synchronised backward per step: `zero_grad -> backward -> finalize -> optimizer.step`.  Gradient accumulation: run the
      earlier backward passes under `with reducer.no_sync():` — nothing is launched there, gradients just add up in the buckets.
      A second backward outside `no_sync()` before `finalize()` would add to a buffer that is already being reduced: it raises.
    * ANY `zero_grad` is fine.  `reducer.zero_grad()` zeroes the flat buffers: backward then ADDS every gradient into its view
      (one `add_` launch per parameter).  `reducer.zero_grad(set_to_none=True)` — or torch's default `optimizer.zero_grad()` /
      `module.zero_grad()` — DROPS the `.grad` views instead: autograd then hands each parameter the gradient tensor itself (no
      kernel), the hook notes it, and the moment a bucket is complete its gradients are copied into the flat buffer by ONE
      multi-tensor launch (`torch._foreach_copy_`) and the views are re-attached, so the collective always reduces the real
      gradients.  This is the cheap mode for a step with one backward (~150 launches and dispatcher calls less per step of the
      K-Net head); the gradient tensors may alias a captured graph's static buffers (`enable_chain_graphs`), which is fine because
      they are consumed before the next replay.  Under `no_sync()` a dropped view is filled and re-attached at once.
    * which parameters take part in backward (the video head builds its link modules in every stage but uses the last stage's
      only), and how often each one reports per step, is learned during the first synchronised step (reduced in `finalize()`):
      from the second step on a bucket is launched the moment its expected reports are in, so stage buckets with unused members
      also overlap with backward.  When the set of used parameters changes
      (e.g. switching between `forward_train` and `forward_train_with_previous`), call `reset_usage()`; a gradient arriving in a
      bucket that is already in flight raises instead of being silently lost."""

    def __init__(self, module, bucket_of=None, group=None, force_collectives=False):
        import re
        self.group = group
        self.world = dist.get_world_size(group) if (dist.is_available() and dist.is_initialized()) else 1
        # force_collectives: issue the all-reduces even in a ONE-rank group (a 1-GPU box still exercises the RCCL path)
        self._coll = self.world > 1 or (force_collectives and dist.is_available() and dist.is_initialized())
        self._sync = True
        if bucket_of is None:
            def bucket_of(name):
                m = re.search(r'mask_head\.(\d+)\.', name)
                return f'stage{m.group(1)}' if m else 'rest'
        groups = {}
        seen = set()
        self._hook_of = {}
        for name, p in module.named_parameters():
            if not p.requires_grad or id(p) in seen:        # shared parameters (recursive heads) are bucketed once
                continue
            seen.add(id(p))
            groups.setdefault((bucket_of(name), p.device, p.dtype), []).append(p)
        self.buckets = []
        for (key, dev, dt), params in groups.items():
            # every slot starts on a 256-byte boundary (the padding stays zero): a view is then as aligned as a tensor of its own —
            # the kernels' 16-byte accesses, and `FlatSGD`'s parameter views, which the chain kernels read in place
            flat = torch.zeros(sum(self._slot(p.numel()) for p in params), device=dev, dtype=dt)
            b = dict(key=key, flat=flat, params=params, views=[], fired={}, nfired=0, expect=None, expect_total=0, handle=None, grew=False, pending=set())
            off = 0
            for i, p in enumerate(params):
                v = flat[off:off + p.numel()].view_as(p)
                b['views'].append(v)
                p.grad = v
                off += self._slot(p.numel())
                hook = self._make_hook(b, i)
                self._hook_of[id(p)] = hook
                p.register_post_accumulate_grad_hook(hook)
            self.buckets.append(b)
        # heads whose captured chain graphs deliver parameter gradients in bulk (KernelUpdateHead.enable_chain_graphs) report here
        for m in module.modules():
            if hasattr(m, 'on_param_grads'):
                m.on_param_grads = self.params_ready

    @staticmethod
    def _slot(n):
        return (n + 63) // 64 * 64

    def params_ready(self, params):
        """The gradients of `params` have been written to their `.grad` outside autograd's accumulation nodes (a captured backward
        graph): the same bookkeeping as the post-accumulate hook."""
        for p in params:
            hook = self._hook_of.get(id(p))
            if hook is not None:
                hook(p)

    @staticmethod
    def _flush(b):
        """Gradients that arrived as tensors of their own (dropped views): into the flat buffer with one multi-tensor copy."""
        if b['pending']:
            idx = sorted(b['pending'])
            torch._foreach_copy_([b['views'][i] for i in idx], [b['params'][i].grad for i in idx])
            for i in idx:
                b['params'][i].grad = b['views'][i]
            b['pending'] = set()

    def _launch(self, b):
        self._flush(b)
        # members without a gradient in this step (`zero_grad(set_to_none=True)` and no use): their slots of the flat buffer still
        # hold a previous step's averaged gradient — they must contribute ZERO to the sum, as DDP's unused parameters do.
        # Parameter usage is expected to be the same on every rank (the launch points are learned per rank: rank-divergent usage
        # would order the collectives differently); with identical usage this zeroing is what keeps the slot clean everywhere.
        stale = [v for p, v in zip(b['params'], b['views']) if p.grad is None]
        if stale:
            torch._foreach_zero_(stale)
        b['handle'] = dist.all_reduce(b['flat'], op=dist.ReduceOp.SUM, group=self.group, async_op=True)

    def _make_hook(self, b, i):
        def hook(p):
            view = b['views'][i]
            g = p.grad
            if g is not view and (g is None or g.data_ptr() != view.data_ptr()):
                # `zero_grad(set_to_none=True)` or an external `p.grad = ...` dropped the view
                if g is not None and self._sync:
                    b['pending'].add(i)              # stays `p.grad` (a second use of the parameter adds into it) until the bucket is flushed
                else:
                    if g is not None:
                        view.copy_(g)
                    p.grad = view
            if b['handle'] is not None:
                raise RuntimeError(f"BucketedGradAllReducer: a gradient arrived in bucket '{b['key']}' while its all-reduce is in "
                                   'flight (a second backward before finalize() — wrap the earlier ones in no_sync() — or the set '
                                   'of used parameters changed — call reset_usage())')
            if not self._sync:
                return
            # a parameter may report more than once per backward (a captured chain delivers its share in bulk, an eager use of the same
            # parameter reports through autograd later): the bucket is complete when every member has reported as often as it did
            # in the steps seen so far.  The first synchronised step only learns (everything is reduced in finalize()).
            n = b['fired'][i] = b['fired'].get(i, 0) + 1
            b['nfired'] += 1
            exp = b['expect']
            if exp is None:
                return
            if n > exp.get(i, 0):
                b['grew'] = True                                  # more than we expected: reduce this bucket in finalize()
            if self._coll and not b['grew'] and b['nfired'] == b['expect_total']:
                self._launch(b)
        return hook

    class _NoSync:
        def __init__(self, owner):
            self.owner = owner

        def __enter__(self):
            self.prev, self.owner._sync = self.owner._sync, False

        def __exit__(self, *exc):
            self.owner._sync = self.prev
            return False

    def no_sync(self):
        """Context manager for the non-final backward passes of a gradient-accumulation step (DDP's `no_sync`)."""
        return self._NoSync(self)

    def reset_usage(self):
        """Forget which parameters take part in backward (re-learned during the next synchronised step)."""
        for b in self.buckets:
            b['expect'] = None

    def zero_grad(self, set_to_none=False):
        """Re-arm the hooks and either zero the flat buffers and (re-)attach the parameters' `.grad` views (gradients are added
        into the buckets), or — `set_to_none=True` — drop the views (gradients arrive as tensors, one batched copy per bucket)."""
        for b in self.buckets:
            if set_to_none:
                for p in b['params']:
                    p.grad = None
            else:
                b['flat'].zero_()
                for p, v in zip(b['params'], b['views']):
                    if p.grad is not v:
                        p.grad = v
            b['fired'], b['nfired'], b['handle'], b['grew'], b['pending'] = {}, 0, None, False, set()

    def finalize(self):
        """Launch the collectives of the buckets that are not in flight yet (first step, unused members, accumulation), wait for
        all of them, then average.  Call after the step's last `backward()` and before `optimizer.step()`."""
        for b in self.buckets:
            if b['handle'] is None:
                self._flush(b)
            late = []
            for p, v in zip(b['params'], b['views']):
                # `p.grad is None`: the parameter took no part in this step after a set_to_none zero_grad — it stays None (the
                # optimizer skips it; its slot of the flat buffer is zeroed before the reduction, see _launch)
                if p.grad is not None and p.grad is not v and p.grad.data_ptr() != v.data_ptr():
                    if b['handle'] is not None:   # a gradient assigned behind the hooks' back
                        raise RuntimeError(f"BucketedGradAllReducer: bucket '{b['key']}' was reduced without a member's gradient")
                    late.append((p, v))
            if late:
                torch._foreach_copy_([v for _, v in late], [p.grad for p, _ in late])
                for p, v in late:
                    p.grad = v
        if self._coll:
            for b in self.buckets:
                if b['handle'] is None:
                    self._launch(b)
            for b in self.buckets:
                b['handle'].wait()
                b['flat'].div_(self.world)
        for b in self.buckets:
            if self._sync and b['fired']:
                exp = b['expect'] if b['expect'] is not None else {}
                for i, n in b['fired'].items():
                    exp[i] = max(exp.get(i, 0), n)
                b['expect'], b['expect_total'] = exp, sum(exp.values())
            b['fired'], b['nfired'], b['handle'], b['grew'] = {}, 0, None, False


def _flatten_params(reducer, who):
    """Move the parameters of every bucket of `reducer` into one flat fp32 buffer laid out like the bucket's gradient buffer (each
    `p.data` becomes a view of it on the same 256-byte slot boundaries, values unchanged, padding zero) -> the flat buffers, in bucket
    order.  The optimizers below run on the library's kernels only: anything but fp32 CUDA parameters raises (no CPU fallback)."""
    for b in reducer.buckets:
        if not b['flat'].is_cuda or b['flat'].dtype != torch.float32:
            raise RuntimeError(f'{who} runs on the GPU kernels: fp32 CUDA parameters only (no CPU fallback)')
    pflats = []
    for b in reducer.buckets:
        pflat = torch.zeros_like(b['flat'])
        off = 0
        for p in b['params']:
            n = p.numel()
            pflat[off:off + n].copy_(p.detach().reshape(-1))
            p.data = pflat[off:off + n].view_as(p)
            off += reducer._slot(n)
        pflats.append(pflat)
    return pflats


class FlatSGD:
    """SGD with momentum over the FLAT buckets of a `BucketedGradAllReducer` (torch.optim.SGD's rule, dampening 0, no nesterov): the
    parameters of a bucket are moved into one flat buffer laid out like the bucket's gradient buffer (every `p.data` becomes a view of
    it — values unchanged), and a step is ONE pass per bucket over (parameters, gradients, momentum) on the library's kernel
    (`vkn_sgd_momentum_f32`) instead of torch's multi-tensor walk over ~300 tensors (0.54 ms -> 0.05 ms per step of the cfg3 head).
    Call order: `reducer.zero_grad -> backward -> reducer.finalize -> opt.step`.
    A parameter without a gradient in a step counts as a ZERO gradient (its momentum still decays and is applied) — what
    DistributedDataParallel + SGD do with unused parameters; torch.optim.SGD alone would skip it.  `reducer_divides=True` (default):
    `finalize()` has already divided by the world size."""

    def __init__(self, reducer, lr, momentum=0.0, weight_decay=0.0, nesterov=False, dampening=0.0):
        if nesterov or dampening:
            raise NotImplementedError('FlatSGD: nesterov / dampening are not provided')
        self.reducer, self.lr, self.momentum, self.weight_decay = reducer, float(lr), float(momentum), float(weight_decay)
        self.state = [dict(param=pflat, mom=torch.zeros_like(b['flat'])) for b, pflat in zip(reducer.buckets, _flatten_params(reducer, 'FlatSGD'))]

    def zero_grad(self, set_to_none=True):
        self.reducer.zero_grad(set_to_none=set_to_none)

    @torch.no_grad()
    def step(self):
        from . import _lib
        L = _lib.lib()
        for b, st in zip(self.reducer.buckets, self.state):
            # after finalize() every gradient that exists is a view of the flat buffer; a member without one contributes zero
            stale = [v for p, v in zip(b['params'], b['views']) if p.grad is None]
            if stale:
                torch._foreach_zero_(stale)
            with torch.cuda.device(b['flat'].device):
                _lib.check(L.vkn_sgd_momentum_f32(st['param'].data_ptr(), b['flat'].data_ptr(), st['mom'].data_ptr(), b['flat'].numel(),
                                                  self.lr, self.momentum, self.weight_decay, 1.0,
                                                  torch.cuda.current_stream(b['flat'].device).cuda_stream))


class FlatAdamW(torch.optim.Optimizer):
    """AdamW behind a global L2 gradient clip over the FLAT buckets of a `BucketedGradAllReducer`: the optimizer of every shipped
    schedule (configs/det/_base_/schedules/schedule_1x.py:1-8: AdamW lr 1e-4, weight_decay 0.05, grad_clip max_norm 1, norm_type 2),
    which the reference runs as mmcv's OptimizerHook — `clip_grad_norm_(params, max_norm)` then `torch.optim.AdamW.step()` (external/
    train.py:67, 98-104).  A step is ONE library call per device (`vkn_adamw_flat_f32`: squared-norm partials, a one-workgroup finish,
    the update) over a work-item table built here once; it never reads anything back to the host.

    * `params`: None (one group of every reducer parameter), an iterable of parameters, or torch-style group dicts (mmcv's
      DefaultOptimizerConstructor makes one group per parameter).  Every listed parameter must belong to the reducer; reducer
      parameters in no group are never touched.  torch.optim.lr_scheduler.* and mmcv's LR hooks drive `group['lr']` as usual.
    * Layout: as FlatSGD, every reducer parameter becomes a view of one flat fp32 buffer per bucket (values unchanged), so the chain
      kernels keep reading aligned views; exp_avg / exp_avg_sq live in two more flat buffers per bucket (`flat_state`).
    * A parameter whose `.grad is None` after `reducer.finalize()` is skipped as torch.optim.AdamW skips it: no decay, no moment
      update, no step, no part in the norm (its flat gradient slot may still hold an older step's values — only `.grad` decides).
    * `max_norm` (None: no clip): the norm is taken over the parameters of this optimizer only.  After `step()`, `last_grad_norm` is
      the fp32 device scalar `clip_grad_norm_` would have returned (what mmcv logs as `grad_norm`).  Unlike clip_grad_norm_, the flat
      gradient is NOT scaled in place: after the step it still holds the reduced, unclipped gradient.
    * `state_dict()` / `load_state_dict()` use torch.optim.AdamW's format (per parameter `step` as a 0-dim float32 tensor, `exp_avg`,
      `exp_avg_sq`; torch's group keys), so checkpoints move between the two optimizers in both directions.  `state_dict()` reads the
      step counters back to the host (checkpoint time, not every step).
    Call order: `reducer.zero_grad -> backward -> reducer.finalize -> opt.step`.  fp32 parameters on ONE CUDA device; AMSGrad,
    `maximize` and norms other than L2 are not provided (they raise)."""

    CHUNK = 8192        # elements per work item (a workgroup of the norm and update kernels): one 16-byte load per lane and array, x8

    def __init__(self, reducer, params=None, lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, max_norm=None, norm_type=2.0,
                 amsgrad=False, *, maximize=False, foreach=None, capturable=False, differentiable=False, fused=None):
        if amsgrad or maximize or differentiable:
            raise NotImplementedError('FlatAdamW: amsgrad / maximize / differentiable are not provided')
        if float(norm_type) != 2.0:
            raise NotImplementedError(f'FlatAdamW: only the L2 gradient norm is provided (norm_type={norm_type})')
        if max_norm is not None and not float(max_norm) > 0:
            raise ValueError(f'FlatAdamW: max_norm must be positive or None, got {max_norm}')
        self._frozen = False
        self.reducer = reducer
        self.max_norm = None if max_norm is None else float(max_norm)
        self.norm_type = 2.0
        self.last_grad_norm = None
        if params is None:
            params = [p for b in reducer.buckets for p in b['params']]
        defaults = dict(lr=lr, betas=tuple(betas), eps=eps, weight_decay=weight_decay, amsgrad=False, maximize=False, foreach=foreach,
                        capturable=capturable, differentiable=False, fused=fused, decoupled_weight_decay=True)
        super().__init__(params, defaults)
        where = {}
        for bi, b in enumerate(reducer.buckets):
            off = 0
            for i, p in enumerate(b['params']):
                where[id(p)] = (bi, i, off)
                off += reducer._slot(p.numel())
        for gi, g in enumerate(self.param_groups):
            self._check_group(g)
            for k, p in enumerate(g['params']):
                if id(p) not in where:
                    names = g.get('param_names')
                    nm = f"'{names[k]}' " if names else ''
                    raise ValueError(f"FlatAdamW: param_groups[{gi}]['params'][{k}] {nm}(shape {tuple(p.shape)}) is not a parameter of "
                                     'the reducer')
        self._params = [p for g in self.param_groups for p in g['params']]
        used = sorted({where[id(p)][0] for p in self._params})
        devs = {reducer.buckets[bi]['flat'].device for bi in used}
        if len(devs) > 1:
            raise NotImplementedError('FlatAdamW: the parameters span several devices (one process per GPU, as DDP)')
        pflats = _flatten_params(reducer, 'FlatAdamW')
        self.flat_state = [dict(param=pf, exp_avg=torch.zeros_like(pf), exp_avg_sq=torch.zeros_like(pf)) for pf in pflats]
        dev = next(iter(devs))
        self._device = dev
        from . import _lib
        items, self._mv, self._gviews = [], [], []
        gi_of = [gi for gi, g in enumerate(self.param_groups) for _ in g['params']]
        for pi, p in enumerate(self._params):
            bi, i, off = where[id(p)]
            b, st = reducer.buckets[bi], self.flat_state[bi]
            n = p.numel()
            self._mv.append((st['exp_avg'][off:off + n].view_as(p), st['exp_avg_sq'][off:off + n].view_as(p)))
            self._gviews.append(b['views'][i])
            n4 = (n + 3) // 4 * 4            # inside the 64-element slot: the zero padding stays exactly zero under AdamW
            for c0 in range(0, n4, self.CHUNK):
                o = 4 * (off + c0)
                items.append(_lib.VknAdamwItem(st['param'].data_ptr() + o, b['flat'].data_ptr() + o, st['exp_avg'].data_ptr() + o,
                                               st['exp_avg_sq'].data_ptr() + o, min(self.CHUNK, n4 - c0), pi, gi_of[pi], 0))
        arr = (_lib.VknAdamwItem * len(items))(*items)
        self._items = torch.frombuffer(bytearray(arr), dtype=torch.uint8).to(dev)
        self._n_items = len(items)
        self._steps = torch.zeros(len(self._params), dtype=torch.int32, device=dev)
        # group rows (fp64 [n_groups][5]) and active bytes ([n_params]) in ONE device buffer, rewritten from pinned memory on change
        self._rows_bytes = 8 * _lib.ADAMW_GROUP_ROW * len(self.param_groups)
        self._hyper = torch.zeros(self._rows_bytes + len(self._params), dtype=torch.uint8, device=dev)
        self._staging = []              # [pinned buffer, event of its last copy]: a buffer is refilled only once its copy is done
        self._uploaded = None
        nb = _lib.lib().vkn_adamw_workspace_bytes(self._n_items, len(self._params), len(self.param_groups))
        self._ws = torch.zeros(nb, dtype=torch.uint8, device=dev)
        self._frozen = True

    @staticmethod
    def _check_group(g):
        if g.get('amsgrad') or g.get('maximize') or g.get('differentiable'):
            raise NotImplementedError('FlatAdamW: amsgrad / maximize / differentiable are not provided')
        b1, b2 = g['betas']
        if not (0.0 <= float(g['lr']) and 0.0 <= float(g['eps']) and 0.0 <= float(g['weight_decay']) and 0.0 <= b1 < 1.0 and 0.0 <= b2 < 1.0):
            raise ValueError(f"FlatAdamW: invalid hyper-parameters lr={g['lr']} betas={g['betas']} eps={g['eps']} "
                             f"weight_decay={g['weight_decay']}")

    def add_param_group(self, param_group):
        if self._frozen:
            raise NotImplementedError('FlatAdamW: the parameter groups are fixed at construction (the work-item table is built once)')
        super().add_param_group(param_group)

    def zero_grad(self, set_to_none=True):
        self.reducer.zero_grad(set_to_none=set_to_none)

    def _active(self):
        act = []
        for p, v in zip(self._params, self._gviews):
            g = p.grad
            if g is not None and g is not v and g.data_ptr() != v.data_ptr():
                raise RuntimeError('FlatAdamW: a gradient is not in its bucket — call reducer.finalize() before step()')
            act.append(g is not None)
        return act

    def _upload(self, stream):
        """Group rows + active bytes to the device when they changed: a non-blocking copy from a pinned buffer that no copy in flight
        still reads (an event per buffer; a new buffer when every one is busy) — no host synchronisation."""
        import numpy as np
        rows = [(float(g['lr']), float(g['weight_decay']), float(g['betas'][0]), float(g['betas'][1]), float(g['eps'])) for g in self.param_groups]
        act = self._active()
        key = (rows, act)
        if key == self._uploaded:
            return
        slot = next((s for s in self._staging if s[1].query()), None)
        if slot is None:
            slot = [torch.empty(self._hyper.numel(), dtype=torch.uint8, pin_memory=True), torch.cuda.Event()]
            self._staging.append(slot)
        h = slot[0].numpy()
        h[:self._rows_bytes] = np.asarray(rows, dtype=np.float64).reshape(-1).view(np.uint8)
        h[self._rows_bytes:] = np.asarray(act, dtype=np.uint8)
        self._hyper.copy_(slot[0], non_blocking=True)
        slot[1].record(stream)
        self._uploaded = key

    @torch.no_grad()
    def step(self, closure=None):
        loss = None
        if closure is not None:
            with torch.enable_grad():
                loss = closure()
        from . import _lib
        L = _lib.lib()
        dev = self._device
        with torch.cuda.device(dev):
            stream = torch.cuda.current_stream(dev)
            self._upload(stream)
            norm = torch.empty((), dtype=torch.float32, device=dev) if self.max_norm is not None else None
            _lib.check(L.vkn_adamw_flat_f32(self._items.data_ptr(), self._n_items, len(self._params), self._hyper.data_ptr(),
                                            len(self.param_groups), self._steps.data_ptr(), self._hyper.data_ptr() + self._rows_bytes,
                                            self.max_norm or 0.0, None if norm is None else norm.data_ptr(), None,
                                            self._ws.data_ptr(), self._ws.numel(), stream.cuda_stream))
        self.last_grad_norm = norm
        return loss

    def state_dict(self):
        steps = self._steps.cpu().tolist()
        state = {}
        for i, (m, v) in enumerate(self._mv):
            if steps[i] > 0:            # a parameter that never had a gradient has no state (as in torch)
                state[i] = {'step': torch.tensor(float(steps[i]), dtype=torch.float32), 'exp_avg': m.clone(), 'exp_avg_sq': v.clone()}
        groups, start = [], 0
        for g in self.param_groups:
            d = {k: v for k, v in g.items() if k != 'params'}
            d['params'] = list(range(start, start + len(g['params'])))
            start += len(g['params'])
            groups.append(d)
        return {'state': state, 'param_groups': groups}

    def load_state_dict(self, state_dict):
        saved = state_dict['param_groups']
        if len(saved) != len(self.param_groups) or any(len(s['params']) != len(g['params']) for s, g in zip(saved, self.param_groups)):
            raise ValueError('FlatAdamW.load_state_dict: the saved parameter groups do not match this optimizer\'s')
        index = {}
        for s, g, start in zip(saved, self.param_groups, _prefix_sums([len(g['params']) for g in self.param_groups])):
            self._check_group(dict(s, params=None))
            for k, saved_id in enumerate(s['params']):
                index[saved_id] = start + k
        steps = torch.zeros(len(self._params), dtype=torch.int32)
        with torch.no_grad():
            for st in self.flat_state:
                st['exp_avg'].zero_()
                st['exp_avg_sq'].zero_()
            for saved_id, st in state_dict['state'].items():
                i = index[saved_id]
                m, v = self._mv[i]
                m.copy_(st['exp_avg'])
                v.copy_(st['exp_avg_sq'])
                steps[i] = int(round(float(st['step'])))
            self._steps.copy_(steps)
        for s, g in zip(saved, self.param_groups):
            ps = g['params']
            g.clear()
            g.update({k: v for k, v in s.items() if k != 'params'})
            g['params'] = ps
        self._uploaded = None


def _prefix_sums(lens):
    out, s = [], 0
    for n in lens:
        out.append(s)
        s += n
    return out
