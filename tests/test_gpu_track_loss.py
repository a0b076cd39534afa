"""The fused tracking loss (csrc/vkn_trackloss.hip, include/vkn_track_train.h) on the GPU, through the C ABI: values against the
reference's goldens and the float64 restatement of tests/track_loss_ref.py, the full-row form bit-identical to the compact one,
gradients held to a bound measured on the package's own fp32 host path, the decision edges of the hard-negative mining, the
envelope, the status word, stream capture (= no host synchronisation), determinism, and the Python layers above it.

Measured 2026-10-18 on an MI355X (docs/LAB_NOTEBOOK.md, "Fused tracking loss", has every case and gout): relative max-norm error of
d_key / d_ref against float64 at gout = (1, 1), host path (fp32, CPU) vs kernel — emb_cfg 6.4e-6 / 2.4e-6 vs 1.4e-5 / 4.8e-6,
emb_one 2.4e-7 / 1.3e-7 vs 3.3e-7 / 1.8e-7, emb_temp 4.3e-7 / 4.1e-7 vs 7.8e-7 / 6.0e-7, capacity 4.4e-6 / 2.8e-6 vs 1.4e-5 / 8.0e-6;
every case inside its bound (8 x the host path's error, at least 4 fp32 ulps)."""
import ctypes

import numpy as np
import pytest
import torch

import track_loss_ref as R

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
PAD = 64          # guard elements on either side of every output buffer


class Guard:
    """An output buffer pre-filled with a sentinel, with PAD guard elements before and behind it."""
    FILL = {torch.float32: float('nan'), torch.int32: 0x5A5A5A5A, torch.uint8: 0xA5}

    def __init__(self, shape, dtype):
        n = int(np.prod(shape))
        self.buf = torch.full((n + 2 * PAD,), self.FILL[dtype], dtype=dtype, device=DEV)
        self.out = self.buf[PAD:PAD + n].view(shape)
        assert self.out.data_ptr() % 16 == 0

    def check(self):
        g = torch.cat([self.buf[:PAD], self.buf[-PAD:]]).cpu()
        want = torch.full_like(g, self.FILL[g.dtype])
        assert torch.equal(torch.isnan(g), torch.isnan(want)) if g.dtype.is_floating_point else torch.equal(g, want), 'guard overwritten'
        return self.out.cpu().numpy()


def run_abi(vkn, case, gouts=()):
    """Forward (and one backward per gout) through the raw entry points on guarded outputs -> dict of host arrays."""
    L, ops = vkn._lib.lib(), vkn.ops
    B, N, E = case.shape
    cfg = ops.track_loss_cfg(**R.loss_cfg(case.head))
    key, ref = case.key.to(DEV).contiguous(), case.ref.to(DEV).contiguous()
    kgt, rgt = case.key_gt.to(DEV).contiguous(), case.ref_gt.to(DEV).contiguous()
    match = torch.cat(case.matches).to(DEV)
    off = torch.tensor(np.concatenate([[0], np.cumsum([len(m) for m in case.matches])]), dtype=torch.int64).to(DEV)
    losses, stats, kept = Guard((2,), torch.float32), Guard((B, 4), torch.int32), Guard((B, N, N), torch.uint8)
    status = torch.zeros(64, dtype=torch.int32, device=DEV)
    ws = torch.empty(L.vkn_track_loss_workspace_bytes(B, N), dtype=torch.uint8, device=DEV)
    st = ops._stream()
    vkn._lib.check(L.vkn_track_loss_fwd_f32(ctypes.byref(cfg), key.data_ptr(), ref.data_ptr(), kgt.data_ptr(), rgt.data_ptr(), match.data_ptr(),
                                            off.data_ptr(), match.numel(), B, N, E, losses.out.data_ptr(), stats.out.data_ptr(),
                                            kept.out.data_ptr(), status.data_ptr(), ws.data_ptr(), ws.numel(), st))
    out = dict(grads={})
    for gout in gouts:
        g = torch.tensor(gout, dtype=torch.float32).to(DEV)
        dk, dr = Guard((B, N, E), torch.float32), Guard((B, N, E), torch.float32)
        vkn._lib.check(L.vkn_track_loss_bwd_f32(ctypes.byref(cfg), key.data_ptr(), ref.data_ptr(), g.data_ptr(), B, N, E, dk.out.data_ptr(),
                                                dr.out.data_ptr(), ws.data_ptr(), ws.numel(), st))
        torch.cuda.synchronize()
        out['grads'][gout] = (dk.check(), dr.check())
    torch.cuda.synchronize()
    out.update(losses=losses.check(), stats=stats.check(), kept=kept.check(), status=int(status[0]))
    return out


_RUNS = {}


def gpu_run(vkn, name):
    """Every case runs once on the GPU (forward + the four backwards); the tests share the result and leave it unchanged."""
    if name not in _RUNS:
        _RUNS[name] = run_abi(vkn, R.CASES[name](), R.GOUTS)
    return _RUNS[name]


def _losses_close(got, want, rel=1e-5):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    nan = np.isnan(want)
    return np.array_equal(nan, np.isnan(got)) and bool(np.all(np.abs(got[~nan] - want[~nan]) < rel * np.maximum(1.0, np.abs(want[~nan]))))


# ---------------------------------------------------------------------------------------------------- values
@pytest.mark.parametrize('name', ['emb_cfg', 'emb_one', 'emb_temp'])
def test_golden_values_in_both_forms(vkn, name):
    """Losses against the reference's golden (1e-5 relative), stats and the kept mask bit-exact against the float64 restatement, and
    the full-row form (the same rows scattered among gt = 0 rows up to N = 100) bit-identical to the compact form in every output,
    with exact zeros on the gt = 0 rows of d_key / d_ref and untouched guards around every output buffer."""
    g = np.load(R.GOLDEN)
    compact, full = R.CASES[name + '_compact'](), R.CASES[name + '_full']()
    a, b = gpu_run(vkn, compact.name), gpu_run(vkn, full.name)
    want_a, want_b = R.reference(compact), R.reference(full)
    gold = [float(g[f'{name}_loss_track']), float(g[f'{name}_loss_track_aux']) if f'{name}_loss_track_aux' in g.files else 0.0]
    print(f'{name}: losses kernel {a["losses"].tolist()} golden {gold}')
    for run, want in ((a, want_a), (b, want_b)):
        assert run['status'] == 0
        assert _losses_close(run['losses'], gold)
        assert np.array_equal(run['stats'], want['stats'])
        assert np.array_equal(run['kept'], want['kept'])
    assert a['losses'].tobytes() == b['losses'].tobytes() and np.array_equal(a['stats'], b['stats'])
    for img in range(2):
        ka, ra = np.flatnonzero(compact.key_gt[img].numpy()), np.flatnonzero(compact.ref_gt[img].numpy())
        kb, rb = np.flatnonzero(full.key_gt[img].numpy()), np.flatnonzero(full.ref_gt[img].numpy())
        assert np.array_equal(a['kept'][img][np.ix_(ka, ra)], b['kept'][img][np.ix_(kb, rb)])
        for gout in R.GOUTS:
            for side, (ia, ib) in enumerate(((ka, kb), (ra, rb))):
                da, db = a['grads'][gout][side][img], b['grads'][gout][side][img]
                assert da[ia].tobytes() == db[ib].tobytes(), (gout, side)
                rest = np.ones(db.shape[0], dtype=bool)
                rest[ib] = False
                assert rest.sum() == 100 - len(ib) and not db[rest].any() and not np.isnan(db).any()


@pytest.mark.parametrize('name', R.EDGE_CASES)
def test_decision_edges(vkn, name):
    """The smallest shapes at which the loss takes another path (tests/track_loss_ref.py: CASES), and the capacity shape 128 x 128 rows
    at E = 1024: losses 1e-5 against the float64 restatement (NaN where it has NaN), stats bit-exact, the kept mask bit-exact wherever
    the cut is unambiguous (tests/test_track_loss_refs.py asserts that it is; the capacity case cuts among zero costs)."""
    case = R.CASES[name]()
    run, want = gpu_run(vkn, name), R.reference(case)
    print(f'{name}: losses kernel {run["losses"].tolist()} float64 {want["losses"].tolist()} stats {run["stats"].tolist()}')
    assert run['status'] == 0
    assert _losses_close(run['losses'], want['losses'])
    assert np.array_equal(run['stats'], want['stats'])
    if name != 'capacity':
        assert np.array_equal(run['kept'], want['kept'])
    else:
        pos = want['targets'][0] > 0                      # every row is a positive there: compact order = row order
        assert run['kept'].sum() == want['kept'].sum() and run['kept'][0][pos].all()


def test_image_without_a_partner_is_the_host_path(vkn):
    """num_pos = 0 in one image: 0 / 0 in both losses.  Losses and gradients equal the host path's, NaN positions included."""
    case = R.CASES['no_partner']()
    run = gpu_run(vkn, 'no_partner')
    for gout in R.GOUTS:
        host = R.host_path(vkn, case, gout)
        assert np.array_equal(np.isnan(run['losses']), np.isnan(host['losses'])) and np.isnan(run['losses']).all()
        for got, want in zip(run['grads'][gout], (host['d_key'], host['d_ref'])):
            assert np.array_equal(np.isnan(got), np.isnan(want)), gout
            assert not np.isnan(got[0]).any()
            assert R.rel_err(got, want.astype(np.float64)) < 1e-4


# ---------------------------------------------------------------------------------------------------- gradients
@pytest.mark.parametrize('gout', R.GOUTS)
@pytest.mark.parametrize('name', list(R.CASES))
def test_gradients_against_float64(vkn, name, gout):
    """d_key, d_ref per element against the float64 restatement; gout = (1, 0) and (0, 1) are the single-loss gradients.  The bound is
    8 x the error of the package's fp32 host path against the same float64 reference (a different summation order over up to 1024
    terms), at least 4 fp32 ulps of the tensor's largest magnitude — measured on the reference arithmetic at test time, not on the
    kernel.  A wrong term (a missing margin, a mis-kept negative, a wrong avg_factor) moves the result by >= 1e-3."""
    bounds, host_errs, want = R.grad_bounds(vkn, name, gout)
    got = gpu_run(vkn, name)['grads'][gout]
    errs = (R.rel_err(got[0], want['d_key']), R.rel_err(got[1], want['d_ref']))
    print(f'GRADERR {name} gout={gout} host d_key {host_errs[0]:.3e} d_ref {host_errs[1]:.3e} | kernel d_key {errs[0]:.3e} d_ref {errs[1]:.3e} '
          f'| bound {bounds[0]:.3e} {bounds[1]:.3e}')
    assert errs[0] <= bounds[0] and errs[1] <= bounds[1], (errs, bounds)


# ---------------------------------------------------------------------------------------------------- envelope, status word
def test_envelope_and_status_word(vkn):
    """N = 129 and E = 18 return VKN_E_SHAPE; a gt entry beyond the image's G sets VKN_STATUS_RANGE: `ops.workspace_status` raises once
    and is clear afterwards."""
    ops = vkn.ops
    case = R.CASES['no_mining']()
    cfg = ops.track_loss_cfg(**R.loss_cfg(case.head))
    match = torch.cat(case.matches).to(DEV)
    off = ops.track_match_offsets([len(m) for m in case.matches], DEV)
    assert off.tolist() == [0, len(case.matches[0])]
    for N, E in ((129, 16), (16, 18)):
        z = torch.zeros(1, N, E, device=DEV)
        gt = torch.zeros(1, N, dtype=torch.int64, device=DEV)
        with pytest.raises(vkn.VknError) as e:
            ops.track_loss_fwd(cfg, z, z, gt, gt, match, off)
        assert e.value.code == -2
        assert not ops.track_loss_supported(N, E)
    ops.workspace_status(DEV)
    args = [case.key.to(DEV), case.ref.to(DEV), case.key_gt.to(DEV), case.ref_gt.to(DEV), match, off]
    ops.track_loss_fwd(cfg, *args)
    ops.workspace_status(DEV)                                  # valid inputs: clear
    bad = case.key_gt.clone()
    bad[0, int(np.flatnonzero(bad[0].numpy())[0])] = len(case.matches[0]) + 1
    args[2] = bad.to(DEV)
    ops.track_loss_fwd(cfg, *args)
    with pytest.raises(vkn.VknError) as e:
        ops.workspace_status(DEV)
    assert e.value.code == -6
    ops.workspace_status(DEV)


# ---------------------------------------------------------------------------------------------------- the Python layers
def _cfg_inputs(vkn):
    """The emb_cfg head on the device, raw features [2,100,256,1,1] for the key and reference frames, and the full-row case's gt."""
    from oracle import synth
    case = R.CASES['emb_cfg_full']()
    cfg, sizes, seed = R.EMBED_CASES['emb_cfg']
    head = R.build_head(vkn, cfg)
    head.load_state_dict(R.embed_case_inputs(cfg, sizes, seed)[0], strict=True)
    head = head.to(DEV).train()
    kf = torch.from_numpy(synth.normalish((2, 100, 256, 1, 1), 8800, 1.0)).to(DEV)
    rf = torch.from_numpy(synth.normalish((2, 100, 256, 1, 1), 8801, 1.0)).to(DEV)
    return case, head, kf, rf


def _compact_inputs(case):
    kidx, ridx, kres, rres, matches = R.sampling(case, DEV)
    ke = torch.cat([case.key[b, kidx[b]] for b in range(case.shape[0])]).to(DEV)
    re_ = torch.cat([case.ref[b, ridx[b]] for b in range(case.shape[0])]).to(DEV)
    return ke, re_, kres, rres, matches


def test_track_train_tail_is_the_host_path_on_all_rows(vkn):
    """`TrackTrainTail` (slice, embed, track head on all rows, fused loss) against gather -> track head -> match / targets / loss on
    the same device: losses 1e-5; parameter gradients 5e-4 of each tensor's largest magnitude — both sides are fp32 and carry the
    rounding of their logits into the softmax weights, |s| eps sqrt(E) = 300 x 2^-24 x 16 = 2.9e-4 at most for logits below 300
    (asserted), once per side."""
    case, head, kf, rf = _cfg_inputs(vkn)
    embed = torch.nn.Sequential(torch.nn.Linear(256, 256), torch.nn.ReLU()).to(DEV)
    tail = vkn.TrackTrainTail(100, head, embed=embed)
    kgt, rgt = case.key_gt.to(DEV), case.ref_gt.to(DEV)
    matches = [m.to(DEV) for m in case.matches]
    params = list(head.parameters()) + list(embed.parameters())
    got = tail(torch.cat([kf, kf[:, :5]], 1), torch.cat([rf, rf[:, :5]], 1), [torch.cat([g, g[:5]]) for g in kgt], list(rgt), matches)
    g_got = torch.autograd.grad(got['loss_track'] + got['loss_track_aux'], params)
    kidx, ridx, kres, rres, _ = R.sampling(case, DEV)
    ke = torch.cat([head(embed(kf[b].reshape(100, 256))[kidx[b].to(DEV)]) for b in range(2)])
    re_ = torch.cat([head(embed(rf[b].reshape(100, 256))[ridx[b].to(DEV)]) for b in range(2)])
    dists, cos = head.match(ke, re_, kres, rres)
    assert max(float(d.abs().max()) for d in dists) < 300
    want = head.loss(dists, cos, *head.get_track_targets(matches, kres, rres))
    g_want = torch.autograd.grad(want['loss_track'] + want['loss_track_aux'], params)
    assert sorted(got) == sorted(want)
    for k in want:
        assert abs(float(got[k]) - float(want[k])) < 1e-5 * max(1.0, abs(float(want[k]))), k
    for a, b in zip(g_got, g_want):
        assert float((a - b).abs().max()) <= 5e-4 * float(b.abs().max())


def test_match_loss_layers(vkn, monkeypatch):
    """`match_loss` on CUDA inputs takes the fused path and equals `loss(*match, *get_track_targets)` within the measured bound; a
    `hard_mining=False, neg_pos_ub=3` head goes down the host path: the fused op is not called."""
    case = R.CASES['emb_cfg_compact']()
    bounds, _, want = R.grad_bounds(vkn, 'emb_cfg_compact', (1.0, 1.0))
    head = R.build_head(vkn, case.head).to(DEV)
    ke, re_, kres, rres, matches = _compact_inputs(case)
    calls = []
    real = vkn.ops.track_loss_fwd
    monkeypatch.setattr(vkn.ops, 'track_loss_fwd', lambda *a, **k: calls.append(1) or real(*a, **k))
    ke.requires_grad_(True); re_.requires_grad_(True)
    got = head.match_loss(ke, re_, kres, rres, matches)
    assert len(calls) == 1
    d_got = torch.autograd.grad(got['loss_track'] + got['loss_track_aux'], (ke, re_))
    host = head.loss(*head.match(ke, re_, kres, rres), *head.get_track_targets(matches, kres, rres))
    d_host = torch.autograd.grad(host['loss_track'] + host['loss_track_aux'], (ke, re_))
    for k in host:
        assert abs(float(got[k]) - float(host[k])) < 1e-5 * max(1.0, abs(float(host[k]))), k
    for a, b, bound in zip(d_got, d_host, bounds):
        assert float((a - b).abs().max()) <= bound * float(b.abs().max())
    soft = R.build_head(vkn, dict(case.head, loss_track_aux=dict(case.head['loss_track_aux'], hard_mining=False))).to(DEV)
    np.random.seed(0)
    out = soft.match_loss(ke.detach(), re_.detach(), kres, rres, matches)
    assert len(calls) == 1 and sorted(out) == ['loss_track', 'loss_track_aux']


def test_no_host_synchronisation_and_determinism(vkn):
    """`TrackTrainTail` and `match_loss`, forward and backward, under stream capture at the emb_cfg shape (one linear stream): capture and
    one replay succeed and the replayed results equal the eager ones bit for bit — a host synchronisation or a data-dependent shape
    would fail the capture.  Two eager calls on the same inputs are bit-identical."""
    case, head, kf, rf = _cfg_inputs(vkn)
    tail = vkn.TrackTrainTail(100, head)
    kgt, rgt = list(case.key_gt.to(DEV)), list(case.ref_gt.to(DEV))
    matches = [m.to(DEV) for m in case.matches]
    kf.requires_grad_(True); rf.requires_grad_(True)
    ke, re_, kres, rres, _ = _compact_inputs(R.CASES['emb_cfg_compact']())
    ke.requires_grad_(True); re_.requires_grad_(True)

    def step():
        a = tail(kf, rf, kgt, rgt, matches)
        b = head.match_loss(ke, re_, kres, rres, matches)
        grads = torch.autograd.grad(a['loss_track'] + 2.0 * a['loss_track_aux'] + b['loss_track'] - b['loss_track_aux'], (kf, rf, ke, re_))
        return [a['loss_track'], a['loss_track_aux'], b['loss_track'], b['loss_track_aux'], *grads]

    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        first = [t.clone() for t in step()]
        second = [t.clone() for t in step()]
    stream.synchronize()
    for a, b in zip(first, second):
        assert torch.equal(a, b) and not torch.isnan(a).any()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        captured = step()
    graph.replay()
    torch.cuda.synchronize()
    for a, b in zip(first, captured):
        assert torch.equal(a, b)
    vkn.ops.workspace_status(DEV)
