"""CPU: the float64 references of tests/chain_block_refs.py are themselves pinned — against this package's torch composition of the
kernel update (`kernel_update_head._updator_torch`), against the oracle's `kernel_updator` (what the reference goldens pin), by
`torch.autograd.gradcheck`, and against torch's own `nn.MultiheadAttention`.  tests/test_gpu_chain_blocks.py trusts them after this."""
import pytest
import torch

import chain_block_refs as R


def _ku(vkn, C, seed):
    torch.manual_seed(seed)
    ku = vkn.kernel_updator.KernelUpdator(in_channels=C, feat_channels=C).double()
    with torch.no_grad():                               # norm parameters off their init values (ones / zeros hide a swap)
        for n, p in ku.named_parameters():
            if 'norm' in n:
                p.copy_(torch.randn_like(p) * (0.5 if n.endswith('weight') else 0.3) + (1.0 if n.endswith('weight') else 0.0))
    return ku


@pytest.mark.parametrize('M,C', [(7, 8), (33, 64)])
def test_updator_reference_equals_the_package_torch_composition(vkn, M, C):
    from importlib import import_module
    kuh = import_module('video_k_net_amd.kernel_update_head')
    ku = _ku(vkn, C, 3)
    u, k = torch.randn(M, C, dtype=torch.float64), torch.randn(M, C, dtype=torch.float64)
    with torch.no_grad():
        want = kuh._updator_torch(ku, u, k.reshape(M, 1, C)).reshape(M, C)
        got = R.kernel_updator(dict(ku.named_parameters()), u, k, ku.norm_in.eps)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())
    assert bool((want > 0).any()) and bool((want == 0).any())


@pytest.mark.parametrize('M,C', [(7, 8), (33, 64)])
def test_updator_reference_equals_the_oracle(vkn, M, C):
    from oracle.knet_oracle import HeadCfg, kernel_updator
    ku = _ku(vkn, C, 4)
    u, k = torch.randn(M, C, dtype=torch.float64), torch.randn(M, C, dtype=torch.float64)
    sd = {'ku.' + n: p.detach() for n, p in ku.named_parameters()}
    cfg = HeadCfg(in_channels=C, feat_channels=C, ln_eps=ku.norm_in.eps)
    want = kernel_updator(sd, 'ku', u.reshape(1, M, C), k.reshape(1, M, 1, C), cfg).reshape(M, C)
    got = R.kernel_updator({n: p.detach() for n, p in ku.named_parameters()}, u, k, ku.norm_in.eps)
    assert float((got - want).abs().max()) < 1e-12 * float(want.abs().max())


def test_updator_mix_stats_are_the_layernorms_statistics():
    """the `stats` the reference reports are the (mean, rstd) its own LayerNorms used: rebuilding each LayerNorm from them gives F"""
    M, C, eps = 5, 12, 1e-5
    g = torch.Generator().manual_seed(1)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)      # noqa: E731
    p, i, gt = rnd(M, 2 * C), rnd(M, 2 * C), rnd(M, 2 * C)
    norms = [rnd(C) for _ in range(8)]
    bi, bu = rnd(C), rnd(C)
    f, st, zu, zi = R.updator_mix(p, i, gt, norms, bi, bu, eps, with_stats=True)
    xs = (gt[:, C:] + bu, p[:, C:], gt[:, :C] + bi, i[:, C:])
    z = [(x - st[:, 2 * j, None]) * st[:, 2 * j + 1, None] * norms[2 * j] + norms[2 * j + 1] for j, x in enumerate(xs)]
    assert float((torch.sigmoid(z[0]) * z[1] + torch.sigmoid(z[2]) * z[3] - f).abs().max()) < 1e-12
    assert float((z[0] - zu).abs().max()) < 1e-12 and float((z[2] - zi).abs().max()) < 1e-12


def test_updator_reference_passes_gradcheck():
    M, C = 3, 4
    g = torch.Generator().manual_seed(2)
    rnd = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64).requires_grad_(True)      # noqa: E731
    p, i, gt = rnd(M, 2 * C), rnd(M, 2 * C), rnd(M, 2 * C)
    norms = [rnd(C) for _ in range(8)]
    bi, bu = rnd(C), rnd(C)
    assert torch.autograd.gradcheck(lambda *a: R.updator_mix(a[0], a[1], a[2], a[5:], a[3], a[4], 1e-5), (p, i, gt, bi, bu, *norms))
    assert torch.autograd.gradcheck(R.gate_product, (p, i))
    wig, wug = rnd(C, C), rnd(C, C)
    assert torch.autograd.gradcheck(lambda *a: R.updator_core(a[0], a[1], a[2], a[3], a[6:], a[4], a[5], 1e-5), (p, i, wig, wug, bi, bu, *norms))


@pytest.mark.parametrize('B,Nq,Nk,heads,hd', [(2, 5, 5, 2, 4), (3, 7, 11, 4, 8), (1, 1, 9, 1, 16), (2, 6, 1, 8, 4)])
def test_attention_reference_equals_torch_multihead_attention_core(B, Nq, Nk, heads, hd):
    """nn.MultiheadAttention with identity projections and no biases IS its attention core"""
    E = heads * hd
    g = torch.Generator().manual_seed(5)
    q, k, v = (torch.randn(B * n, E, generator=g, dtype=torch.float64) for n in (Nq, Nk, Nk))
    mha = torch.nn.MultiheadAttention(E, heads, bias=False).double()
    with torch.no_grad():
        mha.in_proj_weight.copy_(torch.eye(E, dtype=torch.float64).repeat(3, 1))
        mha.out_proj.weight.copy_(torch.eye(E, dtype=torch.float64))
    seq = lambda t, n: t.reshape(B, n, E).transpose(0, 1)                    # noqa: E731   rows b * N + i -> [L, B, E]
    with torch.no_grad():
        want = mha(seq(q, Nq), seq(k, Nk), seq(v, Nk), need_weights=False)[0].transpose(0, 1).reshape(B * Nq, E)
    got, s = R.attention(q, k, v, B, heads, with_scores=True)
    assert s.shape == (B, heads, Nq, Nk)
    assert float((got - want).abs().max()) < 1e-12


def test_layernorm_and_dw_references():
    g = torch.Generator().manual_seed(6)
    x, r = torch.randn(9, 7, generator=g, dtype=torch.float64), torch.randn(9, 7, generator=g, dtype=torch.float64)
    gm, bt = torch.randn(7, generator=g, dtype=torch.float64), torch.randn(7, generator=g, dtype=torch.float64)
    ln = torch.nn.LayerNorm(7, eps=1e-5).double()
    with torch.no_grad():
        ln.weight.copy_(gm)
        ln.bias.copy_(bt)
    assert float((R.layernorm_act(x, r, gm, bt, 1e-5, 2) - torch.sigmoid(ln(x + r))).abs().max()) < 1e-14
    assert float((R.layernorm_act(x, None, None, bt, 1e-5, 0) - (torch.nn.functional.layer_norm(x, (7,)) + bt)).abs().max()) < 1e-14
    assert torch.equal(R.layernorm_act(x, None, None, None, 1e-5, 1), torch.relu(torch.nn.functional.layer_norm(x, (7,))))
    mean, rstd = R.ln_stats(x, 1e-5)
    assert float((((x - mean[:, None]) * rstd[:, None]) - torch.nn.functional.layer_norm(x, (7,))).abs().max()) < 1e-12
    dy, a = torch.randn(9, 3, generator=g, dtype=torch.float64), torch.randn(9, 5, generator=g, dtype=torch.float64)
    w = torch.zeros(3, 5, dtype=torch.float64, requires_grad=True)
    b = torch.zeros(3, dtype=torch.float64, requires_grad=True)
    (torch.nn.functional.linear(a, w, b) * dy).sum().backward()
    dW, db = R.linear_dw(dy, a)
    assert float((dW - w.grad).abs().max()) < 1e-12 and float((db - b.grad).abs().max()) < 1e-12
