"""Plain float64 references of the training chain's building blocks (tests/test_gpu_chain_blocks.py compares csrc/vkn_train.hip with
them element by element; tests/test_chain_block_refs.py pins THEM on the CPU against `_updator_torch`, the oracle and torch's own
MultiheadAttention).  torch ops only, differentiable, no kernel of this library — device-agnostic (they run where their inputs live).

Order of the eight norm vectors everywhere: (norm_in w, b, norm_out w, b, input_norm_in w, b, input_norm_out w, b) — the order of
`VknUpdatorNorms` / `VknUpdatorNormGrads` in include/vkn.h; of the four (mean, rstd) pairs of `stats` [M, 8]: norm_in(UG),
norm_out(param_out), input_norm_in(IG), input_norm_out(input_out)."""
import torch
import torch.nn.functional as F

NORM_NAMES = ('norm_in', 'norm_out', 'input_norm_in', 'input_norm_out')


def gate_product(params, inputs):
    """knet/kernel_updator.py:70 — the first halves of the packed [M, 2C] layer outputs, multiplied."""
    C = params.shape[1] // 2
    return params[:, :C] * inputs[:, :C]


def ln_stats(x, eps):
    """(mean, 1 / sqrt(var + eps)) per row, biased variance — what nn.LayerNorm normalises with."""
    mean = x.mean(1)
    var = ((x - mean[:, None]) ** 2).mean(1)
    return mean, 1.0 / torch.sqrt(var + eps)


def updator_mix(params, inputs, gates, norms, b_i=None, b_u=None, eps=1e-5, with_stats=False):
    """knet/kernel_updator.py:74-90 (gate_sigmoid=True, gate_norm_act=False): gates [M, 2C] = [IG | UG] is the bias-free output of the two
    gate layers, b_i / b_u their biases (or None).
      F = sigmoid(LN_norm_in(UG + b_u)) LN_norm_out(params[:, C:]) + sigmoid(LN_input_norm_in(IG + b_i)) LN_input_norm_out(inputs[:, C:])"""
    C = params.shape[1] // 2
    in_w, in_b, out_w, out_b, iin_w, iin_b, iout_w, iout_b = norms
    ig = gates[:, :C] + (b_i if b_i is not None else 0.0)
    ug = gates[:, C:] + (b_u if b_u is not None else 0.0)
    po, io = params[:, C:], inputs[:, C:]
    zu = F.layer_norm(ug, (C,), in_w, in_b, eps)
    zi = F.layer_norm(ig, (C,), iin_w, iin_b, eps)
    feats = torch.sigmoid(zu) * F.layer_norm(po, (C,), out_w, out_b, eps) + torch.sigmoid(zi) * F.layer_norm(io, (C,), iout_w, iout_b, eps)
    if not with_stats:
        return feats
    stats = torch.stack([v for x in (ug, po, ig, io) for v in ln_stats(x.detach(), eps)], 1)      # [M, 8]
    return feats, stats, zu.detach(), zi.detach()


def updator_core(params, inputs, wig, wug, norms, b_i=None, b_u=None, eps=1e-5):
    """:70-90 with the gate layers: ONE GEMM on the stacked weights [W_ig ; W_ug], as `UpdatorCoreFn` launches it."""
    gates = F.linear(gate_product(params, inputs), torch.cat([wig, wug]))
    return updator_mix(params, inputs, gates, norms, b_i, b_u, eps)


def kernel_updator(ku_sd, update_feature, input_feature, eps=1e-5, pre_relu=False):
    """The whole `KernelUpdator.forward` (:56-93, K*K = 1) from a state dict of its parameters: [M, C] x [M, C] -> [M, C]."""
    params = F.linear(update_feature, ku_sd['dynamic_layer.weight'], ku_sd['dynamic_layer.bias'])
    inputs = F.linear(input_feature, ku_sd['input_layer.weight'], ku_sd['input_layer.bias'])
    norms = [ku_sd[f'{n}.{p}'] for n in NORM_NAMES for p in ('weight', 'bias')]
    feats = updator_core(params, inputs, ku_sd['input_gate.weight'], ku_sd['update_gate.weight'], norms, ku_sd['input_gate.bias'],
                         ku_sd['update_gate.bias'], eps)
    z = F.layer_norm(F.linear(feats, ku_sd['fc_layer.weight'], ku_sd['fc_layer.bias']), (feats.shape[1],), ku_sd['fc_norm.weight'],
                     ku_sd['fc_norm.bias'], eps)
    return z if pre_relu else torch.relu(z)


def attention(q, k, v, B, heads, with_scores=False):
    """The attention core of nn.MultiheadAttention: q [B Nq, C], k / v [B Nk, C], rows b * N + i, head h = columns [h hd, (h + 1) hd)
    -> softmax_j(q_i . k_j / sqrt(hd)) v_j  [B Nq, C]"""
    Mq, C = q.shape
    hd = C // heads
    qh = q.reshape(B, -1, heads, hd).transpose(1, 2)
    kh = k.reshape(B, -1, heads, hd).transpose(1, 2)
    vh = v.reshape(B, -1, heads, hd).transpose(1, 2)
    s = qh @ kh.transpose(-1, -2) / hd ** 0.5
    out = (torch.softmax(s, -1) @ vh).transpose(1, 2).reshape(Mq, C)
    return (out, s.detach()) if with_scores else out


def layernorm_act(x, resid, gamma, beta, eps, act):
    """act(LayerNorm_C(x + resid) gamma + beta): act 0 none / 1 ReLU / 2 sigmoid; resid / gamma / beta may be None"""
    z = F.layer_norm(x + resid if resid is not None else x, (x.shape[1],), None, None, eps)     # (affine by hand: either may be None)
    if gamma is not None:
        z = z * gamma
    if beta is not None:
        z = z + beta
    return torch.relu(z) if act == 1 else torch.sigmoid(z) if act == 2 else z


def linear_dw(dy, a):
    """dW [Nout, K] = dy^T a, db [Nout] = column sums of dy"""
    return dy.t() @ a, dy.sum(0)
