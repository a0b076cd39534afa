"""References, draws and premises of the tests of the deformable-attention core's BACKWARD (include/vkn_msda_train.h), on top of
tests/msda_ref.py.  Independent of the package: nothing here imports it.  tests/test_msda_bwd_refs.py proves the premises on the CPU;
tests/test_gpu_msda_bwd.py uses them.

  * reference = float64 autograd through `msda_ref.core_f64`; the second float64 form, autograd through `msda_ref.core_grid_sample` in
    float64, must agree with it to 1e-12 of each tensor's largest magnitude;
  * yardstick = fp32 autograd through `msda_ref.core_grid_sample`;
  * bound = `msda_ref.judge`: 8 x the yardstick's max error, at least 4 fp32 ulps of the tensor's largest magnitude.

The sampled value is continuous across integer pixel coordinates, its derivative by the offsets is not: a point within rounding of an
integer coordinate may fall on either side in fp32 and in float64.  So the backward's draw is `msda_ref.draw_core` followed by a
NUDGE: any offset whose coordinate (float64 evaluation of the fp32 inputs) lies within 1/64 of an integer gets + 1/16, at most four
times; 1/64 is several thousand times the fp32 error of a coordinate of magnitude <= 133."""
import numpy as np
import torch

import msda_ref as R

NEAR = 1.0 / 64
NUDGE = 1.0 / 16
DVALUE_FLOOR_EXEMPT = ('row-130',)      # its 3 x 130 level is sparsely hit at B = 1, Q = 33: 0.12 of dvalue is non-zero


def integer_distance(shapes, off, ref):
    """per offset component [B, Q, M, L, P, 2]: the distance of its pixel coordinate (float64 of the fp32 inputs) to the nearest integer"""
    x, y = R.pixel_coords(shapes, off.double(), ref.double())
    xy = torch.stack([x, y], -1)
    return (xy - xy.round()).abs()


def nudge(shapes, off, ref):
    off = off.clone()
    for _ in range(4):
        near = integer_distance(shapes, off, ref) < NEAR
        if not bool(near.any()):
            break
        off[near] += NUDGE
    return off


def draw_core_bwd(case, seed):
    """(value, off, logits, ref, dout): `draw_core`'s operands with the offsets nudged, dout ~ N(0, 1) [B, Q, M D]"""
    value, off, logits, ref = R.draw_core(case, seed)
    off = nudge(case.shapes, off, ref)
    gen = torch.Generator().manual_seed(seed + 77)
    dout = torch.randn((case.B, case.Q, case.M * case.D), generator=gen)
    return value, off, logits, ref, dout


def draw_exact_bwd(case, seed):
    """`draw_exact`'s operands and an integer dout in [-8, 8]"""
    value, off, logits, ref = R.draw_exact(case, seed)
    rng = np.random.default_rng(seed + 77)
    Q = off.shape[1]
    dout = torch.from_numpy(rng.integers(-8, 9, (case.B, Q, case.M * case.D)).astype(np.float32))
    return value, off, logits, ref, dout


def grads(core, shapes, value, off, logits, ref, dout, dtype):
    """(dvalue, doff, dlogits) by autograd through `core` (`R.core_f64`, or `R.core_grid_sample` at `dtype`) on leaves of `dtype`"""
    leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in (value, off, logits)]
    if core is R.core_f64:
        out = core(leaves[0], shapes, leaves[1], leaves[2], ref.to(dtype))
    else:
        out = core(leaves[0], shapes, leaves[1], leaves[2], ref.to(dtype), dtype)
    out.backward(dout.to(dtype))
    return tuple(t.grad for t in leaves)


def reference(case, value, off, logits, ref, dout):
    return grads(R.core_f64, case.shapes, value, off, logits, ref, dout, torch.float64)


def reference_grid_sample(case, value, off, logits, ref, dout):
    return grads(R.core_grid_sample, case.shapes, value, off, logits, ref, dout, torch.float64)


def yardstick(case, value, off, logits, ref, dout):
    return grads(R.core_grid_sample, case.shapes, value, off, logits, ref, dout, torch.float32)


def premises(name, case, off, ref, want):
    """what a per-element case relies on, from the actual operands and the float64 gradients `want` = (dvalue, doff, dlogits)"""
    dist = float(integer_distance(case.shapes, off, ref).min())
    if dist < NEAR:
        raise R.PremiseError(f'{name}: a pixel coordinate lies {dist:.4f} from an integer')
    if name in R.BANDS_ASSERTED:
        shares = R.band_shares(case.shapes, off, ref)
        if min(shares.values()) < 0.20:
            raise R.PremiseError(f'{name}: band shares {shares}')
    nz_value, nz_off = float((want[0] != 0).double().mean()), float((want[1] != 0).double().mean())
    if nz_off < 0.3 or (nz_value < 0.3 and name not in DVALUE_FLOOR_EXEMPT):
        raise R.PremiseError(f'{name}: vacuous, {nz_off:.2f} of doff and {nz_value:.2f} of dvalue are non-zero')
    return dict(min_distance=dist, nonzero_dvalue=nz_value, nonzero_doff=nz_off)


def _on_grid(t, log2_step):
    s = t * 2.0 ** log2_step
    return torch.equal(s, s.round())


def exact_premise_bwd(name, case, value, off, logits, ref, dout):
    """what makes an exact case's BACKWARD exact in fp32 in any order: the forward's premise, an integer dout of at most 8, and float64
    gradients that are fp32 numbers on the grid 2^-10 (dvalue, doff) / 2^-12 (dlogits) -> the three float64 gradients.
    Partial sums: a dvalue term is a multiple of 2^-6 (a softmax weight down to 1/4 times a corner weight down to 1/16) of at most 8,
    at most 512 of them reach a cell; a doff term is a multiple of 2^-4 with sum |.| <= 2^17: both fit 24 bits in any order."""
    R.exact_premise(case, value, off, logits, ref)
    if not torch.equal(dout, dout.round()) or float(dout.abs().max()) > 8:
        raise R.PremiseError(f'{name}: dout is not an integer of at most 8')
    want = reference(case, value, off, logits, ref, dout)
    for label, g, step in (('dvalue', want[0], 10), ('doff', want[1], 10), ('dlogits', want[2], 12)):
        if not torch.equal(g.float().double(), g):
            raise R.PremiseError(f'{name}: the float64 {label} is not an fp32 number')
        if not _on_grid(g, step):
            raise R.PremiseError(f'{name}: the float64 {label} is not a multiple of 2^-{step}')
    Q, P = off.shape[1], case.P
    if Q * P > 512 or Q * P * 8 * 2 ** 6 >= 2 ** 24:                       # a cell receives at most Q P terms, each |.| <= 8 on the grid 2^-6
        raise R.PremiseError(f'{name}: {Q * P} terms may reach a cell of dvalue')
    if case.D * 8 * 256 * 2 ** 4 >= 2 ** 24:                              # D terms |dout| <= 8 times |hh (v2 - v1) + lh (v4 - v3)| <= 256 on 2^-4
        raise R.PremiseError(f'{name}: a doff sum may not fit 24 bits')
    if float((want[0] != 0).double().mean()) < 0.3 or float((want[1] != 0).double().mean()) < 0.05:
        raise R.PremiseError(f'{name}: vacuous gradients')
    return want


class Leaf:
    """`msda_ref.decoder_f64` takes `t.detach().cpu().double()` of every state-dict entry and input: handed a `Leaf`, it computes on the
    float64 leaf itself, so that autograd reaches it"""

    def __init__(self, t):
        self.t = t.detach().cpu().double().clone().requires_grad_(True)

    def detach(self):
        return self

    def cpu(self):
        return self

    def double(self):
        return self.t


def decoder_grads_f64(state_dict, feats, weights, num_heads):
    """loss = sum_k (out_k * weights_k).sum() through `msda_ref.decoder_f64` in float64 -> ({parameter name: grad}, [input grads])"""
    sd = {k: Leaf(v) for k, v in state_dict.items()}
    ins = [Leaf(f) for f in feats]
    outs = R.decoder_f64(sd, ins, num_heads=num_heads)
    loss = sum((o * w.double()).sum() for o, w in zip(outs, weights))
    loss.backward()
    return {k: v.t.grad for k, v in sd.items()}, [f.t.grad for f in ins]
