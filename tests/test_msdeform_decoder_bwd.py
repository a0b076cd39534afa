"""CPU: `MSDeformAttnPixelDecoder(fused_backward=...)`, the flag that gives the training path the library's sampling core with its HIP
backward (include/vkn_msda_train.h) on CUDA tensors.  Without a GPU: the flag exists with its default, CPU tensors take the torch
composition whatever it says and give bitwise the same gradients either way, and it adds no state-dict key.
tests/test_gpu_msda_bwd.py judges the gradients on the GPU."""
import copy
import inspect

import torch

import msda_ref as R
from test_msdeform_decoder import BASE

# profiles/msda_bwd_ab.txt qualifies True (2.3 - 2.4 x faster at all four shipped points); the default stays False because
# tests/test_gpu_msda.py::test_module_path_choices pins the DEFAULT training call to the torch composition with no kernel call.
FLAG_DEFAULT = False


def _neck(vkn, **kw):
    torch.manual_seed(21)
    neck = vkn.build_neck(dict(R.module_cfg(R.MODULE_CASES['narrow'], BASE), **kw))
    neck.init_weights()
    R.randomise(neck, 22)
    return neck


def test_the_flag_and_its_default(vkn):
    sig = inspect.signature(vkn.MSDeformAttnPixelDecoder.__init__).parameters
    assert sig['fused_backward'].default is FLAG_DEFAULT and sig['fused'].default is True
    assert list(sig)[-2:] == ['fused', 'fused_backward']                           # behind the reference's own arguments
    plain = vkn.MSDeformAttnPixelDecoder()
    assert plain.fused_backward is FLAG_DEFAULT and plain.fused is True
    assert all(layer.attentions[0].fused_backward is FLAG_DEFAULT for layer in plain.encoder.layers)
    on = vkn.build_neck(dict(copy.deepcopy(BASE), fused_backward=True))
    assert on.fused_backward is True and all(layer.attentions[0].fused_backward is True for layer in on.encoder.layers)
    # the attention's own ctor arguments are mmcv's: the flag is an attribute the decoder sets
    attn = type(plain.encoder.layers[0].attentions[0])
    assert 'fused_backward' not in inspect.signature(attn.__init__).parameters


def test_state_dict_keys_are_unchanged(vkn):
    for flag in (False, True):
        neck = vkn.build_neck(dict(copy.deepcopy(BASE), fused_backward=flag))
        assert sorted(neck.state_dict()) == R.expected_keys(num_layers=6)
    a, b = _neck(vkn, fused_backward=False), _neck(vkn, fused_backward=True)
    assert list(a.state_dict()) == list(b.state_dict())
    b.load_state_dict(a.state_dict(), strict=True)


def test_cpu_tensors_take_the_torch_composition_either_way(vkn, monkeypatch):
    def forbidden(*a, **k):
        raise AssertionError('the library core was called on CPU tensors')
    monkeypatch.setattr(vkn.autograd, 'msda_sample', forbidden)
    monkeypatch.setattr(vkn.ops, 'msda_sample', forbidden)
    feats = R.module_inputs(R.MODULE_CASES['narrow'], 23)
    gen = torch.Generator().manual_seed(24)
    results = []
    for flag in (False, True):
        neck = _neck(vkn, fused_backward=flag)
        ins = [f.clone().requires_grad_(True) for f in feats]
        outs = neck(ins)
        if not results:
            weights = [torch.randn(o.shape, generator=gen) for o in outs]
        sum((o * w).sum() for o, w in zip(outs, weights)).backward()
        results.append(([o.detach() for o in outs], {k: p.grad for k, p in neck.named_parameters()}, [x.grad for x in ins]))
    (o0, p0, x0), (o1, p1, x1) = results
    assert all(torch.equal(a, b) for a, b in zip(o0, o1)) and all(torch.equal(a, b) for a, b in zip(x0, x1))
    assert p0.keys() == p1.keys() and all(g is not None for g in p0.values())
    assert all(torch.equal(p0[k], p1[k]) for k in p0)
    assert float(p0['encoder.layers.0.attentions.0.sampling_offsets.weight'].abs().max()) > 0
