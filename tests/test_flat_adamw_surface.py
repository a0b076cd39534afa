"""CPU (-m "not gpu"): the host surface of the flat AdamW optimizer — the C ABI of vkn_adamw_flat_f32 (struct mirror, workspace query,
argument checks before any launch) and dist.FlatAdamW's validation.  No compute kernel is launched here."""
import ctypes
from importlib import import_module

import pytest
import torch


def _dist(vkn):
    return import_module('video_k_net_amd.dist')


def test_adamw_item_mirror_and_workspace_query_are_host_only(vkn):
    L = vkn._lib.lib()
    assert L.vkn_sizeof_adamw_item() == ctypes.sizeof(vkn._lib.VknAdamwItem) == 48
    for sym in ('vkn_sizeof_adamw_item', 'vkn_adamw_workspace_bytes', 'vkn_adamw_flat_f32'):
        assert sym in vkn._lib.SYMBOLS
    nb = L.vkn_adamw_workspace_bytes(700, 300, 3)
    assert nb >= 700 * 8 and nb % 256 == 0
    assert L.vkn_adamw_workspace_bytes(1, 1, 1) > 0
    for bad in ((0, 1, 1), (1, 0, 1), (1, 1, 0), (-5, 1, 1)):
        assert L.vkn_adamw_workspace_bytes(*bad) == 0


def test_adamw_entry_point_validates_on_the_host(vkn):
    """Null pointers, bad counts, a NaN max_norm, a missing / short workspace and misaligned pointers come back as error codes
    before anything is launched (the fake device addresses below are never dereferenced)."""
    L = vkn._lib.lib()
    fake = 1 << 40                                       # 256-byte aligned, never touched: every call below fails its checks first
    ws = L.vkn_adamw_workspace_bytes(4, 2, 1)
    ok = dict(items=fake, n_items=4, n_params=2, rows=fake, n_groups=1, steps=fake, active=fake, max_norm=1.0, tn=None, coef=None,
              ws=fake, ws_bytes=ws)

    def call(**over):
        a = dict(ok, **over)
        return L.vkn_adamw_flat_f32(a['items'], a['n_items'], a['n_params'], a['rows'], a['n_groups'], a['steps'], a['active'],
                                    a['max_norm'], a['tn'], a['coef'], a['ws'], a['ws_bytes'], None)
    for over in (dict(items=None), dict(rows=None), dict(steps=None), dict(active=None), dict(n_items=0), dict(n_params=0),
                 dict(n_groups=-1), dict(max_norm=float('nan'))):
        assert call(**over) == -1, over
    assert call(ws=None) == -3 and call(ws_bytes=ws - 1) == -3
    assert call(ws=fake + 4) == -5 and call(items=fake + 4) == -5 and call(rows=fake + 2) == -5 and call(tn=fake + 2) == -5


def test_flat_adamw_rejects_what_it_does_not_provide(vkn):
    d = _dist(vkn)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    red = d.BucketedGradAllReducer(net)
    for kw in (dict(amsgrad=True), dict(maximize=True), dict(norm_type=float('inf')), dict(norm_type=1)):
        with pytest.raises(NotImplementedError):
            d.FlatAdamW(red, **kw)
    with pytest.raises(NotImplementedError):
        d.FlatAdamW(red, [dict(params=[net[0].weight], amsgrad=True)])
    with pytest.raises(ValueError):
        d.FlatAdamW(red, max_norm=0.0)
    with pytest.raises(ValueError):
        d.FlatAdamW(red, lr=-1.0)


def test_flat_adamw_names_a_parameter_outside_the_reducer(vkn):
    d = _dist(vkn)
    net = torch.nn.Sequential(torch.nn.Linear(5, 7), torch.nn.Linear(7, 3))
    red = d.BucketedGradAllReducer(net)
    stranger = torch.nn.Parameter(torch.zeros(11, 2))
    before = [p.data_ptr() for p in net.parameters()]
    with pytest.raises(ValueError, match=r"param_groups\[1\]\['params'\]\[0\].*\(11, 2\)"):
        d.FlatAdamW(red, [dict(params=list(net[0].parameters())), dict(params=[stranger], lr=1e-4)])
    with pytest.raises(ValueError, match='not a parameter of the reducer'):
        d.FlatAdamW(red, [stranger])
    # validation happens before the parameters are moved: a failed construction leaves the module as it was
    assert [p.data_ptr() for p in net.parameters()] == before


def test_flat_adamw_cpu_parameters_raise(vkn):
    """fp32 CUDA parameters only: no CPU fallback."""
    d = _dist(vkn)
    net = torch.nn.Linear(5, 7)
    red = d.BucketedGradAllReducer(net)
    w = net.weight.detach().clone()
    with pytest.raises(RuntimeError, match='no CPU fallback'):
        d.FlatAdamW(red, lr=1e-4, weight_decay=0.05, max_norm=1.0)
    assert torch.equal(net.weight.detach(), w)
