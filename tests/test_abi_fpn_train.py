"""The C ABI of the training part include/vkn_fpn_train.h, judged as tests/test_abi_vpq.py judges its header: a regex reading of the
argument lists, the built library's exports, a C compiler for the header, the workspace sizes and the refusals in their order.  The
part is bound through a FIFTH table, `_lib.TRAIN_HEADERS` / `_lib.ABI_TRAIN`, and leaves the four tables before it and their constant
records as they were."""
import ctypes
import os
import re

import pytest

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_fpn_train.h'
SYMBOLS = {'vkn_gn_relu_apply_f32': 11, 'vkn_gn_relu_bwd_workspace_bytes': 5, 'vkn_gn_relu_bwd_f32': 16, 'vkn_conv_wgrad_workspace_bytes': 7,
           'vkn_conv_wgrad_f32': 13, 'vkn_conv_dgrad_workspace_bytes': 5, 'vkn_conv_dgrad_f32': 13}
CONSTS = dict(VKN_FPN_BWD_RUN_PX=2048, VKN_FPN_WGRAD_MAX_SPLITS=64, VKN_FPN_WGRAD_TARGET_WGS=256)
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def test_the_training_table_leaves_the_four_tables_alone(vkn):
    lib = vkn._lib
    assert lib.TRAIN_HEADERS == (HEADER,) == tuple(lib.ABI_TRAIN)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    part = lib.ABI_TRAIN[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) and set(part.symbols) == set(SYMBOLS)
    others = {s for t in (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC) for h in t.values() for s in h.symbols}
    assert not set(part.symbols) & others                                            # no name is declared twice
    assert part.consts == CONSTS == lib.FPN_TRAIN and not set(CONSTS) & (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ))
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert lib.SEG == lib.ABI_EXT['vkn_seg_loss.h'].consts and lib.STQ == lib.ABI_METRIC['vkn_stq.h'].consts and lib.VPQ == lib.ABI_WINDOW_METRIC['vkn_vpq.h'].consts
    assert not part.structs and not part.mirrors and 'vkn_fpn_bwd.hip' in lib.SOURCES
    # the five tables go through the same loops: every prototype of the part is among `_each`'s
    assert {n for h, n, _ in lib._each('protos') if h == HEADER} == set(SYMBOLS)
    names = [n for _, n, _ in lib._each('protos')]
    assert len(names) == len(set(names))
    # one reading over the five tables: the part sees vkn.h's error codes through its #include, and declares nothing in vkn.h
    every = lib.read_abi(os.path.join(ROOT, 'include'), lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS)
    assert every[HEADER].protos == part.protos and {h: every[h].protos for h in HEADERS} == {h: lib.ABI[h].protos for h in HEADERS}
    assert not any(n.startswith(('vkn_gn_relu', 'vkn_conv_wgrad', 'vkn_conv_dgrad')) for n in lib.PROTOS)
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_TRAIN[HEADER].symbols) and len(declared) == len(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert getattr(raw, name) is not None
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith('_workspace_bytes') else ctypes.c_int), name
        assert len(fn.argtypes) == params.count(',') + 1 == SYMBOLS[name], name
        assert all(t in (ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t) for t in fn.argtypes), name
        if not name.endswith('_workspace_bytes'):
            assert fn.argtypes[-1] is ctypes.c_void_p and fn.argtypes[0] is ctypes.c_void_p, name        # device pointers travel as integers; stream last


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ size_t n = vkn_conv_wgrad_workspace_bytes(2, 32, 3, 7, 32, 3, 1);\n'
                   '  return n > (size_t)(VKN_FPN_BWD_RUN_PX + VKN_FPN_WGRAD_MAX_SPLITS + VKN_FPN_WGRAD_TARGET_WGS + VKN_E_SHAPE) ? 0 : 1; }\n')
    _compile('c99', src)


def test_workspace_sizes_and_envelope(vkn):
    L = vkn._lib.lib()
    al = lambda n: (n + 255) // 256 * 256                                            # noqa: E731
    gn, wg, dg = L.vkn_gn_relu_bwd_workspace_bytes, L.vkn_conv_wgrad_workspace_bytes, L.vkn_conv_dgrad_workspace_bytes
    # GroupNorm backward: header, fp64 (sum dz, sum dz xhat) per (frame, channel, run), the same per (frame, channel), fp32 means per (frame, group)
    assert gn(2, 32, 3, 7, 8) == 256 + al(2 * 32 * 1 * 16) + al(2 * 32 * 16) + al(2 * 8 * 8)
    assert gn(2, 32, 33, 63, 8) == 256 + al(2 * 32 * 2 * 16) + al(2 * 32 * 16) + al(2 * 8 * 8)          # 2079 pixels: two runs
    assert gn(1, 32, 32, 64, 8) == 256 + al(32 * 1 * 16) + al(32 * 16) + al(8 * 8)                       # 2048: one
    # weight gradient: header, the two powers of two, the max |v| partials, `splits` partial tiles
    tile = lambda s, co, ci, k: al(s * co * ci * k * k * 4)                          # noqa: E731
    assert wg(2, 32, 3, 7, 32, 3, 1) == 256 + 256 + 1024 + tile(6, 32, 32, 3)                            # 6 runs: 6 splits
    assert wg(1, 32, 1, 64, 32, 3, 1) == 256 + 256 + 1024 + tile(1, 32, 32, 3)                           # one run
    assert wg(2, 256, 64, 128, 256, 3, 1) == 256 + 256 + 1024 + tile(16, 256, 256, 3)                    # 16 tiles of (32 ci, 128 co): 256 / 16 splits
    assert wg(2, 32, 128, 128, 32, 1, 1) == 256 + 256 + 1024 + tile(64, 32, 32, 1)                       # never above VKN_FPN_WGRAD_MAX_SPLITS
    assert wg(2, 32, 5, 67, 32, 3, 2) == 256 + 256 + 1024 + tile(6, 32, 32, 3)                           # stride 2: 3 x 34 outputs
    assert dg(2, 32, 3, 7, 1) == dg(3, 512, 100, 100, 2) == 256 + 256 + 1024
    for bad in ((0, 32, 3, 7, 8), (2, 48, 3, 7, 8), (2, 544, 3, 7, 8), (2, 32, 0, 7, 8), (2, 32, 3, 7, 5), (2, 32, 3, 7, 0), (64, 512, 128, 128, 32)):
        assert gn(*bad) == 0, bad
    for bad in ((2, 48, 3, 7, 32, 3, 1), (2, 32, 3, 7, 48, 3, 1), (2, 32, 3, 7, 32, 5, 1), (2, 32, 3, 7, 32, 1, 2), (2, 32, 3, 7, 32, 3, 3),
                (0, 32, 3, 7, 32, 3, 1), (2, 32, 3, -7, 32, 3, 1), (64, 512, 128, 128, 32, 3, 1), (64, 32, 128, 128, 512, 1, 1)):
        assert wg(*bad) == 0, bad
    for bad in ((0, 32, 3, 7, 1), (2, 48, 3, 7, 1), (2, 32, 3, 7, 3), (2, 32, 0, 7, 1), (64, 512, 128, 128, 1)):
        assert dg(*bad) == 0, bad


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / counts <= 0 -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the workspace -> VKN_E_WORKSPACE, then alignment ->
    VKN_E_ALIGN: all decided before the library asks the runtime anything (the pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd = 4096, 4096 + 4

    def call(fn, ok, **kw):
        return fn(*dict(ok, **kw).values())
    # ---- apply (no workspace)
    ok = dict(r=p, stats=p, gamma=p, beta=p, groups=8, y=p, B=2, C=32, H=3, W=7, stream=None)
    f = L.vkn_gn_relu_apply_f32
    for k in ('r', 'stats', 'gamma', 'beta', 'y'):
        assert call(f, ok, **{k: None}) == call(f, ok, **{k: None, 'C': 48}) == E_ARG, k
        assert call(f, ok, **{k: odd}) == E_ALIGN and call(f, ok, **{k: odd, 'groups': 5}) == E_SHAPE, k
    assert call(f, ok, B=0) == call(f, ok, H=-1) == E_ARG
    for kw in (dict(C=48), dict(C=544), dict(groups=5), dict(groups=0), dict(B=64, C=512, H=128, W=128)):
        assert call(f, ok, **kw) == E_SHAPE, kw
    # ---- the three with a workspace
    nb = L.vkn_gn_relu_bwd_workspace_bytes(2, 32, 3, 7, 8)
    gn = (L.vkn_gn_relu_bwd_f32, dict(dy=p, r=p, stats=p, gamma=p, beta=p, groups=8, dr=p, dgamma=p, dbeta=p, B=2, C=32, H=3, W=7, ws=p, ws_bytes=nb, stream=None),
          ('dy', 'r', 'stats', 'gamma', 'beta', 'dr', 'dgamma', 'dbeta'), (dict(C=48), dict(groups=5), dict(B=64, C=512, H=128, W=128)))
    nb = L.vkn_conv_wgrad_workspace_bytes(2, 32, 3, 7, 64, 3, 1)
    wg = (L.vkn_conv_wgrad_f32, dict(dr=p, x=p, dw=p, B=2, Cin=32, H=3, W=7, Cout=64, ksize=3, stride=1, ws=p, ws_bytes=nb, stream=None),
          ('dr', 'x', 'dw'), (dict(Cin=48), dict(Cout=544), dict(ksize=2), dict(ksize=1, stride=2), dict(stride=3)))
    nb = L.vkn_conv_dgrad_workspace_bytes(2, 64, 3, 7, 1)
    dg = (L.vkn_conv_dgrad_f32, dict(dr=p, wimg_t=p, dx=p, B=2, Cin=32, H=3, W=7, Cout=64, ksize=3, stride=1, ws=p, ws_bytes=nb, stream=None),
          ('dr', 'wimg_t', 'dx'), (dict(Cin=48), dict(Cout=544), dict(ksize=2), dict(ksize=1, stride=2), dict(stride=3)))
    for f, ok, pointers, shapes in (gn, wg, dg):
        for k in pointers:
            assert call(f, ok, **{k: None}) == call(f, ok, **{k: None, 'ws_bytes': 0}) == E_ARG, k                     # ARG speaks first
            assert call(f, ok, **{k: odd}) == E_ALIGN and call(f, ok, **{k: odd, 'ws_bytes': ok['ws_bytes'] - 1}) == E_WORKSPACE, k     # WORKSPACE before ALIGN
        assert call(f, ok, B=0) == call(f, ok, W=-3) == E_ARG
        for kw in shapes:
            assert call(f, ok, **kw) == call(f, ok, ws=None, **kw) == call(f, ok, ws=odd, **kw) == E_SHAPE, kw       # SHAPE before WORKSPACE and ALIGN
        assert call(f, ok, ws=None) == call(f, ok, ws_bytes=ok['ws_bytes'] - 1) == call(f, ok, ws_bytes=0) == E_WORKSPACE
        assert call(f, ok, ws=odd) == call(f, ok, ws=p + 8) == E_ALIGN
