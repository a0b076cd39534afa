"""The C ABI of the backbone training part include/vkn_wattn_train.h, judged as tests/test_abi_swin.py and tests/test_abi_msda_train.py judge
their headers: a regex reading of the argument lists, the built library's exports, a C compiler for the header, the envelope with the exact
workspace size and the refusals in their order.  The part is bound through a TWELFTH table, `_lib.BACKBONE_TRAIN_HEADERS` /
`_lib.ABI_BACKBONE_TRAIN`, and leaves the eleven tables before it, their constant records and `_all_tables` as they were."""
import ctypes
import os
import re

import pytest

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_wattn_train.h'
SYMBOLS = {'vkn_wattn_bwd_supported': 6, 'vkn_wattn_bwd_workspace_bytes': 5, 'vkn_wattn_bwd_f32': 17}
CONSTS = dict(VKN_WATTN_PART_FLOATS=64, VKN_WATTN_MERGE_SLICES=16, VKN_WATTN_WS_ALIGN=256)
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def _bytes(B, H, W, heads, ws):
    """the header's rule for the workspace, restated"""
    windows = B * (-(-H // ws)) * (-(-W // ws))
    return (4 * windows * heads * (2 * ws - 1) ** 2 + 255) // 256 * 256 + 4 * windows * heads * 64


def test_the_twelfth_table_leaves_the_eleven_tables_alone(vkn):
    lib = vkn._lib
    assert lib.BACKBONE_TRAIN_HEADERS == (HEADER,) == tuple(lib.ABI_BACKBONE_TRAIN)
    assert lib.BACKBONE_HEADERS == ('vkn_swin.h',) == tuple(lib.ABI_BACKBONE) and lib.ABI_HEADERS == HEADERS == tuple(lib.ABI)
    part = lib.ABI_BACKBONE_TRAIN[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) == tuple(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN, lib.ABI_NECK, lib.ABI_NECK_TRAIN, lib.ABI_RESULT, lib.ABI_INSTANCE_METRIC,
              lib.ABI_INSTANCE_RESULT, lib.ABI_BACKBONE)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == CONSTS == lib.WATTN_TRAIN and all(k.startswith('VKN_WATTN_') for k in part.consts)
    others = (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN) | set(lib.MSDA) | set(lib.MSDA_TRAIN) | set(lib.RLE) | set(lib.MASKAP)
              | set(lib.INSTMASK) | set(lib.SWIN))
    assert not set(part.consts) & others
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()} and lib.SWIN == lib.ABI_BACKBONE['vkn_swin.h'].consts
    assert not part.structs and not part.mirrors and 'vkn_swin_bwd.hip' in lib.SOURCES and 'vkn_swin.hip' in lib.SOURCES
    # `_all_tables` is the eleven tables, as before; the binding loops go over `_all_abi`: those and the twelfth
    assert lib._all_tables('protos') == lib._each('protos', before) and lib._all_parts('protos') == lib._each('protos', before[:10])
    assert not any(h == HEADER for h, _, _ in lib._all_tables('protos'))
    bound = lib._all_abi('protos')
    assert bound[:-len(SYMBOLS)] == lib._all_tables('protos') and [(h, n) for h, n, _ in bound[-len(SYMBOLS):]] == [(HEADER, n) for n in SYMBOLS]
    names = [n for _, n, _ in bound]
    assert len(names) == len(set(names))
    order = (lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS + lib.NECK_HEADERS
             + lib.NECK_TRAIN_HEADERS + lib.RESULT_HEADERS + lib.INSTANCE_METRIC_HEADERS + lib.INSTANCE_RESULT_HEADERS + lib.BACKBONE_HEADERS
             + lib.BACKBONE_TRAIN_HEADERS)
    read = lib.read_abi(os.path.join(ROOT, 'include'), order)
    assert tuple(read) == order and read[HEADER].protos == part.protos
    assert {h: read[h].protos for h in order[:-1]} == {h: hdr.protos for t in before for h, hdr in t.items()}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), ('vkn.h', HEADER))              # "vkn_swin.h" is not listed before it
    assert re.findall(r'#include "([^"]+)"', open(part.path).read()) == ['vkn_swin.h']


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    full = open(os.path.join(ROOT, 'include', HEADER)).read()
    text = re.sub(r'/\*.*?\*/', ' ', full, flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_BACKBONE_TRAIN[HEADER].symbols) == list(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith('_workspace_bytes') else ctypes.c_int), name
        assert len(fn.argtypes) == params.count(',') + 1 == SYMBOLS[name], name
    out = os.popen(f'nm -D --defined-only {lib.LIBPATH}').read()
    assert set(re.findall(r'\b(vkn_wattn\w*)\b', out)) == set(SYMBOLS)
    bwd = L.vkn_wattn_bwd_f32
    assert list(bwd.argtypes) == [ctypes.c_void_p] * 7 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_void_p]
    assert L.vkn_wattn_bwd_supported.argtypes == [ctypes.c_int] * 6 and L.vkn_wattn_bwd_workspace_bytes.argtypes == [ctypes.c_int] * 5
    assert 'pad tokens ONLY' in full and 'No float atomics' in full and 'Nothing of the forward is saved' in full
    # the ops of the binding, the autograd function and the module's switch
    assert callable(vkn.ops.swin_window_attention_bwd) and callable(vkn.ops.swin_window_attention_bwd_supported)
    assert callable(vkn.autograd.swin_window_attention) and issubclass(vkn.autograd.SwinWindowAttnFn, __import__('torch').autograd.Function)


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ int ok = vkn_wattn_bwd_supported(1, 7, 7, 4, 7, 3);\n'
                   '  size_t n = vkn_wattn_bwd_workspace_bytes(1, 7, 7, 4, 7);\n'
                   '  int rc = vkn_wattn_bwd_f32(0, 0, 0, 0, 0, 0, 0, 1, 7, 7, 4, 7, 3, 0.5f, 0, n, 0);\n'
                   '  return ok && rc == VKN_E_ARG && n > 0 && VKN_WATTN_PART_FLOATS == 2 * VKN_SWIN_HEAD_DIM && VKN_WATTN_MERGE_SLICES > 0\n'
                   '    && VKN_WATTN_WS_ALIGN % 16 == 0 ? 0 : 1; }\n')
    _compile('c99', src)


def test_envelope_and_workspace_size(vkn):
    L = vkn._lib.lib()
    sup, fwd, nb = L.vkn_wattn_bwd_supported, L.vkn_swin_window_attn_supported, L.vkn_wattn_bwd_workspace_bytes
    # every shipped stage: Swin-B and Swin-L, a KITTI-STEP and a COCO frame, both arms, B = 1 and 2 (the 64 of tests/test_abi_swin.py)
    count = 0
    for maps in (((96, 312), (48, 156), (24, 78), (12, 39)), ((200, 336), (100, 168), (50, 84), (25, 42))):
        for heads in ((4, 8, 16, 32), (6, 12, 24, 48)):
            for (H, W), nh in zip(maps, heads):
                for B in (1, 2):
                    for shift in (0, 3):
                        assert sup(B, H, W, nh, 7, shift) == 1 and nb(B, H, W, nh, 7) == _bytes(B, H, W, nh, 7) > 0, (B, H, W, nh)
                        count += 1
    assert count == 64
    assert nb(1, 7, 7, 1, 7) == 768 + 256 and nb(1, 10, 17, 3, 7) == _bytes(1, 10, 17, 3, 7) == (4 * 6 * 3 * 169 + 255) // 256 * 256 + 4 * 6 * 3 * 64
    for ws in range(1, 9):
        assert all(sup(1, 5, 9, 2, ws, s) == 1 for s in range(ws)) and sup(1, 5, 9, 2, ws, ws) == sup(1, 5, 9, 2, ws, -1) == 0
        assert nb(1, 5, 9, 2, ws) == _bytes(1, 5, 9, 2, ws)
    assert sup(1, 5, 9, 1, 8, 7) == sup(1, 5, 9, 64, 8, 7) == sup(1, 1, 1, 1, 1, 0) == 1 and nb(1, 1, 1, 1, 1) == 256 + 256
    # every bad value; the size is 0 exactly outside the envelope (the shift does not enter it)
    for bad in ((0, 5, 9, 2, 7, 0), (1, 0, 9, 2, 7, 0), (1, 5, 0, 2, 7, 0), (1, 5, 9, 0, 7, 0), (1, 5, 9, 65, 7, 0), (1, 5, 9, 2, 0, 0), (1, 5, 9, 2, 9, 0), (-1, 5, 9, 2, 7, 0),
                (1, -5, 9, 2, 7, 0), (1, 5, 9, 2, -7, 0), (1, 1 << 16, 1 << 16, 1, 7, 0), (1 << 30, 1 << 16, 1 << 16, 1, 7, 0), (1 << 20, 64, 64, 3, 7, 0)):
        assert sup(*bad) == 0 and nb(*bad[:5]) == 0, bad
    for shape in ((1, 5, 9, 2, 7), (2, 200, 336, 4, 7), (1, 1, 1, 1, 1), (1, 5, 9, 64, 8), (1, 5, 9, 65, 8), (1, 5, 9, 2, 9), (0, 5, 9, 2, 7)):
        assert (nb(*shape) > 0) == bool(sup(*shape, 0)), shape
    # the sizes: inside the forward's envelope the workspace stays below qkv, so both envelopes end at the same token
    tokens = ((1 << 31) - 1) // (3 * 4 * 32 * 4)
    assert sup(1, 1, tokens, 4, 7, 0) == 1 and sup(1, 1, tokens + 1, 4, 7, 0) == 0 and sup(2, 1, tokens // 2 + 1, 4, 7, 0) == 0
    assert 0 < nb(1, 1, tokens, 4, 7) == _bytes(1, 1, tokens, 4, 7) < 1 << 31
    for shape in ((1, 1, tokens, 4, 1, 0), (1, 1, tokens, 4, 2, 1), (1, 1, tokens, 4, 8, 4), (1, tokens, 1, 4, 8, 0)):
        assert sup(*shape) == fwd(*shape) == 1 and nb(*shape[:5]) == _bytes(*shape[:5]) < 1 << 31, shape


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / counts <= 0 / a bias without its gradient or the reverse -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the
    workspace -> VKN_E_WORKSPACE, then alignment -> VKN_E_ALIGN: all decided before the library asks the runtime anything (the pointers
    below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd4, odd8 = 4096, 4096 + 4, 4096 + 8
    nb = L.vkn_wattn_bwd_workspace_bytes(1, 10, 17, 3, 7)
    assert nb > 0
    ok = dict(qkv=p, qkv_bias=p, bias_table=p, dout=p, dqkv=p, dqkv_bias=p, dbias_table=p, B=1, H=10, W=17, heads=3, window=7, shift=3, scale=0.5,
              ws=p, ws_bytes=nb, stream=None)

    def bwd(**kw):
        return L.vkn_wattn_bwd_f32(*dict(ok, **kw).values())
    for k in ('qkv', 'bias_table', 'dout', 'dqkv', 'dbias_table'):
        assert bwd(**{k: None}) == bwd(**{k: None, 'heads': 65}) == bwd(**{k: None, 'ws_bytes': 0}) == bwd(**{k: None, 'qkv_bias': odd4}) == E_ARG, k
    for k in ('B', 'H', 'W', 'heads'):
        assert bwd(**{k: 0}) == bwd(**{k: -1}) == bwd(**{k: 0, 'window': 9}) == bwd(**{k: 0, 'ws': None}) == E_ARG, k
    # the bias and its gradient come together or not at all
    assert bwd(qkv_bias=None) == bwd(dqkv_bias=None) == bwd(qkv_bias=None, window=9) == bwd(dqkv_bias=None, ws_bytes=0) == bwd(dqkv_bias=None, dqkv=odd4) == E_ARG
    for kw in (dict(heads=65), dict(window=0), dict(window=-7), dict(window=9), dict(shift=7), dict(shift=-1), dict(window=3, shift=3), dict(B=1 << 20, H=64, W=64)):
        assert bwd(**kw) == bwd(dqkv=odd4, **kw) == bwd(ws=None, **kw) == bwd(ws_bytes=0, **kw) == bwd(qkv_bias=None, dqkv_bias=None, **kw) == E_SHAPE, kw
    assert bwd(ws=None) == bwd(ws_bytes=nb - 1) == bwd(ws_bytes=0) == bwd(ws=None, dqkv=odd4) == bwd(ws_bytes=nb - 1, dout=odd8) == E_WORKSPACE
    assert bwd(qkv_bias=None, dqkv_bias=None, ws_bytes=nb - 1) == E_WORKSPACE                      # the size does not depend on the bias
    for k in ('qkv', 'qkv_bias', 'bias_table', 'dout', 'dqkv', 'dqkv_bias', 'dbias_table', 'ws'):
        assert bwd(**{k: odd4}) == bwd(**{k: odd8}) == E_ALIGN, k
    assert bwd(qkv_bias=None, dqkv_bias=None, dqkv=odd4) == E_ALIGN and bwd(ws_bytes=nb + 1, dout=odd4) == E_ALIGN
