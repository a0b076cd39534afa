"""The C ABI of the backbone part include/vkn_swin.h, judged as tests/test_abi_instmask.py judges its header: a regex reading of the
argument lists, the built library's exports, a C compiler for the header, the envelope and the refusals in their order.  The part is bound
through an ELEVENTH table, `_lib.BACKBONE_HEADERS` / `_lib.ABI_BACKBONE`, and leaves the ten tables before it, their constant records,
`_each`'s default, `_bound`, `_every`, `_all_bound` and `_all_parts` as they were."""
import ctypes
import os
import re

import pytest

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_swin.h'
SYMBOLS = {'vkn_swin_window_attn_supported': 6, 'vkn_swin_window_attn_f32': 12}
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -5


def test_the_eleventh_table_leaves_the_ten_tables_alone(vkn):
    lib = vkn._lib
    assert lib.BACKBONE_HEADERS == (HEADER,) == tuple(lib.ABI_BACKBONE)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.TRAIN_HEADERS == ('vkn_fpn_train.h',) == tuple(lib.ABI_TRAIN) and lib.NECK_HEADERS == ('vkn_msda.h',) == tuple(lib.ABI_NECK)
    assert lib.NECK_TRAIN_HEADERS == ('vkn_msda_train.h',) == tuple(lib.ABI_NECK_TRAIN) and lib.RESULT_HEADERS == ('vkn_rle.h',) == tuple(lib.ABI_RESULT)
    assert lib.INSTANCE_METRIC_HEADERS == ('vkn_maskap.h',) == tuple(lib.ABI_INSTANCE_METRIC)
    assert lib.INSTANCE_RESULT_HEADERS == ('vkn_instmask.h',) == tuple(lib.ABI_INSTANCE_RESULT)
    part = lib.ABI_BACKBONE[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) == tuple(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN, lib.ABI_NECK, lib.ABI_NECK_TRAIN, lib.ABI_RESULT, lib.ABI_INSTANCE_METRIC,
              lib.ABI_INSTANCE_RESULT)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == lib.SWIN and all(k.startswith('VKN_SWIN_') for k in part.consts)
    assert part.consts == dict(VKN_SWIN_HEAD_DIM=32, VKN_SWIN_MAX_WINDOW_TOKENS=64, VKN_SWIN_MAX_WINDOW=8, VKN_SWIN_MAX_HEADS=64, VKN_SWIN_MASK=-100)
    others = (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN) | set(lib.MSDA) | set(lib.MSDA_TRAIN) | set(lib.RLE) | set(lib.MASKAP)
              | set(lib.INSTMASK))
    assert not set(part.consts) & others
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert lib.INSTMASK == lib.ABI_INSTANCE_RESULT['vkn_instmask.h'].consts and lib.MASKAP == lib.ABI_INSTANCE_METRIC['vkn_maskap.h'].consts
    assert not part.structs and not part.mirrors and 'vkn_swin.hip' in lib.SOURCES
    # the five loops of the ten tables are what they were; the binding loops go over `_all_tables`: those and the eleventh
    assert lib._each('protos') == lib._each('protos', before[:6]) and lib._bound('protos') == lib._each('protos', before[:7])
    assert lib._every('protos') == lib._each('protos', before[:8]) and lib._all_bound('protos') == lib._each('protos', before[:9])
    assert lib._all_parts('protos') == lib._each('protos', before)
    assert not any(h == HEADER for h, _, _ in lib._all_parts('protos'))
    bound = lib._all_tables('protos')
    assert bound[:-len(SYMBOLS)] == lib._all_parts('protos') and [(h, n) for h, n, _ in bound[-len(SYMBOLS):]] == [(HEADER, n) for n in SYMBOLS]
    names = [n for _, n, _ in bound]
    assert len(names) == len(set(names))
    order = (lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS + lib.NECK_HEADERS
             + lib.NECK_TRAIN_HEADERS + lib.RESULT_HEADERS + lib.INSTANCE_METRIC_HEADERS + lib.INSTANCE_RESULT_HEADERS + lib.BACKBONE_HEADERS)
    read = lib.read_abi(os.path.join(ROOT, 'include'), order)
    assert tuple(read) == order and read[HEADER].protos == part.protos
    assert {h: read[h].protos for h in order[:-1]} == {h: hdr.protos for t in before for h, hdr in t.items()}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))            # "vkn.h" is not listed before it
    assert re.findall(r'#include "([^"]+)"', open(part.path).read()) == ['vkn.h']


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    full = open(os.path.join(ROOT, 'include', HEADER)).read()
    text = re.sub(r'/\*.*?\*/', ' ', full, flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_BACKBONE[HEADER].symbols) == list(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == params.count(',') + 1 == SYMBOLS[name], name
    out = os.popen(f'nm -D --defined-only {lib.LIBPATH}').read()
    assert set(re.findall(r'\b(vkn_swin\w*)\b', out)) == set(SYMBOLS)
    attn = L.vkn_swin_window_attn_f32
    assert list(attn.argtypes) == [ctypes.c_void_p] * 4 + [ctypes.c_int] * 6 + [ctypes.c_float, ctypes.c_void_p]
    assert L.vkn_swin_window_attn_supported.argtypes == [ctypes.c_int] * 6
    assert 'swin/swin_transformer.py:79-180' in full and 'not -inf' in full and 'Not built: a backward' in full
    # the op of the binding and the module that calls it
    assert callable(vkn.ops.swin_window_attention) and callable(vkn.ops.swin_window_attention_supported)


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ int ok = vkn_swin_window_attn_supported(1, 7, 7, 4, 7, 3);\n'
                   '  int rc = vkn_swin_window_attn_f32(0, 0, 0, 0, 1, 7, 7, 4, 7, 3, 0.5f, 0);\n'
                   '  return ok && rc == VKN_E_ARG && VKN_SWIN_HEAD_DIM * VKN_SWIN_MAX_HEADS > VKN_SWIN_MAX_WINDOW_TOKENS\n'
                   '    && VKN_SWIN_MAX_WINDOW * VKN_SWIN_MAX_WINDOW == VKN_SWIN_MAX_WINDOW_TOKENS && VKN_SWIN_MASK < 0 ? 0 : 1; }\n')
    _compile('c99', src)


def test_envelope(vkn):
    sup = vkn._lib.lib().vkn_swin_window_attn_supported
    # every shipped stage: Swin-B and Swin-L, a KITTI-STEP and a COCO frame, both arms, B = 1 and 2
    for maps in (((96, 312), (48, 156), (24, 78), (12, 39)), ((200, 336), (100, 168), (50, 84), (25, 42))):
        for heads in ((4, 8, 16, 32), (6, 12, 24, 48)):
            for (H, W), nh in zip(maps, heads):
                for B in (1, 2):
                    assert sup(B, H, W, nh, 7, 0) == sup(B, H, W, nh, 7, 3) == 1, (B, H, W, nh)
    for ws in range(1, 9):
        assert all(sup(1, 5, 9, 2, ws, s) == 1 for s in range(ws)) and sup(1, 5, 9, 2, ws, ws) == sup(1, 5, 9, 2, ws, -1) == 0
    assert sup(1, 5, 9, 1, 8, 7) == sup(1, 5, 9, 64, 8, 7) == sup(1, 1, 1, 1, 1, 0) == 1
    for bad in ((0, 5, 9, 2, 7, 0), (1, 0, 9, 2, 7, 0), (1, 5, 0, 2, 7, 0), (1, 5, 9, 0, 7, 0), (1, 5, 9, 65, 7, 0), (1, 5, 9, 2, 0, 0), (1, 5, 9, 2, 9, 0), (-1, 5, 9, 2, 7, 0)):
        assert sup(*bad) == 0, bad
    # every tensor below 2^31 bytes: qkv, 3 heads 32 floats a token, is the largest
    tokens = ((1 << 31) - 1) // (3 * 4 * 32 * 4)              # of 4 heads: the most that stay below
    assert sup(1, 1, tokens, 4, 7, 0) == 1 and sup(1, 1, tokens + 1, 4, 7, 0) == 0 and sup(2, 1, tokens // 2 + 1, 4, 7, 0) == 0
    assert sup(1, 1 << 16, 1 << 16, 1, 7, 0) == 0 and sup(1 << 30, 1 << 16, 1 << 16, 1, 7, 0) == 0


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / counts <= 0 -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then alignment -> VKN_E_ALIGN: all three are decided
    before the library asks the runtime anything (the pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd4, odd8 = 4096, 4096 + 4, 4096 + 8
    ok = dict(qkv=p, qkv_bias=p, bias_table=p, out=p, B=1, H=10, W=17, heads=3, window=7, shift=3, scale=0.5, stream=None)

    def attn(**kw):
        return L.vkn_swin_window_attn_f32(*dict(ok, **kw).values())
    for k in ('qkv', 'bias_table', 'out'):
        assert attn(**{k: None}) == attn(**{k: None, 'heads': 65}) == attn(**{k: None, 'qkv_bias': odd4}) == E_ARG, k
    for k in ('B', 'H', 'W', 'heads'):
        assert attn(**{k: 0}) == attn(**{k: -1}) == attn(**{k: 0, 'window': 9}) == E_ARG, k
    for kw in (dict(heads=65), dict(window=0), dict(window=-7), dict(window=9), dict(shift=7), dict(shift=-1), dict(window=3, shift=3), dict(B=1 << 20, H=64, W=64)):
        assert attn(**kw) == attn(out=odd4, **kw) == attn(qkv_bias=None, **kw) == E_SHAPE, kw
    for k in ('qkv', 'qkv_bias', 'bias_table', 'out'):
        assert attn(**{k: odd4}) == attn(**{k: odd8}) == E_ALIGN, k
    assert attn(qkv_bias=None, out=odd4) == E_ALIGN
