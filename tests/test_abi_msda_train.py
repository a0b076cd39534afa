"""The C ABI of the neck training part include/vkn_msda_train.h, judged as tests/test_abi_msda.py judges its header: a regex reading of
the argument lists, the built library's exports, a C compiler for the header, the workspace size and the refusals in their order.  The
part is bound through a SEVENTH table, `_lib.NECK_TRAIN_HEADERS` / `_lib.ABI_NECK_TRAIN`, and leaves the six tables before it, their
constant records and `_each`'s default as they were."""
import ctypes
import os
import re

import pytest

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_msda_train.h'
SYMBOLS = {'vkn_msda_bwd_workspace_bytes': 7, 'vkn_msda_sample_bwd_f32': 22}
CONSTS = dict(VKN_MSDA_BWD_MAX_QP=1 << 24, VKN_MSDA_BWD_WS_HEAD=1536)
HOST_ARRAY = {'vkn_msda_bwd_workspace_bytes': 0, 'vkn_msda_sample_bwd_f32': 6}           # the position of `shapes`
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def test_the_seventh_table_leaves_the_six_tables_alone(vkn):
    lib = vkn._lib
    assert lib.NECK_TRAIN_HEADERS == (HEADER,) == tuple(lib.ABI_NECK_TRAIN)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.TRAIN_HEADERS == ('vkn_fpn_train.h',) == tuple(lib.ABI_TRAIN) and lib.NECK_HEADERS == ('vkn_msda.h',) == tuple(lib.ABI_NECK)
    part = lib.ABI_NECK_TRAIN[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) == tuple(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN, lib.ABI_NECK)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == CONSTS == lib.MSDA_TRAIN
    assert not set(CONSTS) & (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN) | set(lib.MSDA))
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()} and lib.MSDA == lib.ABI_NECK['vkn_msda.h'].consts
    assert not part.structs and not part.mirrors and 'vkn_msda_bwd.hip' in lib.SOURCES and 'vkn_msda.hip' in lib.SOURCES
    # `_each`'s default is the six tables, as before; the binding loops go over `_bound`: those and the seventh
    assert lib._each('protos') == lib._each('protos', before) and lib._each('protos')[-1][0] == 'vkn_msda.h'
    assert not any(h == HEADER for h, _, _ in lib._each('protos'))
    bound = lib._bound('protos')
    assert bound[:-len(SYMBOLS)] == lib._each('protos') and [(h, n) for h, n, _ in bound[-len(SYMBOLS):]] == [(HEADER, n) for n in SYMBOLS]
    names = [n for _, n, _ in bound]
    assert len(names) == len(set(names))
    # one reading over the seven tables: the part sees vkn.h's codes and vkn_msda.h's limits through its #include
    order = (lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS + lib.NECK_HEADERS
             + lib.NECK_TRAIN_HEADERS)
    every = lib.read_abi(os.path.join(ROOT, 'include'), order)
    assert tuple(every) == order and every[HEADER].protos == part.protos
    assert {h: every[h].protos for h in order[:-1]} == {h: hdr.protos for t in before for h, hdr in t.items()}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), ('vkn.h', HEADER))              # "vkn_msda.h" is not listed before it


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_NECK_TRAIN[HEADER].symbols) == list(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    exported = {n for n in ('vkn_msda_bwd_workspace_bytes', 'vkn_msda_sample_bwd_f32', 'vkn_msda_sample_f32') if hasattr(raw, n)}
    assert exported == set(SYMBOLS) | {'vkn_msda_sample_f32'}
    for name, params in declared:
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith('_workspace_bytes') else ctypes.c_int), name
        assert len(fn.argtypes) == params.count(',') + 1 == SYMBOLS[name], name
        host = lib.POINTER_EXCEPTIONS[(name, 'shapes')]
        assert host == ctypes.POINTER(ctypes.c_int) and fn.argtypes[HOST_ARRAY[name]] is host               # the one HOST array
        assert all(t in (ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t) for i, t in enumerate(fn.argtypes) if i != HOST_ARRAY[name]), name
    fn = L.vkn_msda_sample_bwd_f32
    assert fn.argtypes[0] is ctypes.c_void_p and fn.argtypes[-1] is ctypes.c_void_p and fn.argtypes[-2] is ctypes.c_size_t


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ int shapes[2] = {{2, 3}};\n'
                   '  size_t n = vkn_msda_bwd_workspace_bytes(shapes, 1, 6, 1, 32, 1, 1);\n'
                   '  int rc = vkn_msda_sample_bwd_f32(0, 0, 0, 0, 0, 0, shapes, 0, 0, 0, 0, 0, 0, 1, 6, 1, 32, 1, 1, 0, n, 0);\n'
                   '  return rc == VKN_E_ARG && n > VKN_MSDA_BWD_WS_HEAD && VKN_MSDA_BWD_MAX_QP > VKN_MSDA_MAX_POINTS ? 0 : 1; }\n')
    _compile('c99', src)


def test_workspace_size_and_envelope(vkn):
    L = vkn._lib.lib()
    nb = L.vkn_msda_bwd_workspace_bytes
    al = lambda n: (n + 255) // 256 * 256                                          # noqa: E731
    lv3 = (ctypes.c_int * 6)(2, 3, 4, 5, 7, 9)
    assert nb(lv3, 2, 89, 8, 32, 3, 4) == 1536 + al(8 * 2 * 89 * 8 * 32)            # the header, the power of two, the max partials; int64 [B][S][M][D]
    assert nb(lv3, 2, 5, 8, 32, 3, 4) == nb(lv3, 2, 89, 8, 32, 3, 4)                # Q does not enter the size
    assert nb((ctypes.c_int * 2)(1, 1), 1, 4096, 8, 16, 1, 1) == 1536 + al(8 * 8 * 16) == 1536 + 1024
    assert nb((ctypes.c_int * 2)(1, 3), 1, 7, 1, 32, 1, 1) == 1536 + al(8 * 3 * 32)
    for bad in ((None, 2, 89, 8, 32, 3, 4), (lv3, 0, 89, 8, 32, 3, 4), (lv3, 2, 0, 8, 32, 3, 4), (lv3, 2, 89, 8, 24, 3, 4), (lv3, 2, 89, 16, 32, 3, 4),
                (lv3, 2, 89, 8, 32, 5, 4), (lv3, 2, 89, 8, 32, 3, 9), (lv3, 2, 89, 8, 32, 0, 4), ((ctypes.c_int * 6)(2, 3, 0, 5, 7, 9), 2, 89, 8, 32, 3, 4),
                (lv3, 30000, 89, 8, 32, 3, 4), (lv3, 1, (1 << 24) // 8 + 1, 1, 32, 3, 8)):
        assert nb(*bad) == 0, bad[1:]
    # Q P = 2^24 exactly is inside (with one narrow head, so that no tensor reaches 2^31 bytes); one more query is not
    one = (ctypes.c_int * 2)(2, 3)
    assert nb(one, 1, (1 << 24) // 8, 1, 32, 1, 8) == 1536 + al(8 * 6 * 32) and nb(one, 1, (1 << 24) // 8 + 1, 1, 32, 1, 8) == 0


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / counts <= 0 / a short row stride / an empty level -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the workspace
    -> VKN_E_WORKSPACE, then alignment -> VKN_E_ALIGN: all decided before the library asks the runtime anything (the device pointers
    below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd = 4096, 4096 + 4
    shapes = (ctypes.c_int * 8)(2, 3, 4, 5, 7, 9, 1, 1)
    nb = L.vkn_msda_bwd_workspace_bytes(shapes, 2, 89, 8, 32, 3, 4)
    assert nb > 0
    ok = dict(value=p, off=p, ld_off=192, logits=p, ld_logits=96, ref=p, shapes=shapes, dout=p, dvalue=p, doff=p, ld_doff=192, dlogits=p,
              ld_dlogits=96, B=2, Q=89, M=8, D=32, L=3, P=4, ws=p, ws_bytes=nb, stream=None)

    def call(**kw):
        return L.vkn_msda_sample_bwd_f32(*dict(ok, **kw).values())
    pointers = ('value', 'off', 'logits', 'ref', 'dout', 'dvalue', 'doff', 'dlogits')
    for k in pointers:
        other = 'dvalue' if k != 'dvalue' else 'value'
        assert call(**{k: None}) == call(**{k: None, 'D': 24}) == call(**{k: None, 'ws_bytes': 0}) == call(**{k: None, other: odd}) == E_ARG, k
        assert call(**{k: odd}) == E_ALIGN and call(**{k: odd, 'ws_bytes': nb - 1}) == E_WORKSPACE and call(**{k: odd, 'D': 24}) == E_SHAPE, k
    assert call(shapes=None) == E_ARG
    for kw in (dict(B=0), dict(Q=-1), dict(M=0), dict(D=0), dict(L=0), dict(P=-2), dict(ld_off=191), dict(ld_logits=95), dict(ld_doff=191),
               dict(ld_dlogits=95), dict(ld_doff=0), dict(shapes=(ctypes.c_int * 6)(2, 3, 0, 5, 7, 9)), dict(shapes=(ctypes.c_int * 6)(2, 3, 4, 5, 7, -9)),
               dict(D=24, B=0), dict(ld_dlogits=95, ws=None), dict(ld_doff=191, D=24)):
        assert call(**kw) == E_ARG, kw
    for kw in (dict(D=24), dict(D=8), dict(D=128), dict(M=16, ld_off=384, ld_logits=192, ld_doff=384, ld_dlogits=192), dict(M=5, D=64), dict(L=5, ld_off=320, ld_logits=160, ld_doff=320, ld_dlogits=160),
               dict(P=9, ld_off=432, ld_logits=216, ld_doff=432, ld_dlogits=216), dict(B=1 << 20, Q=1 << 10), dict(Q=1 << 23), dict(B=30000),
               dict(ld_doff=1 << 23), dict(ld_dlogits=1 << 23),
               dict(L=1, ld_off=64, ld_logits=32, shapes=(ctypes.c_int * 2)(1 << 15, 1 << 14))):
        assert call(**kw) == call(**dict(kw, ws=None)) == call(**dict(kw, ws_bytes=0)) == call(**dict(kw, dvalue=odd)) == E_SHAPE, kw
    # Q P > 2^24 with every tensor below 2^31 bytes: only the scatter's own limit refuses
    one = (ctypes.c_int * 2)(2, 3)
    wide = dict(shapes=one, B=1, M=1, D=32, L=1, P=8, ld_off=16, ld_logits=8, ld_doff=16, ld_dlogits=8)
    inside = L.vkn_msda_bwd_workspace_bytes(one, 1, (1 << 24) // 8, 1, 32, 1, 8)
    assert call(**wide, Q=(1 << 24) // 8 + 1, ws_bytes=inside) == call(**wide, Q=(1 << 24) // 8 + 1, ws=None) == E_SHAPE
    assert call(**wide, Q=(1 << 24) // 8, ws_bytes=inside, dvalue=odd) == E_ALIGN and call(**wide, Q=(1 << 24) // 8, ws_bytes=inside - 1) == E_WORKSPACE
    # the workspace: NULL, one byte short, empty; then alignment, the workspace's included
    assert call(ws=None) == call(ws_bytes=nb - 1) == call(ws_bytes=0) == call(ws=None, dvalue=odd) == E_WORKSPACE
    assert call(ws=odd) == call(ws=p + 8) == E_ALIGN
    # both gradients in ONE [B Q][288] buffer: the strides pass, only the pointer is refused
    assert call(ld_doff=288, ld_dlogits=288, ld_off=288, ld_logits=288, dlogits=odd) == E_ALIGN
    for good in (dict(M=4, D=64, ld_off=96, ld_logits=48, ld_doff=96, ld_dlogits=48), dict(M=8, D=16),
                 dict(L=4, P=8, ld_off=512, ld_logits=256, ld_doff=512, ld_dlogits=256)):
        size = L.vkn_msda_bwd_workspace_bytes(shapes, 2, 89, good.get('M', 8), good.get('D', 32), good.get('L', 3), good.get('P', 4))
        assert size > 0 and call(**dict(good, ws_bytes=size, dout=odd)) == E_ALIGN and call(**dict(good, ws_bytes=size - 1)) == E_WORKSPACE, good
