"""The C ABI of the neck part include/vkn_msda.h, judged as tests/test_abi_fpn_train.py judges its header: a regex reading of the
argument list, the built library's export, a C compiler for the header and the refusals in their order.  The part is bound through a
SIXTH table, `_lib.NECK_HEADERS` / `_lib.ABI_NECK`, and leaves the five tables before it and their constant records as they were."""
import ctypes
import os
import re

import pytest

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_msda.h'
SYMBOLS = {'vkn_msda_sample_f32': 15}
CONSTS = dict(VKN_MSDA_MAX_LEVELS=4, VKN_MSDA_MAX_POINTS=8, VKN_MSDA_MAX_CHANNELS=256)
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -5


def test_the_neck_table_leaves_the_five_tables_alone(vkn):
    lib = vkn._lib
    assert lib.NECK_HEADERS == (HEADER,) == tuple(lib.ABI_NECK)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.TRAIN_HEADERS == ('vkn_fpn_train.h',) == tuple(lib.ABI_TRAIN)
    part = lib.ABI_NECK[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) and set(part.symbols) == set(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == CONSTS == lib.MSDA
    assert not set(CONSTS) & (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN))
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert lib.SEG == lib.ABI_EXT['vkn_seg_loss.h'].consts and lib.STQ == lib.ABI_METRIC['vkn_stq.h'].consts
    assert lib.VPQ == lib.ABI_WINDOW_METRIC['vkn_vpq.h'].consts and lib.FPN_TRAIN == lib.ABI_TRAIN['vkn_fpn_train.h'].consts
    assert not part.structs and not part.mirrors and 'vkn_msda.hip' in lib.SOURCES
    # the six tables go through the same loops: the part's prototype is among `_each`'s default, after the five
    each = lib._each('protos')
    assert {n for h, n, _ in each if h == HEADER} == set(SYMBOLS) and each[-1][0] == HEADER
    assert each[:-len(SYMBOLS)] == lib._each('protos', before)
    names = [n for _, n, _ in each]
    assert len(names) == len(set(names))
    # one reading over the six tables: the part sees vkn.h's error codes through its #include, and declares nothing in vkn.h
    every = lib.read_abi(os.path.join(ROOT, 'include'), lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS
                         + lib.TRAIN_HEADERS + lib.NECK_HEADERS)
    assert every[HEADER].protos == part.protos and {h: every[h].protos for h in HEADERS} == {h: lib.ABI[h].protos for h in HEADERS}
    assert not any(n.startswith('vkn_msda') for t in before for h in t.values() for n in h.protos)
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it


def test_header_is_exported_with_its_own_argument_list(vkn):
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_NECK[HEADER].symbols) and len(declared) == len(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert getattr(raw, name) is not None
        fn = getattr(L, name)
        assert fn.restype is ctypes.c_int and len(fn.argtypes) == params.count(',') + 1 == SYMBOLS[name], name
        host = lib.POINTER_EXCEPTIONS[(name, 'shapes')]
        assert host == ctypes.POINTER(ctypes.c_int) and fn.argtypes[6] is host                            # the one HOST array
        assert all(t in (ctypes.c_void_p, ctypes.c_int) for i, t in enumerate(fn.argtypes) if i != 6), name
        assert fn.argtypes[-1] is ctypes.c_void_p and fn.argtypes[0] is ctypes.c_void_p, name            # device pointers travel as integers; stream last


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ int shapes[2] = {{2, 3}};\n'
                   '  int rc = vkn_msda_sample_f32(0, 0, 0, 0, 0, 0, shapes, 0, 1, 1, 1, 32, 1, 1, 0);\n'
                   '  return rc == VKN_E_ARG && VKN_MSDA_MAX_LEVELS * VKN_MSDA_MAX_POINTS * 3 <= VKN_MSDA_MAX_CHANNELS ? 0 : 1; }\n')
    _compile('c99', src)


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / counts <= 0 / a short row stride / an empty level -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then alignment ->
    VKN_E_ALIGN: all decided before the library asks the runtime anything (the device pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd = 4096, 4096 + 4
    shapes = (ctypes.c_int * 8)(2, 3, 4, 5, 7, 9, 1, 1)

    def call(**kw):
        ok = dict(value=p, off=p, ld_off=192, logits=p, ld_logits=96, ref=p, shapes=shapes, out=p, B=2, Q=89, M=8, D=32, L=3, P=4, stream=None)
        return L.vkn_msda_sample_f32(*dict(ok, **kw).values())
    for k in ('value', 'off', 'logits', 'ref', 'out'):
        other = 'out' if k != 'out' else 'value'
        assert call(**{k: None}) == call(**{k: None, 'D': 24}) == call(**{k: None, other: odd}) == E_ARG, k     # ARG speaks first
        assert call(**{k: odd}) == E_ALIGN and call(**{k: odd, 'D': 24}) == E_SHAPE, k                   # SHAPE before ALIGN
    assert call(shapes=None) == E_ARG
    for kw in (dict(B=0), dict(Q=-1), dict(M=0), dict(D=0), dict(L=0), dict(P=-2), dict(ld_off=191), dict(ld_logits=95), dict(ld_off=0),
               dict(shapes=(ctypes.c_int * 6)(2, 3, 0, 5, 7, 9)), dict(shapes=(ctypes.c_int * 6)(2, 3, 4, 5, 7, -9)), dict(D=24, B=0)):
        assert call(**kw) == E_ARG, kw
    assert call(ld_off=288, ld_logits=288, out=odd) == E_ALIGN                                           # the strides of one [B Q][288] GEMM output pass
    for kw in (dict(D=24), dict(D=8), dict(D=128), dict(M=1, D=16, ld_off=24, ld_logits=12), dict(M=16, D=32, ld_off=384, ld_logits=192),
               dict(M=5, D=64, ld_off=120, ld_logits=60), dict(L=5, ld_off=320, ld_logits=160), dict(P=9, ld_off=432, ld_logits=216),
               dict(B=1 << 20, Q=1 << 10), dict(Q=1 << 23), dict(B=30000),
               dict(L=1, ld_off=64, ld_logits=32, shapes=(ctypes.c_int * 2)(1 << 15, 1 << 14))):
        assert call(**kw) == call(**dict(kw, out=odd)) == E_SHAPE, kw
    for ok in (dict(M=4, D=64, ld_off=96, ld_logits=48), dict(M=8, D=16), dict(M=2, D=16, ld_off=48, ld_logits=24), dict(L=4, P=8, ld_off=512, ld_logits=256)):
        assert call(**dict(ok, out=odd)) == E_ALIGN, ok                                                   # inside the envelope: only the pointer is refused
