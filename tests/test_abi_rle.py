"""The C ABI of the result part include/vkn_rle.h, judged as tests/test_abi_stq.py judges its header: a regex reading of the argument
lists, the built library's exports, a C compiler for the header, the workspace size and the refusals in their order.  The part is bound
through an EIGHTH table, `_lib.RESULT_HEADERS` / `_lib.ABI_RESULT`, and leaves the seven tables before it, their constant records,
`_each`'s default and `_bound` as they were."""
import ctypes
import os
import re

import pytest
import torch

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_rle.h'
SYMBOLS = {'vkn_rle_workspace_bytes': 3, 'vkn_rle_encode_u8': 13, 'vkn_rle_encode_f32': 14}
CONSTS = dict(VKN_RLE_STRIP_COLS=64, VKN_RLE_MAX_K=1024, VKN_RLE_MAX_RUN_BYTES=7, VKN_RLE_LAUNCHES=8, VKN_RLE_RECORD_INTS=9, VKN_RLE_REC_NRUNS=0,
              VKN_RLE_REC_RUN_OFF=1, VKN_RLE_REC_NBYTES=2, VKN_RLE_REC_BYTE_OFF=3, VKN_RLE_REC_AREA=4, VKN_RLE_REC_BBOX=5,
              VKN_RLE_STATUS_FULL_RUNS=1, VKN_RLE_STATUS_FULL_BYTES=2, VKN_RLE_STATUS_FULL=3)
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def _ws(K, H, W):
    """the workspace as include/vkn_rle.h and csrc/vkn_rle.hip lay it out: the masks as bits, two states and one statistics record per
    strip, two words per strip, two per mask; every part padded to 16 bytes"""
    up16 = lambda n: (n + 15) // 16 * 16          # noqa: E731
    strips = K * ((W + 63) // 64)
    return up16(strips * H * 8) + 2 * 16 * strips + 32 * strips + 2 * up16(4 * strips) + up16(8 * K)


def test_the_eighth_table_leaves_the_seven_tables_alone(vkn):
    lib = vkn._lib
    assert lib.RESULT_HEADERS == (HEADER,) == tuple(lib.ABI_RESULT)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.TRAIN_HEADERS == ('vkn_fpn_train.h',) == tuple(lib.ABI_TRAIN) and lib.NECK_HEADERS == ('vkn_msda.h',) == tuple(lib.ABI_NECK)
    assert lib.NECK_TRAIN_HEADERS == ('vkn_msda_train.h',) == tuple(lib.ABI_NECK_TRAIN)
    part = lib.ABI_RESULT[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) == tuple(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN, lib.ABI_NECK, lib.ABI_NECK_TRAIN)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == CONSTS == lib.RLE
    assert not set(CONSTS) & (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN) | set(lib.MSDA) | set(lib.MSDA_TRAIN))
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()} and lib.MSDA_TRAIN == lib.ABI_NECK_TRAIN['vkn_msda_train.h'].consts
    assert not part.structs and not part.mirrors and 'vkn_rle.hip' in lib.SOURCES
    # `_each`'s default is the six tables and `_bound` the seven, as before; the binding loops go over `_every`: those and the eighth
    assert lib._each('protos') == lib._each('protos', before[:6]) and lib._bound('protos') == lib._each('protos', before)
    assert not any(h == HEADER for h, _, _ in lib._bound('protos'))
    every = lib._every('protos')
    assert every[:-len(SYMBOLS)] == lib._bound('protos') and [(h, n) for h, n, _ in every[-len(SYMBOLS):]] == [(HEADER, n) for n in SYMBOLS]
    names = [n for _, n, _ in every]
    assert len(names) == len(set(names))
    # one reading over the eight tables: the part sees vkn.h's error codes through its #include
    order = (lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS + lib.NECK_HEADERS
             + lib.NECK_TRAIN_HEADERS + lib.RESULT_HEADERS)
    read = lib.read_abi(os.path.join(ROOT, 'include'), order)
    assert tuple(read) == order and read[HEADER].protos == part.protos
    assert {h: read[h].protos for h in order[:-1]} == {h: hdr.protos for t in before for h, hdr in t.items()}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    full = open(os.path.join(ROOT, 'include', HEADER)).read()
    text = re.sub(r'/\*.*?\*/', ' ', full, flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_RESULT[HEADER].symbols) == list(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    # the library exports what the header declares, and no other vkn_rle_* name
    exported = {n for n in (*SYMBOLS, 'vkn_rle_encode', 'vkn_rle_encode_f16', 'vkn_rle_decode', 'vkn_rle_sizeof') if hasattr(raw, n)}
    assert exported == set(SYMBOLS)
    for name, params in declared:
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith('_workspace_bytes') else ctypes.c_int), name
        assert len(fn.argtypes) == params.count(',') + 1 == SYMBOLS[name], name
    u8, f32 = L.vkn_rle_encode_u8.argtypes, L.vkn_rle_encode_f32.argtypes
    assert f32[1] is ctypes.c_float and list(f32[:1] + f32[2:]) == list(u8)                 # one-to-one but for `thr`
    assert u8[0] is ctypes.c_void_p and list(u8[1:4]) == [ctypes.c_int] * 3 and u8[-2] is ctypes.c_size_t and u8[-1] is ctypes.c_void_p
    assert L.vkn_rle_workspace_bytes.argtypes == [ctypes.c_int] * 3
    # the header cites what it replaces and where the format is documented, and states the format
    assert 'external/test.py:55-70' in full and 'tools_vis/apis/test.py:36,80' in full and 'external/ext/mask.py:10-15' in full
    assert 'p = x * H + y' in full and 'more = (c & 16) ? (x != -1) : (x != 0)' in full


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ size_t n = vkn_rle_workspace_bytes(1, 2, 3);\n'
                   '  int rc = vkn_rle_encode_u8(0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0, n, 0) + vkn_rle_encode_f32(0, 0.5f, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0, n, 0);\n'
                   '  return rc == 2 * VKN_E_ARG && VKN_RLE_RECORD_INTS == VKN_RLE_REC_BBOX + 4 && VKN_RLE_STRIP_COLS + VKN_RLE_MAX_K + VKN_RLE_MAX_RUN_BYTES'
                   ' + VKN_RLE_LAUNCHES + VKN_RLE_REC_NRUNS + VKN_RLE_REC_RUN_OFF + VKN_RLE_REC_NBYTES + VKN_RLE_REC_BYTE_OFF + VKN_RLE_REC_AREA'
                   ' > (int)(VKN_RLE_STATUS_FULL | VKN_RLE_STATUS_FULL_RUNS | VKN_RLE_STATUS_FULL_BYTES) ? 0 : 1; }\n')
    _compile('c99', src)


def test_workspace_size_and_envelope(vkn):
    nb = vkn._lib.lib().vkn_rle_workspace_bytes
    for shape in ((1, 1, 1), (1, 37, 63), (1, 37, 64), (1, 37, 65), (3, 37, 131), (100, 720, 1280), (100, 384, 1248), (20, 1024, 2048), (1, 4099, 1),
                  (1, 1080, 1920), (1024, 1, 1), (7, 45, 80)):
        assert nb(*shape) == _ws(*shape) > 0, shape
    assert nb(100, 720, 1280) == 100 * 20 * 720 * 8 + 64 * 2000 + 2 * 8000 + 800            # the masks as bits are all but 0.15 MB of it
    # the envelope: 1 <= K <= 1024, H, W >= 1, H * W < 2^31, K * H * W < 2^31
    for bad in ((0, 4, 4), (1025, 4, 4), (-1, 4, 4), (1, 0, 4), (1, 4, 0), (1, -4, 4), (1, 4, -4), (1, 1 << 16, 1 << 15), (1, 1 << 15, 1 << 16),
                (2, 1 << 15, 1 << 15), (1024, 1 << 11, 1 << 10), (1, (1 << 31) - 1, 2)):
        assert nb(*bad) == 0, bad
    for good in ((1, (1 << 31) - 1, 1), (1, 1, (1 << 31) - 1), (1023, 1 << 11, 1 << 10), (1, 1 << 15, (1 << 16) - 1)):
        assert nb(*good) == _ws(*good) > 0, good


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / negative counts -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the workspace's size -> VKN_E_WORKSPACE, then
    alignment -> VKN_E_ALIGN: all four are decided before the library asks the runtime anything, so a machine without a GPU sees them
    (the pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd4, odd8 = 4096, 4096 + 4, 4096 + 8
    K, H, W = 3, 37, 131
    nb = L.vkn_rle_workspace_bytes(K, H, W)
    ok = dict(masks=p, K=K, H=H, W=W, records=p, runs=p, cap_runs=100, bytes=p, cap_bytes=100, status=p, ws=p, ws_bytes=nb, stream=None)

    def u8(**kw):
        return L.vkn_rle_encode_u8(*dict(ok, **kw).values())

    def f32(**kw):
        a = dict(ok, **kw)
        return L.vkn_rle_encode_f32(a.pop('masks'), 0.5, *a.values())
    for call in (u8, f32):
        for k in ('masks', 'records', 'runs', 'bytes', 'status', 'ws'):
            other = 'runs' if k != 'runs' else 'bytes'
            assert call(**{k: None}) == call(**{k: None, 'K': 0}) == call(**{k: None, 'ws_bytes': 0}) == call(**{k: None, other: odd4}) == E_ARG, k   # ARG speaks first
        for kw in (dict(K=-1), dict(H=-1), dict(W=-1), dict(cap_runs=-1), dict(cap_bytes=-1), dict(K=-1, H=0), dict(cap_runs=-1, ws_bytes=0)):
            assert call(**kw) == E_ARG, kw
        for kw in (dict(K=0), dict(K=1025), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(K=2, H=1 << 15, W=1 << 15)):
            assert call(**kw) == call(ws_bytes=0, **kw) == call(runs=odd4, **kw) == E_SHAPE, kw
            assert call(records=None, **kw) == E_ARG, kw
        for d in (-16, 16, -1, 1):
            assert call(ws_bytes=nb + d) == call(ws_bytes=nb + d, runs=odd4) == call(ws_bytes=nb + d, status=4096 + 2) == E_WORKSPACE, d   # WORKSPACE before ALIGN
        assert call(ws_bytes=0) == E_WORKSPACE
        for k in ('masks', 'records', 'runs', 'bytes', 'ws'):
            assert call(**{k: odd4}) == call(**{k: odd8}) == E_ALIGN, k                    # 16 bytes
        assert call(status=4096 + 2) == E_ALIGN and call(status=4096 + 1) == E_ALIGN       # the status word: 4 bytes
        assert call(cap_runs=0, cap_bytes=0, masks=odd4) == E_ALIGN                        # empty pools are capacities like any other
    # the element size enters the envelope: K H W < 2^31 <= 4 K H W is the u8 entry's alone
    big = dict(K=1, H=1 << 15, W=1 << 14, ws_bytes=L.vkn_rle_workspace_bytes(1, 1 << 15, 1 << 14))
    assert big['ws_bytes'] > 0 and u8(masks=odd4, **big) == E_ALIGN and f32(masks=odd4, **big) == f32(**dict(big, ws_bytes=0)) == E_SHAPE


@pytest.mark.gpu
def test_host_pointers_are_refused_last_and_nothing_is_launched(vkn):
    """With a device present: a HOST pointer where device memory is expected is VKN_E_ARG, after shape, size and alignment had their say."""
    lib = vkn._lib
    L = lib.lib()
    dev = torch.device('cuda:0')
    K, H, W = 2, 5, 7
    nb = L.vkn_rle_workspace_bytes(K, H, W)
    masks = torch.ones((K, H, W), dtype=torch.uint8, device=dev)
    logits = torch.ones((K, H, W), dtype=torch.float32, device=dev)
    outs = {k: torch.full((n,), 0x5A, dtype=torch.uint8, device=dev) for k, n in (('records', 4 * 9 * K), ('runs', 400), ('bytes', 100), ('status', 4), ('ws', nb))}
    host = (ctypes.c_int * 4096)()
    hp = ctypes.addressof(host)
    hp += (-hp) % 16
    names = ('records', 'runs', 'bytes', 'status', 'ws')

    def call(f32=False, masks_ptr=None, **kw):
        a = {k: outs[k].data_ptr() for k in names}
        a.update(kw)
        src = masks_ptr or (logits if f32 else masks).data_ptr()
        tail = (K, H, W, a['records'], a['runs'], 100, a['bytes'], 100, a['status'], a['ws'], kw.get('ws_bytes', nb), None)
        return L.vkn_rle_encode_f32(src, 0.5, *tail) if f32 else L.vkn_rle_encode_u8(src, *tail)
    with torch.cuda.device(dev):
        for f32 in (False, True):
            assert call(f32, masks_ptr=hp) == E_ARG
            for k in names:
                assert call(f32, **{k: hp}) == E_ARG, k
            assert call(f32, runs=hp, ws_bytes=nb + 16) == E_WORKSPACE and call(f32, runs=hp + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in outs.values())
