"""The C ABI of the metric part include/vkn_stq.h, judged as tests/test_abi_seg_loss.py judges its header: a regex reading of the argument
lists, the built library's exports, a C compiler for the header and the struct layout, the size probe, the state's layout and the
refusals in their order.  The part is bound through a THIRD table, `_lib.METRIC_HEADERS` / `_lib.ABI_METRIC`, and leaves
`_lib.ABI_HEADERS`, `_lib.EXTENSION_HEADERS`, `_lib.ABI`, `_lib.ABI_EXT` and `_lib.CONSTS` as they were."""
import ctypes
import os
import re

import pytest
import torch

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_stq.h'
SYMBOLS = {'vkn_sizeof_stq_cfg': 0, 'vkn_stq_state_bytes': 1, 'vkn_stq_state_layout': 2, 'vkn_stq_reset': 4, 'vkn_stq_update_i32': 11}
FIELDS = ['offset', 'num_classes', 'ignore_label', 'label_bit_shift', 'drop_ignored_gt', 'cap_gt', 'cap_pred', 'cap_pair']
CONSTS = dict(VKN_STQ_SPAN_PX=2048, VKN_STQ_MAX_GRID=512, VKN_STQ_LDS_SLOTS=2048, VKN_STQ_HEADER_BYTES=256, VKN_STQ_MAX_CLASSES=255, VKN_STQ_MIN_CAP=16,
              VKN_STQ_MAX_CAP=1 << 20, VKN_STQ_STATUS_ID_RANGE=1, VKN_STQ_STATUS_CLASS_RANGE=2, VKN_STQ_STATUS_FULL_GT=4,
              VKN_STQ_STATUS_FULL_PRED=8, VKN_STQ_STATUS_FULL_PAIR=16, VKN_STQ_STATUS_FULL=28)
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
KITTI = dict(offset=2 ** 16 * 256, num_classes=19, ignore_label=255, label_bit_shift=16, drop_ignored_gt=1, cap_gt=2048, cap_pred=8192, cap_pair=32768)


def _cfg(lib, **kw):
    a = dict(KITTI, **kw)
    return lib.VknStqCfg(*[a[f] for f in FIELDS])


def test_the_metric_table_leaves_the_two_tables_alone(vkn):
    lib = vkn._lib
    assert lib.METRIC_HEADERS == (HEADER,) == tuple(lib.ABI_METRIC)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    met = lib.ABI_METRIC[HEADER]
    assert met.path == os.path.join(ROOT, 'include', HEADER) and met.symbols == tuple(met.protos) and set(met.symbols) == set(SYMBOLS)
    others = {s for t in (lib.ABI, lib.ABI_EXT) for h in t.values() for s in h.symbols}
    assert not set(met.symbols) & others
    assert met.consts == CONSTS == lib.STQ and not set(CONSTS) & set(lib.CONSTS) and not set(CONSTS) & set(lib.SEG)
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert lib.SEG == lib.ABI_EXT['vkn_seg_loss.h'].consts
    assert list(met.structs) == list(met.mirrors) == ['VknStqCfg'] and lib.VknStqCfg is met.mirrors['VknStqCfg']
    assert 'VknStqCfg' not in lib.MIRRORS and 'VknStqCfg' not in lib.ABI_EXT['vkn_seg_loss.h'].mirrors and 'vkn_stq.hip' in lib.SOURCES
    # one reading over the three tables: the part sees vkn.h's error codes through its #include
    every = lib.read_abi(os.path.join(ROOT, 'include'), lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS)
    assert every[HEADER].protos == met.protos and {h: every[h].protos for h in HEADERS} == {h: lib.ABI[h].protos for h in HEADERS}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_METRIC[HEADER].symbols) and len(declared) == len(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert getattr(raw, name) is not None
        fn = getattr(L, name)
        assert fn.restype in (ctypes.c_int, ctypes.c_size_t), name
        assert len(fn.argtypes) == (0 if params.strip() == 'void' else params.count(',') + 1) == SYMBOLS[name], name
    for name in ('vkn_stq_state_bytes', 'vkn_stq_state_layout', 'vkn_stq_reset', 'vkn_stq_update_i32'):
        assert getattr(L, name).argtypes[0]._type_ is lib.VknStqCfg, name
    assert L.vkn_stq_state_bytes.restype is ctypes.c_size_t and L.vkn_sizeof_stq_cfg.restype is ctypes.c_size_t
    assert L.vkn_stq_state_layout.argtypes[1]._type_ is ctypes.c_size_t and L.vkn_stq_reset.argtypes[2] is ctypes.c_size_t
    # the header cites the reference lines it replaces
    assert open(os.path.join(ROOT, 'include', HEADER)).read().count('STQ.py:') >= 4


def test_header_is_c99_on_its_own_and_the_mirror_has_its_layout(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ VknStqCfg c; c.offset = 1ll << 40; c.cap_pair = VKN_STQ_MAX_CAP;\n'
                   '  return c.cap_pair > VKN_STQ_SPAN_PX + VKN_STQ_MAX_GRID + VKN_STQ_LDS_SLOTS + VKN_STQ_HEADER_BYTES + VKN_STQ_MIN_CAP + VKN_STQ_MAX_CLASSES'
                   ' + (int)(VKN_STQ_STATUS_FULL | VKN_STQ_STATUS_ID_RANGE | VKN_STQ_STATUS_CLASS_RANGE) + VKN_E_SHAPE ? 0 : 1; }\n')
    _compile('c99', src)
    m = vkn._lib.VknStqCfg
    assert [f for f, _ in m._fields_] == FIELDS
    lines = ['#include <stddef.h>', f'#include "include/{HEADER}"', f'_Static_assert(sizeof(VknStqCfg) == {ctypes.sizeof(m)}, "sizeof");']
    for field, _ in m._fields_:
        f = getattr(m, field)
        lines.append(f'_Static_assert(offsetof(VknStqCfg, {field}) == {f.offset}, "offsetof {field}");')
        lines.append(f'_Static_assert(sizeof(((VknStqCfg*)0)->{field}) == {f.size}, "sizeof {field}");')
    assert len(lines) == 3 + 2 * 8
    lay = tmp_path / 'layout.c'
    lay.write_text('\n'.join(lines) + '\n')
    _compile('c11', lay)
    assert vkn._lib.lib().vkn_sizeof_stq_cfg() == ctypes.sizeof(m) == 40


def test_state_bytes_layout_and_envelope(vkn):
    lib = vkn._lib
    L = lib.lib()
    sb = lambda **kw: L.vkn_stq_state_bytes(ctypes.byref(_cfg(lib, **kw)))          # noqa: E731

    def layout(**kw):
        off = (ctypes.c_size_t * 8)()
        assert L.vkn_stq_state_layout(ctypes.byref(_cfg(lib, **kw)), off) == 0
        return list(off)
    # header, n x n int64 (padded to 16 bytes), then keys and counts of gt, pred, pair
    assert layout() == [0, 256, 256 + 3200, 256 + 3200 + 16384, 256 + 3200 + 32768, 256 + 3200 + 32768 + 65536, 256 + 3200 + 32768 + 131072,
                        256 + 3200 + 32768 + 131072 + 262144]
    assert sb() == 256 + 3200 + 16 * (2048 + 8192 + 32768)
    small = dict(cap_gt=16, cap_pred=16, cap_pair=16)
    # n: ignore_label >= num_classes -> num_classes + 1 (an odd n pads the matrix to 16 bytes), else num_classes
    assert sb(num_classes=5, ignore_label=2, **small) == 256 + 208 + 768 and layout(num_classes=5, ignore_label=2, **small)[2] == 256 + 208
    assert sb(num_classes=6, ignore_label=6, **small) == 256 + 400 + 768 and sb(num_classes=6, ignore_label=7, **small) == 256 + 400 + 768
    assert sb(num_classes=124, ignore_label=200, label_bit_shift=16) == 256 + (125 * 125 * 8 + 8) + 16 * (2048 + 8192 + 32768)
    assert all(o % 16 == 0 for kw in (dict(), dict(num_classes=5, ignore_label=2), dict(num_classes=6, ignore_label=6)) for o in layout(**kw))
    # the envelope
    for kw in (dict(num_classes=0), dict(num_classes=256), dict(label_bit_shift=0), dict(label_bit_shift=31), dict(offset=(19 << 16) - 1),
               dict(offset=(1 << 62) // (20 << 16) + 1), dict(cap_gt=8), dict(cap_pred=24), dict(cap_pair=1 << 21), dict(cap_pair=0), dict(cap_gt=-16)):
        assert sb(**kw) == 0, kw
        assert L.vkn_stq_state_layout(ctypes.byref(_cfg(lib, **kw)), (ctypes.c_size_t * 8)()) == E_SHAPE, kw
    for kw in (dict(num_classes=1, label_bit_shift=1, offset=2), dict(num_classes=255, offset=255 << 16), dict(num_classes=1, label_bit_shift=30, offset=1 << 30), dict(offset=19 << 16),
               dict(offset=((1 << 62) - 1) // (20 << 16)), dict(cap_gt=16, cap_pred=1 << 20), dict(ignore_label=-1), dict(drop_ignored_gt=0)):
        assert sb(**kw) > 0, kw
    assert L.vkn_stq_state_bytes(None) == 0
    assert L.vkn_stq_state_layout(None, (ctypes.c_size_t * 8)()) == L.vkn_stq_state_layout(ctypes.byref(_cfg(lib)), None) == E_ARG


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / negative counts -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the state's size -> VKN_E_WORKSPACE, then alignment
    -> VKN_E_ALIGN: all four are decided before the library asks the runtime anything, so a machine without a GPU sees them (the pointers
    below are never dereferenced)."""
    lib = vkn._lib
    L = lib.lib()
    good = _cfg(lib)
    nbytes = L.vkn_stq_state_bytes(ctypes.byref(good))
    p, odd4, odd2 = 4096, 4096 + 4, 4096 + 2
    ok = dict(cfg=good, state=p, state_bytes=nbytes, is_thing=p, gt_sem=p, gt_ins=p, pred_sem=p, pred_ins=p, B=1, HW=936, stream=None)

    def upd(**kw):
        a = dict(ok, **kw)
        return L.vkn_stq_update_i32(*[ctypes.byref(a[k]) if k == 'cfg' and a[k] is not None else a[k] for k in ok])

    def rst(cfg=good, state=p, state_bytes=nbytes):
        return L.vkn_stq_reset(ctypes.byref(cfg) if cfg is not None else None, state, state_bytes, None)
    bad_cfg = _cfg(lib, cap_pair=24)
    for k in ('cfg', 'state', 'is_thing', 'gt_sem', 'gt_ins', 'pred_sem', 'pred_ins'):
        assert upd(**{k: None}) == E_ARG, k
        assert upd(**{k: None, 'state_bytes': nbytes + 16, 'B': 0}) == E_ARG, k                                   # ARG speaks first
    assert upd(B=-1) == upd(HW=-1) == E_ARG
    for kw in (dict(cfg=bad_cfg), dict(B=0), dict(HW=0), dict(B=1 << 15, HW=1 << 14), dict(B=1, HW=1 << 29), dict(cfg=_cfg(lib, num_classes=256))):
        assert upd(**kw) == E_SHAPE, kw
        assert upd(gt_sem=None, **kw) == E_ARG and upd(state_bytes=nbytes - 16, **kw) == E_SHAPE and upd(state=odd4, **kw) == E_SHAPE, kw
    for d in (-16, 16, -8, 1):
        assert upd(state_bytes=nbytes + d) == E_WORKSPACE and upd(state_bytes=nbytes + d, state=odd4) == E_WORKSPACE, d     # WORKSPACE before ALIGN
        assert upd(state_bytes=nbytes + d, gt_ins=odd2) == E_WORKSPACE
    assert upd(state=odd4) == upd(state=4096 + 8) == E_ALIGN                                # the state: 16 bytes
    for k in ('gt_sem', 'gt_ins', 'pred_sem', 'pred_ins'):
        assert upd(**{k: odd2}) == E_ALIGN, k                                               # the maps: 4 bytes only
    assert rst(cfg=None) == rst(state=None) == E_ARG
    assert rst(cfg=bad_cfg) == rst(cfg=bad_cfg, state_bytes=0) == rst(cfg=bad_cfg, state=odd4) == E_SHAPE and rst(cfg=bad_cfg, state=None) == E_ARG
    assert rst(state_bytes=nbytes - 16) == rst(state_bytes=nbytes + 16) == rst(state_bytes=nbytes + 16, state=odd4) == E_WORKSPACE
    assert rst(state=odd4) == E_ALIGN


@pytest.mark.gpu
def test_host_pointers_are_refused_last_and_nothing_is_launched(vkn):
    """With a device present: a HOST pointer where device memory is expected is VKN_E_ARG, after shape, size and alignment had their say."""
    lib = vkn._lib
    L = lib.lib()
    dev = torch.device('cuda:0')
    cfg = _cfg(lib, cap_gt=16, cap_pred=16, cap_pair=16)
    nbytes = L.vkn_stq_state_bytes(ctypes.byref(cfg))
    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    thing = torch.zeros((20,), dtype=torch.uint8, device=dev)
    maps = torch.zeros((4, 12), dtype=torch.int32, device=dev)
    host = (ctypes.c_int * 1024)()
    hp = ctypes.addressof(host)
    hp += (-hp) % 16
    d = lambda t: t.data_ptr()          # noqa: E731
    m = [d(maps[i]) for i in range(4)]
    with torch.cuda.device(dev):
        assert L.vkn_stq_reset(ctypes.byref(cfg), hp, nbytes, None) == E_ARG
        assert L.vkn_stq_reset(ctypes.byref(cfg), hp, nbytes + 16, None) == E_WORKSPACE and L.vkn_stq_reset(ctypes.byref(cfg), hp + 4, nbytes, None) == E_ALIGN
        assert L.vkn_stq_update_i32(ctypes.byref(cfg), hp, nbytes, d(thing), *m, 1, 12, None) == E_ARG
        assert L.vkn_stq_update_i32(ctypes.byref(cfg), d(state), nbytes, hp, *m, 1, 12, None) == E_ARG
        for i in range(4):
            assert L.vkn_stq_update_i32(ctypes.byref(cfg), d(state), nbytes, d(thing), *m[:i], hp, *m[i + 1:], 1, 12, None) == E_ARG
        assert L.vkn_stq_update_i32(ctypes.byref(cfg), d(state), nbytes - 16, d(thing), hp, *m[1:], 1, 12, None) == E_WORKSPACE
        assert L.vkn_stq_update_i32(ctypes.byref(cfg), d(state), nbytes, d(thing), hp + 2, *m[1:], 1, 12, None) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all())
