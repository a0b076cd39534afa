"""The C ABI of the windowed metric part include/vkn_vpq.h, judged as tests/test_abi_stq.py judges its header: a regex reading of the
argument lists, the built library's exports, a C compiler for the header and the struct layout, the size probe, the state's layout and
the refusals in their order.  The part is bound through a FOURTH table, `_lib.WINDOW_METRIC_HEADERS` / `_lib.ABI_WINDOW_METRIC`, and
leaves the three tables before it, `_lib.CONSTS`, `_lib.SEG` and `_lib.STQ` as they were."""
import ctypes
import os
import re

import pytest
import torch

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_vpq.h'
SYMBOLS = {'vkn_sizeof_vpq_cfg': 0, 'vkn_vpq_state_bytes': 1, 'vkn_vpq_state_layout': 2, 'vkn_vpq_reset': 4, 'vkn_vpq_update_i32': 10}
FIELDS = ['offset', 'num_cat', 'ign_id', 'label_bit_shift', 'nk', 'ks', 'cap_gt', 'cap_pred', 'cap_pair', 'cap_log']
CONSTS = dict(VKN_VPQ_MAX_KS=4, VKN_VPQ_MAX_K=8, VKN_VPQ_GROUP=8, VKN_VPQ_SPAN_PX=2048, VKN_VPQ_MAX_GRID=512, VKN_VPQ_LDS_SLOTS=2048,
              VKN_VPQ_HEADER_BYTES=256, VKN_VPQ_MAX_CAT=255, VKN_VPQ_MIN_CAP=16, VKN_VPQ_MAX_CAP=1 << 20, VKN_VPQ_STATUS_ID_RANGE=1,
              VKN_VPQ_STATUS_CLASS_RANGE=2, VKN_VPQ_STATUS_FULL_GT=4, VKN_VPQ_STATUS_FULL_PRED=8, VKN_VPQ_STATUS_FULL_PAIR=16,
              VKN_VPQ_STATUS_FULL_LOG=32, VKN_VPQ_STATUS_FULL=60)
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5
STEP = dict(offset=2 ** 30, num_cat=20, ign_id=255, label_bit_shift=16, ks=(1, 2, 4), cap_gt=512, cap_pred=512, cap_pair=2048, cap_log=131072)


def _cfg(lib, **kw):
    a = dict(STEP, **kw)
    ks = tuple(a['ks'])
    a['nk'] = a.get('nk', len(ks))
    a['ks'] = (ctypes.c_int * 4)(*(ks + (0,) * 4)[:4])
    return lib.VknVpqCfg(*[a[f] for f in FIELDS])


def test_the_window_metric_table_leaves_the_three_tables_alone(vkn):
    lib = vkn._lib
    assert lib.WINDOW_METRIC_HEADERS == (HEADER,) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC)
    win = lib.ABI_WINDOW_METRIC[HEADER]
    assert win.path == os.path.join(ROOT, 'include', HEADER) and win.symbols == tuple(win.protos) and set(win.symbols) == set(SYMBOLS)
    others = {s for t in (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC) for h in t.values() for s in h.symbols}
    assert not set(win.symbols) & others
    assert win.consts == CONSTS == lib.VPQ and not set(CONSTS) & (set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ))
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert lib.SEG == lib.ABI_EXT['vkn_seg_loss.h'].consts and lib.STQ == lib.ABI_METRIC['vkn_stq.h'].consts
    assert list(win.structs) == list(win.mirrors) == ['VknVpqCfg'] and lib.VknVpqCfg is win.mirrors['VknVpqCfg']
    assert 'VknVpqCfg' not in lib.MIRRORS and 'VknVpqCfg' not in lib.ABI_METRIC['vkn_stq.h'].mirrors and 'vkn_vpq.hip' in lib.SOURCES
    # the four tables go through the same loops: every prototype, struct and constant of the part is among `_each`'s
    assert {n for h, n, _ in lib._each('protos') if h == HEADER} == set(SYMBOLS) and (HEADER, 'VknVpqCfg') in {(h, n) for h, n, _ in lib._each('mirrors')}
    assert lib.POINTER_EXCEPTIONS[('vkn_vpq_state_layout', 'offsets4')] == ctypes.POINTER(ctypes.c_size_t)
    # one reading over the four tables: the part sees vkn.h's error codes through its #include
    every = lib.read_abi(os.path.join(ROOT, 'include'), lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS)
    assert every[HEADER].protos == win.protos and {h: every[h].protos for h in HEADERS} == {h: lib.ABI[h].protos for h in HEADERS}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_WINDOW_METRIC[HEADER].symbols) and len(declared) == len(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert getattr(raw, name) is not None
        fn = getattr(L, name)
        assert fn.restype in (ctypes.c_int, ctypes.c_size_t), name
        assert len(fn.argtypes) == (0 if params.strip() == 'void' else params.count(',') + 1) == SYMBOLS[name], name
    for name in ('vkn_vpq_state_bytes', 'vkn_vpq_state_layout', 'vkn_vpq_reset', 'vkn_vpq_update_i32'):
        assert getattr(L, name).argtypes[0]._type_ is lib.VknVpqCfg, name
    assert L.vkn_vpq_state_bytes.restype is ctypes.c_size_t and L.vkn_sizeof_vpq_cfg.restype is ctypes.c_size_t
    assert L.vkn_vpq_state_layout.argtypes[1]._type_ is ctypes.c_size_t and L.vkn_vpq_reset.argtypes[2] is ctypes.c_size_t
    # the header cites the reference lines it replaces, and names its two departures
    full = open(os.path.join(ROOT, 'include', HEADER)).read()
    assert full.count('eval_dvpq_step.py:') >= 8 and full.count('eval_dvpq_vipseg.py:') >= 4
    assert 'eval_dvpq_step.py:56' in full and 'eval_dvpq_vipseg.py:441' in full


def test_header_is_c99_on_its_own_and_the_mirror_has_its_layout(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ VknVpqCfg c; c.offset = 1ll << 30; c.ks[VKN_VPQ_MAX_KS - 1] = VKN_VPQ_MAX_K; c.cap_log = VKN_VPQ_MAX_CAP;\n'
                   '  return c.cap_log > VKN_VPQ_SPAN_PX + VKN_VPQ_MAX_GRID + VKN_VPQ_LDS_SLOTS + VKN_VPQ_HEADER_BYTES + VKN_VPQ_MIN_CAP + VKN_VPQ_MAX_CAT'
                   ' + VKN_VPQ_GROUP + c.ks[3] + (int)(VKN_VPQ_STATUS_FULL | VKN_VPQ_STATUS_ID_RANGE | VKN_VPQ_STATUS_CLASS_RANGE) + VKN_E_SHAPE ? 0 : 1; }\n')
    _compile('c99', src)
    m = vkn._lib.VknVpqCfg
    assert [f for f, _ in m._fields_] == FIELDS
    lines = ['#include <stddef.h>', f'#include "include/{HEADER}"', f'_Static_assert(sizeof(VknVpqCfg) == {ctypes.sizeof(m)}, "sizeof");']
    for field, _ in m._fields_:
        f = getattr(m, field)
        lines.append(f'_Static_assert(offsetof(VknVpqCfg, {field}) == {f.offset}, "offsetof {field}");')
        lines.append(f'_Static_assert(sizeof(((VknVpqCfg*)0)->{field}) == {f.size}, "sizeof {field}");')
    assert len(lines) == 3 + 2 * 10
    lay = tmp_path / 'layout.c'
    lay.write_text('\n'.join(lines) + '\n')
    _compile('c11', lay)
    assert vkn._lib.lib().vkn_sizeof_vpq_cfg() == ctypes.sizeof(m) == 56 and m.ks.size == 16 and m.ks.offset == 24


def test_state_bytes_layout_and_envelope(vkn):
    lib = vkn._lib
    L = lib.lib()
    sb = lambda **kw: L.vkn_vpq_state_bytes(ctypes.byref(_cfg(lib, **kw)))          # noqa: E731

    def layout(**kw):
        off = (ctypes.c_size_t * 4)()
        assert L.vkn_vpq_state_layout(ctypes.byref(_cfg(lib, **kw)), off) == 0
        return list(off)
    # header, int64 acc[nk][3][num_cat] (padded to 16 bytes), int64 log[cap_log][4], the private part
    assert layout() == [0, 256, 256 + 3 * 3 * 20 * 8, 256 + 1440 + 131072 * 32]
    # the private part: the frame base, a ring of max(ks) - 1 + GROUP frame tables, GROUP * nk window tables (with pred's ignored overlap)
    slot, window = 16 * (512 + 512 + 2048), 16 * (512 + 512 + 2048) + 8 * 512
    assert sb() == layout()[3] + 16 + (4 - 1 + 8) * slot + 8 * 3 * window
    small = dict(cap_gt=16, cap_pred=16, cap_pair=16, cap_log=16)
    assert layout(num_cat=125, ks=(1, 2, 4, 6), **small) == [0, 256, 256 + 4 * 3 * 125 * 8, 256 + 12000 + 512]
    assert layout(num_cat=3, ign_id=3, ks=(1,), **small) == [0, 256, 256 + 80, 256 + 80 + 512]              # 72 bytes of acc, padded
    assert sb(num_cat=3, ign_id=3, ks=(1,), **small) == 256 + 80 + 512 + 16 + 8 * 768 + 8 * (768 + 128)
    assert sb(ks=(8,), **small) == 256 + 480 + 512 + 16 + 15 * 768 + 8 * (768 + 128)
    assert all(o % 16 == 0 for kw in (dict(), dict(num_cat=3, ign_id=3, ks=(1,)), dict(num_cat=125, ks=(1, 2, 4, 6))) for o in layout(**kw) + [sb(**kw)])
    # the envelope
    for kw in (dict(num_cat=0), dict(num_cat=256), dict(ign_id=19), dict(ign_id=256), dict(label_bit_shift=0), dict(label_bit_shift=31),
               dict(offset=(20 << 16) - 1), dict(offset=(1 << 62) // (256 << 16) + 1), dict(ks=(), nk=0), dict(ks=(1, 2, 4, 6), nk=5), dict(ks=(0, 1)),
               dict(ks=(1, 9)), dict(ks=(2, 2)), dict(ks=(4, 2)), dict(ks=(-1,)), dict(cap_gt=8), dict(cap_pred=24), dict(cap_pair=1 << 21),
               dict(cap_pair=0), dict(cap_gt=-16), dict(cap_log=8), dict(cap_log=48)):
        assert sb(**kw) == 0, kw
        assert L.vkn_vpq_state_layout(ctypes.byref(_cfg(lib, **kw)), (ctypes.c_size_t * 4)()) == E_SHAPE, kw
    for kw in (dict(num_cat=1, ign_id=1, label_bit_shift=1, offset=2), dict(num_cat=255, offset=255 << 16), dict(ign_id=20), dict(offset=20 << 16),
               dict(offset=((1 << 62) - 1) // (256 << 16)), dict(num_cat=1, ign_id=1, label_bit_shift=30, offset=1 << 30), dict(ks=(8,)),
               dict(ks=(1, 2, 4, 6)), dict(ks=(5, 6, 7, 8)), dict(ks=(3, 1, 0, -7), nk=1), dict(cap_gt=16, cap_log=1 << 20)):
        assert sb(**kw) > 0, kw
    assert L.vkn_vpq_state_bytes(None) == 0
    assert L.vkn_vpq_state_layout(None, (ctypes.c_size_t * 4)()) == L.vkn_vpq_state_layout(ctypes.byref(_cfg(lib)), None) == E_ARG


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / negative counts -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the state's size -> VKN_E_WORKSPACE, then alignment
    -> VKN_E_ALIGN: all four are decided before the library asks the runtime anything, so a machine without a GPU sees them (the pointers
    below are never dereferenced)."""
    lib = vkn._lib
    L = lib.lib()
    good = _cfg(lib)
    nbytes = L.vkn_vpq_state_bytes(ctypes.byref(good))
    p, odd4, odd2 = 4096, 4096 + 4, 4096 + 2
    ok = dict(cfg=good, state=p, state_bytes=nbytes, gt_sem=p, gt_ins=p, pred_sem=p, pred_ins=p, B=1, HW=936, stream=None)

    def upd(**kw):
        a = dict(ok, **kw)
        return L.vkn_vpq_update_i32(*[ctypes.byref(a[k]) if k == 'cfg' and a[k] is not None else a[k] for k in ok])

    def rst(cfg=good, state=p, state_bytes=nbytes):
        return L.vkn_vpq_reset(ctypes.byref(cfg) if cfg is not None else None, state, state_bytes, None)
    bad_cfg = _cfg(lib, cap_pair=24)
    for k in ('cfg', 'state', 'gt_sem', 'gt_ins', 'pred_sem', 'pred_ins'):
        assert upd(**{k: None}) == E_ARG, k
        assert upd(**{k: None, 'state_bytes': nbytes + 16, 'B': 0}) == E_ARG, k                                   # ARG speaks first
    assert upd(B=-1) == upd(HW=-1) == E_ARG
    for kw in (dict(cfg=bad_cfg), dict(B=0), dict(HW=0), dict(B=1 << 15, HW=1 << 14), dict(B=1, HW=1 << 29), dict(cfg=_cfg(lib, ks=(2, 1)))):
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
    cfg = _cfg(lib, cap_gt=16, cap_pred=16, cap_pair=16, cap_log=16)
    nbytes = L.vkn_vpq_state_bytes(ctypes.byref(cfg))
    state = torch.full((nbytes,), 0x5A, dtype=torch.uint8, device=dev)
    maps = torch.zeros((4, 12), dtype=torch.int32, device=dev)
    host = (ctypes.c_int * 1024)()
    hp = ctypes.addressof(host)
    hp += (-hp) % 16
    d = lambda t: t.data_ptr()          # noqa: E731
    m = [d(maps[i]) for i in range(4)]
    with torch.cuda.device(dev):
        assert L.vkn_vpq_reset(ctypes.byref(cfg), hp, nbytes, None) == E_ARG
        assert L.vkn_vpq_reset(ctypes.byref(cfg), hp, nbytes + 16, None) == E_WORKSPACE and L.vkn_vpq_reset(ctypes.byref(cfg), hp + 4, nbytes, None) == E_ALIGN
        assert L.vkn_vpq_update_i32(ctypes.byref(cfg), hp, nbytes, *m, 1, 12, None) == E_ARG
        for i in range(4):
            assert L.vkn_vpq_update_i32(ctypes.byref(cfg), d(state), nbytes, *m[:i], hp, *m[i + 1:], 1, 12, None) == E_ARG
        assert L.vkn_vpq_update_i32(ctypes.byref(cfg), d(state), nbytes - 16, hp, *m[1:], 1, 12, None) == E_WORKSPACE
        assert L.vkn_vpq_update_i32(ctypes.byref(cfg), d(state), nbytes, hp + 2, *m[1:], 1, 12, None) == E_ALIGN
    torch.cuda.synchronize()
    assert bool((state == 0x5A).all())


def test_default_capacities_are_those_the_premises_were_proved_for(vkn):
    """tests/test_vpq_refs.py proves that the seeded GPU inputs fit `vpq_ref.DEFAULT_CAPACITY`: that must be what `ops.vpq_cfg` fills in"""
    import vpq_ref
    cfg = vkn.ops.vpq_cfg(20, (1, 2, 4))
    assert dict(gt=cfg.cap_gt, pred=cfg.cap_pred, pair=cfg.cap_pair, log=cfg.cap_log) == vpq_ref.DEFAULT_CAPACITY
    assert (cfg.offset, cfg.num_cat, cfg.ign_id, cfg.label_bit_shift, cfg.nk, list(cfg.ks)) == (2 ** 30, 20, 255, 16, 3, [1, 2, 4, 0])
    with pytest.raises(vkn.VknError):
        vkn.ops.vpq_cfg(20, (2, 1))
    with pytest.raises(vkn.VknError):
        vkn.ops.vpq_cfg(20, (1, 2, 3, 4, 5))
