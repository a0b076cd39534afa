"""The C ABI of the instance metric part include/vkn_maskap.h, judged as tests/test_abi_rle.py judges its header: a regex reading of the
argument lists, the built library's exports, a C compiler for the header, the sizes and the refusals in their order.  The part is bound
through a NINTH table, `_lib.INSTANCE_METRIC_HEADERS` / `_lib.ABI_INSTANCE_METRIC`, and leaves the eight tables before it, their constant
records, `_each`'s default, `_bound` and `_every` as they were."""
import ctypes
import os
import re

import pytest
import torch

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_maskap.h'
SYMBOLS = {'vkn_mask_overlap_workspace_bytes': 4, 'vkn_mask_overlap_u8': 12, 'vkn_mask_overlap_f32': 13, 'vkn_sizeof_mask_ap_cfg': 1,
           'vkn_mask_ap_state_bytes': 1, 'vkn_mask_ap_state_layout': 2, 'vkn_mask_ap_reset': 4, 'vkn_mask_ap_match': 16}
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def _ws(K, G, H, W):
    up16 = lambda n: (n + 15) // 16 * 16          # noqa: E731
    strips = (W + 63) // 64
    return up16(8 * K * strips * H) + up16(8 * G * strips * H)


def _cfg(vkn, num_classes=3, T=10, A=4, max_det=100, cap=64):
    return vkn.ops.mask_ap_cfg(num_classes, [0.5 + 0.05 * i for i in range(T)], [(0.0, 1e10), (0.0, 1024.0), (1024.0, 9216.0), (9216.0, 1e10)][:A], max_det, cap)


def test_the_ninth_table_leaves_the_eight_tables_alone(vkn):
    lib = vkn._lib
    assert lib.INSTANCE_METRIC_HEADERS == (HEADER,) == tuple(lib.ABI_INSTANCE_METRIC)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.TRAIN_HEADERS == ('vkn_fpn_train.h',) == tuple(lib.ABI_TRAIN) and lib.NECK_HEADERS == ('vkn_msda.h',) == tuple(lib.ABI_NECK)
    assert lib.NECK_TRAIN_HEADERS == ('vkn_msda_train.h',) == tuple(lib.ABI_NECK_TRAIN) and lib.RESULT_HEADERS == ('vkn_rle.h',) == tuple(lib.ABI_RESULT)
    part = lib.ABI_INSTANCE_METRIC[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) == tuple(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN, lib.ABI_NECK, lib.ABI_NECK_TRAIN, lib.ABI_RESULT)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == lib.MASKAP and all(k.startswith('VKN_MASKAP_') for k in part.consts)
    assert dict(VKN_MASKAP_MAX_MASKS=1024, VKN_MASKAP_MAX_CLASSES=256, VKN_MASKAP_MAX_THRS=16, VKN_MASKAP_MAX_AREAS=4, VKN_MASKAP_RECORD_INTS=12,
                VKN_MASKAP_REC_WORDS=4, VKN_MASKAP_STATUS_FULL=1, VKN_MASKAP_STATUS_LABEL_RANGE=2, VKN_MASKAP_STATUS_SCORE_NAN=4).items() <= part.consts.items()
    others = set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN) | set(lib.MSDA) | set(lib.MSDA_TRAIN) | set(lib.RLE)
    assert not set(part.consts) & others
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()} and lib.RLE == lib.ABI_RESULT['vkn_rle.h'].consts
    assert list(part.structs) == ['VknMaskApCfg'] == list(part.mirrors) and part.mirrors['VknMaskApCfg'] is lib.VknMaskApCfg
    assert 'VknMaskApCfg' not in lib.MIRRORS and 'vkn_maskap.hip' in lib.SOURCES and 'vkn_rle.hip' in lib.SOURCES
    # `_each`'s default is the six tables, `_bound` the seven and `_every` the eight, as before; the binding loops go over `_all_bound`
    assert lib._each('protos') == lib._each('protos', before[:6]) and lib._bound('protos') == lib._each('protos', before[:7])
    assert lib._every('protos') == lib._each('protos', before) and not any(h == HEADER for h, _, _ in lib._every('protos'))
    bound = lib._all_bound('protos')
    assert bound[:-len(SYMBOLS)] == lib._every('protos') and [(h, n) for h, n, _ in bound[-len(SYMBOLS):]] == [(HEADER, n) for n in SYMBOLS]
    names = [n for _, n, _ in bound]
    assert len(names) == len(set(names))
    order = (lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS + lib.NECK_HEADERS
             + lib.NECK_TRAIN_HEADERS + lib.RESULT_HEADERS + lib.INSTANCE_METRIC_HEADERS)
    read = lib.read_abi(os.path.join(ROOT, 'include'), order)
    assert tuple(read) == order and read[HEADER].protos == part.protos
    assert {h: read[h].protos for h in order[:-1]} == {h: hdr.protos for t in before for h, hdr in t.items()}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it
    # the header needs vkn.h alone: not the encoder's
    assert re.findall(r'#include "([^"]+)"', open(part.path).read()) == ['vkn.h']


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    full = open(os.path.join(ROOT, 'include', HEADER)).read()
    text = re.sub(r'/\*.*?\*/', ' ', full, flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_INSTANCE_METRIC[HEADER].symbols) == list(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith('_bytes') or name.startswith('vkn_sizeof') else ctypes.c_int), name
        assert len(fn.argtypes) == (0 if params.strip() == 'void' else params.count(',') + 1) == (SYMBOLS[name] if params.strip() != 'void' else 0), name
    # the exports equal the declarations: no other vkn_mask_overlap_* / vkn_mask_ap_* name, and no vkn_rle_* name beyond the encoder's three
    out = os.popen(f'nm -D --defined-only {lib.LIBPATH}').read()
    exported = set(re.findall(r'\b(vkn_mask_overlap\w*|vkn_mask_ap\w*|vkn_sizeof_mask_ap\w*|vkn_maskap\w*|vkn_rle_\w+)\b', out))
    assert exported == set(SYMBOLS) | {'vkn_rle_workspace_bytes', 'vkn_rle_encode_u8', 'vkn_rle_encode_f32'}
    u8, f32 = L.vkn_mask_overlap_u8.argtypes, L.vkn_mask_overlap_f32.argtypes
    assert f32[1] is ctypes.c_float and list(f32[:1] + f32[2:]) == list(u8)                 # one-to-one but for `thr`
    assert L.vkn_mask_overlap_workspace_bytes.argtypes == [ctypes.c_int] * 4
    assert L.vkn_mask_ap_state_layout.argtypes[1] is ctypes.POINTER(ctypes.c_size_t)
    assert L.vkn_sizeof_mask_ap_cfg() == ctypes.sizeof(lib.VknMaskApCfg) == 8 * (16 + 4 + 4) + 4 * 6
    # the header cites what it replaces and states the rules
    assert 'external/cityscape_panoptic.py:453-568' in full and 'best = min(t, 1 - 1e-10)' in full and 'I = 0 gives iou 0' in full
    assert "argsort(-score, kind='mergesort')" in full and 'Not built: bbox IoU' in full


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ VknMaskApCfg cfg; size_t n = vkn_mask_overlap_workspace_bytes(1, 1, 2, 3);\n'
                   '  int rc = vkn_mask_overlap_u8(0, 0, 1, 1, 2, 3, 0, 0, 0, 0, n, 0) + vkn_mask_overlap_f32(0, 0.5f, 0, 1, 1, 2, 3, 0, 0, 0, 0, n, 0)\n'
                   '    + vkn_mask_ap_reset(0, 0, vkn_mask_ap_state_bytes(0), 0) + vkn_mask_ap_state_layout(0, 0)\n'
                   '    + vkn_mask_ap_match(0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 7, 0, 0);\n'
                   '  cfg.T = VKN_MASKAP_MAX_THRS; cfg.A = VKN_MASKAP_MAX_AREAS; cfg.iou_thrs[cfg.T - 1] = cfg.area_lo[cfg.A - 1] = cfg.area_hi[0] = 0.5;\n'
                   '  return rc == 5 * VKN_E_ARG && sizeof cfg == vkn_sizeof_mask_ap_cfg() && VKN_MASKAP_RECORD_INTS == VKN_MASKAP_REC_WORDS + 2 * VKN_MASKAP_MAX_AREAS\n'
                   '    && VKN_MASKAP_REC_IMAGE + VKN_MASKAP_REC_LABEL + VKN_MASKAP_REC_SCORE + VKN_MASKAP_REC_RANK + VKN_MASKAP_ROW_RUN + VKN_MASKAP_DT_TILE\n'
                   '    + VKN_MASKAP_GT_TILE + VKN_MASKAP_GT_CHUNK + VKN_MASKAP_HEADER_BYTES + VKN_MASKAP_MAX_MASKS + VKN_MASKAP_MAX_CLASSES\n'
                   '    > (int)(VKN_MASKAP_STATUS_FULL | VKN_MASKAP_STATUS_LABEL_RANGE | VKN_MASKAP_STATUS_SCORE_NAN) ? 0 : 1; }\n')
    _compile('c99', src)


def test_sizes_and_envelopes(vkn):
    L = vkn._lib.lib()
    nb = L.vkn_mask_overlap_workspace_bytes
    for shape in ((1, 1, 1, 1), (3, 2, 5, 63), (3, 2, 5, 64), (3, 2, 5, 65), (3, 2, 5, 131), (100, 20, 800, 1344), (100, 10, 720, 1280), (0, 7, 37, 131), (7, 0, 37, 131),
                  (1024, 1024, 1, 1), (1, 1, (1 << 31) - 1, 1), (1, 1, 1, (1 << 31) - 1)):
        assert nb(*shape) == _ws(*shape) > 0, shape
    assert nb(0, 0, 5, 7) == 0                                              # nothing to do: no workspace
    for bad in ((-1, 1, 4, 4), (1, -1, 4, 4), (1025, 1, 4, 4), (1, 1025, 4, 4), (1, 1, 0, 4), (1, 1, 4, 0), (1, 1, -4, 4), (1, 1, 1 << 16, 1 << 15), (2, 1, 1 << 15, 1 << 15),
                (1, 2, 1 << 15, 1 << 15)):
        assert nb(*bad) == 0, bad
    cfg = _cfg(vkn)
    off = (ctypes.c_size_t * 3)()
    assert L.vkn_mask_ap_state_layout(ctypes.byref(cfg), off) == 0 and list(off) == [0, 256, 256 + 3 * 4 * 8]
    assert L.vkn_mask_ap_state_bytes(ctypes.byref(cfg)) == 256 + 96 + 64 * 48
    one = _cfg(vkn, num_classes=1, T=1, A=1, max_det=1, cap=1)
    assert L.vkn_mask_ap_state_bytes(ctypes.byref(one)) == 256 + 16 + 48
    for kw in (dict(num_classes=0), dict(num_classes=257), dict(max_det=0), dict(max_det=1025), dict(cap=0), dict(cap=(1 << 24) + 1)):
        with pytest.raises(vkn.VknError):
            _cfg(vkn, **kw)
    for T, A in ((0, 4), (17, 4), (10, 0)):
        with pytest.raises(vkn.VknError):
            vkn.ops.mask_ap_cfg(3, [0.5] * T, [(0.0, 1.0)] * A, 100, 64)
    with pytest.raises(vkn.VknError):
        vkn.ops.mask_ap_cfg(3, [float('nan')], [(0.0, 1.0)], 100, 64)
    bad = _cfg(vkn)
    bad.T = 17
    assert L.vkn_mask_ap_state_bytes(ctypes.byref(bad)) == 0 and L.vkn_mask_ap_state_layout(ctypes.byref(bad), off) == E_SHAPE
    assert L.vkn_mask_ap_state_bytes(None) == 0 and L.vkn_mask_ap_state_layout(ctypes.byref(cfg), None) == E_ARG


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / negative counts -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the size -> VKN_E_WORKSPACE, then alignment ->
    VKN_E_ALIGN: all four are decided before the library asks the runtime anything (the pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd4, odd8 = 4096, 4096 + 4, 4096 + 8
    K, G, H, W = 3, 2, 37, 131
    nb = L.vkn_mask_overlap_workspace_bytes(K, G, H, W)
    ok = dict(dt=p, gt=p, K=K, G=G, H=H, W=W, inter=p, area_dt=p, area_gt=p, ws=p, ws_bytes=nb, stream=None)

    def u8(**kw):
        return L.vkn_mask_overlap_u8(*dict(ok, **kw).values())

    def f32(**kw):
        a = dict(ok, **kw)
        return L.vkn_mask_overlap_f32(a.pop('dt'), 0.5, *a.values())
    for call in (u8, f32):
        for k in ('dt', 'gt', 'inter', 'area_dt', 'area_gt', 'ws'):
            other = 'inter' if k != 'inter' else 'ws'
            assert call(**{k: None}) == call(**{k: None, 'H': 0}) == call(**{k: None, 'ws_bytes': 0}) == call(**{k: None, other: odd4}) == E_ARG, k
        for kw in (dict(K=-1), dict(G=-1), dict(H=-1), dict(W=-1), dict(K=-1, H=0)):
            assert call(**kw) == E_ARG, kw
        for kw in (dict(K=1025), dict(G=1025), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15), dict(K=2, H=1 << 15, W=1 << 15)):
            assert call(**kw) == call(ws_bytes=0, **kw) == call(inter=odd4, **kw) == E_SHAPE, kw
        for d in (-16, 16, -1, 1):
            assert call(ws_bytes=nb + d) == call(ws_bytes=nb + d, inter=odd4) == E_WORKSPACE, d
        assert call(ws_bytes=0) == E_WORKSPACE
        for k in ('dt', 'gt', 'inter', 'area_dt', 'area_gt', 'ws'):
            assert call(**{k: odd4}) == call(**{k: odd8}) == E_ALIGN, k
        # an empty side needs none of its pointers; its alignment is not looked at
        nk = L.vkn_mask_overlap_workspace_bytes(0, G, H, W)
        assert call(K=0, dt=None, inter=None, area_dt=None, ws_bytes=nk, gt=odd4) == E_ALIGN and call(K=0, dt=odd4, inter=odd4, area_dt=odd4, ws_bytes=nk, ws=odd8) == E_ALIGN
        assert call(K=0, gt=None, ws_bytes=nk) == E_ARG and call(K=0, ws_bytes=nb) == E_WORKSPACE
        ng = L.vkn_mask_overlap_workspace_bytes(K, 0, H, W)
        assert call(G=0, gt=None, inter=None, area_gt=None, ws_bytes=ng, area_dt=odd4) == E_ALIGN and call(G=0, area_dt=None, ws_bytes=ng) == E_ARG
        assert call(K=0, G=0, dt=None, gt=None, inter=None, area_dt=None, area_gt=None, ws=None, ws_bytes=0) == 0       # nothing to do, nothing launched
        assert call(K=0, G=0, ws_bytes=16) == E_WORKSPACE
    big = dict(K=1, H=1 << 15, W=1 << 14, ws_bytes=L.vkn_mask_overlap_workspace_bytes(1, G, 1 << 15, 1 << 14))
    assert big['ws_bytes'] > 0 and u8(dt=odd4, **big) == E_ALIGN and f32(dt=odd4, **big) == f32(**dict(big, ws_bytes=0)) == E_SHAPE

    cfg = _cfg(vkn)
    sb = L.vkn_mask_ap_state_bytes(ctypes.byref(cfg))
    bad = _cfg(vkn)
    bad.A = 5
    okm = dict(cfg=ctypes.byref(cfg), state=p, state_bytes=sb, inter=p, area_dt=p, area_gt=p, scores=p, dt_labels=p, gt_labels=p, gt_crowd=p, gt_area=p, K=K, G=G,
               image=7, match_gt=p, stream=None)

    def match(**kw):
        return L.vkn_mask_ap_match(*dict(okm, **kw).values())
    for k in ('cfg', 'state', 'inter', 'area_dt', 'area_gt', 'scores', 'dt_labels', 'gt_labels', 'gt_crowd'):
        assert match(**{k: None}) == match(**{k: None, 'state_bytes': 0}) == match(**{k: None, 'cfg' if k != 'cfg' else 'state': None}) == E_ARG, k
    assert match(K=-1) == match(G=-1) == E_ARG
    assert match(cfg=ctypes.byref(bad)) == match(cfg=ctypes.byref(bad), state_bytes=0) == match(K=1025) == match(G=1025, state=odd4) == E_SHAPE
    assert match(state_bytes=sb + 16) == match(state_bytes=sb - 1, state=odd4) == match(state_bytes=0) == E_WORKSPACE
    for k in ('state', 'inter', 'area_dt', 'area_gt'):
        assert match(**{k: odd4}) == match(**{k: odd8}) == E_ALIGN, k
    for k in ('scores', 'dt_labels', 'gt_labels', 'match_gt'):
        assert match(**{k: 4096 + 2}) == E_ALIGN, k
    assert match(gt_area=odd4) == E_ALIGN and match(gt_crowd=4097, state=odd4) == E_ALIGN
    assert match(K=0, G=0, **{k: None for k in okm if k not in ('cfg', 'state', 'state_bytes', 'K', 'G', 'image', 'stream')}, state=odd4) == E_ALIGN
    for fn, args in ((L.vkn_mask_ap_reset, (p, sb, None)),):
        assert fn(None, *args) == fn(ctypes.byref(cfg), None, sb, None) == E_ARG and fn(ctypes.byref(bad), *args) == E_SHAPE
        assert fn(ctypes.byref(cfg), p, sb + 16, None) == fn(ctypes.byref(cfg), odd4, sb - 16, None) == E_WORKSPACE and fn(ctypes.byref(cfg), odd4, sb, None) == E_ALIGN


@pytest.mark.gpu
def test_host_pointers_are_refused_last_and_nothing_is_launched(vkn):
    L = vkn._lib.lib()
    dev = torch.device('cuda:0')
    K, G, H, W = 2, 2, 5, 7
    nb = L.vkn_mask_overlap_workspace_bytes(K, G, H, W)
    dt, gt = torch.ones((K, H, W), dtype=torch.uint8, device=dev), torch.ones((G, H, W), dtype=torch.uint8, device=dev)
    logits = torch.ones((K, H, W), dtype=torch.float32, device=dev)
    outs = {k: torch.full((n,), 0x5A, dtype=torch.uint8, device=dev) for k, n in (('inter', 8 * K * G), ('area_dt', 8 * K), ('area_gt', 8 * G), ('ws', nb))}
    host = (ctypes.c_int * 4096)()
    hp = ctypes.addressof(host)
    hp += (-hp) % 16

    def call(f32=False, ws_bytes=nb, **kw):
        a = dict(dt=(logits if f32 else dt).data_ptr(), gt=gt.data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})
        a.update(kw)
        tail = (a['gt'], K, G, H, W, a['inter'], a['area_dt'], a['area_gt'], a['ws'], ws_bytes, None)
        return L.vkn_mask_overlap_f32(a['dt'], 0.5, *tail) if f32 else L.vkn_mask_overlap_u8(a['dt'], *tail)
    with torch.cuda.device(dev):
        for f32 in (False, True):
            for k in ('dt', 'gt', 'inter', 'area_dt', 'area_gt', 'ws'):
                assert call(f32, **{k: hp}) == E_ARG, k
            assert call(f32, inter=hp, ws_bytes=nb + 16) == E_WORKSPACE and call(f32, inter=hp + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in outs.values())
