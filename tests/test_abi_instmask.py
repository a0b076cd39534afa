"""The C ABI of the instance result part include/vkn_instmask.h, judged as tests/test_abi_maskap.py judges its header: a regex reading of
the argument lists, the built library's exports, a C compiler for the header, the sizes and the refusals in their order.  The part is
bound through a TENTH table, `_lib.INSTANCE_RESULT_HEADERS` / `_lib.ABI_INSTANCE_RESULT`, and leaves the nine tables before it, their
constant records, `_each`'s default, `_bound`, `_every` and `_all_bound` as they were."""
import ctypes
import os
import re

import pytest
import torch

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_instmask.h'
SYMBOLS = {'vkn_sizeof_inst_mask_cfg': 1, 'vkn_sizeof_instmask_cfg': 1, 'vkn_instance_bits_workspace_bytes': 2, 'vkn_instance_bits_f32': 10,
           'vkn_bits_rle_workspace_bytes': 3, 'vkn_bits_rle_encode': 13, 'vkn_bits_mask_overlap_workspace_bytes': 4, 'vkn_bits_mask_overlap': 12}
E_ARG, E_SHAPE, E_WORKSPACE, E_ALIGN = -1, -2, -3, -5


def _cfg(vkn, up=4, Hm=12, Wm=20, bis=(48, 80), img=(45, 77), ori=(37, 65)):
    return vkn.ops.instance_mask_cfg(Hm, Wm, dict(batch_input_shape=bis, img_shape=(*img, 3), ori_shape=(*ori, 3)), up)


def test_the_tenth_table_leaves_the_nine_tables_alone(vkn):
    lib = vkn._lib
    assert lib.INSTANCE_RESULT_HEADERS == (HEADER,) == tuple(lib.ABI_INSTANCE_RESULT)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI) and lib.EXTENSION_HEADERS == ('vkn_seg_loss.h',) == tuple(lib.ABI_EXT)
    assert lib.METRIC_HEADERS == ('vkn_stq.h',) == tuple(lib.ABI_METRIC) and lib.WINDOW_METRIC_HEADERS == ('vkn_vpq.h',) == tuple(lib.ABI_WINDOW_METRIC)
    assert lib.TRAIN_HEADERS == ('vkn_fpn_train.h',) == tuple(lib.ABI_TRAIN) and lib.NECK_HEADERS == ('vkn_msda.h',) == tuple(lib.ABI_NECK)
    assert lib.NECK_TRAIN_HEADERS == ('vkn_msda_train.h',) == tuple(lib.ABI_NECK_TRAIN) and lib.RESULT_HEADERS == ('vkn_rle.h',) == tuple(lib.ABI_RESULT)
    assert lib.INSTANCE_METRIC_HEADERS == ('vkn_maskap.h',) == tuple(lib.ABI_INSTANCE_METRIC)
    part = lib.ABI_INSTANCE_RESULT[HEADER]
    assert part.path == os.path.join(ROOT, 'include', HEADER) and part.symbols == tuple(part.protos) == tuple(SYMBOLS)
    before = (lib.ABI, lib.ABI_EXT, lib.ABI_METRIC, lib.ABI_WINDOW_METRIC, lib.ABI_TRAIN, lib.ABI_NECK, lib.ABI_NECK_TRAIN, lib.ABI_RESULT, lib.ABI_INSTANCE_METRIC)
    assert not set(part.symbols) & {s for t in before for h in t.values() for s in h.symbols}          # no name is declared twice
    assert part.consts == lib.INSTMASK and all(k.startswith('VKN_INSTMASK_') for k in part.consts)
    assert dict(VKN_INSTMASK_MAX_K=1024, VKN_INSTMASK_MAX_SCALED_W=4096, VKN_INSTMASK_TILE_ROWS=16, VKN_INSTMASK_LDS_BYTES=65536, VKN_INSTMASK_WS_BYTES=16,
                VKN_INSTMASK_STATUS_ROW_RANGE=1, VKN_INSTMASK_STATUS_FOOTPRINT=2).items() <= part.consts.items()
    others = set(lib.CONSTS) | set(lib.SEG) | set(lib.STQ) | set(lib.VPQ) | set(lib.FPN_TRAIN) | set(lib.MSDA) | set(lib.MSDA_TRAIN) | set(lib.RLE) | set(lib.MASKAP)
    assert not set(part.consts) & others
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert lib.RLE == lib.ABI_RESULT['vkn_rle.h'].consts and lib.MASKAP == lib.ABI_INSTANCE_METRIC['vkn_maskap.h'].consts
    assert list(part.structs) == ['VknInstMaskCfg'] == list(part.mirrors) and part.mirrors['VknInstMaskCfg'] is lib.VknInstMaskCfg
    assert 'VknInstMaskCfg' not in lib.MIRRORS and 'vkn_instmask.hip' in lib.SOURCES
    # the four loops of the nine tables are what they were; the binding loops go over `_all_parts`: those and the tenth
    assert lib._each('protos') == lib._each('protos', before[:6]) and lib._bound('protos') == lib._each('protos', before[:7])
    assert lib._every('protos') == lib._each('protos', before[:8]) and lib._all_bound('protos') == lib._each('protos', before)
    assert not any(h == HEADER for h, _, _ in lib._all_bound('protos'))
    bound = lib._all_parts('protos')
    assert bound[:-len(SYMBOLS)] == lib._all_bound('protos') and [(h, n) for h, n, _ in bound[-len(SYMBOLS):]] == [(HEADER, n) for n in SYMBOLS]
    names = [n for _, n, _ in bound]
    assert len(names) == len(set(names))
    order = (lib.ABI_HEADERS + lib.EXTENSION_HEADERS + lib.METRIC_HEADERS + lib.WINDOW_METRIC_HEADERS + lib.TRAIN_HEADERS + lib.NECK_HEADERS
             + lib.NECK_TRAIN_HEADERS + lib.RESULT_HEADERS + lib.INSTANCE_METRIC_HEADERS + lib.INSTANCE_RESULT_HEADERS)
    read = lib.read_abi(os.path.join(ROOT, 'include'), order)
    assert tuple(read) == order and read[HEADER].protos == part.protos
    assert {h: read[h].protos for h in order[:-1]} == {h: hdr.protos for t in before for h, hdr in t.items()}
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), ('vkn.h', 'vkn_rle.h', HEADER))            # "vkn_maskap.h" is not listed before it
    # it stands on the two parts whose bits entries it declares
    assert re.findall(r'#include "([^"]+)"', open(part.path).read()) == ['vkn.h', 'vkn_rle.h', 'vkn_maskap.h']


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    full = open(os.path.join(ROOT, 'include', HEADER)).read()
    text = re.sub(r'/\*.*?\*/', ' ', full, flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_INSTANCE_RESULT[HEADER].symbols) == list(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert hasattr(raw, name), name
        fn = getattr(L, name)
        assert fn.restype is (ctypes.c_size_t if name.endswith('_bytes') or name.startswith('vkn_sizeof') else ctypes.c_int), name
        assert len(fn.argtypes) == (0 if params.strip() == 'void' else params.count(',') + 1) == (SYMBOLS[name] if params.strip() != 'void' else 0), name
    out = os.popen(f'nm -D --defined-only {lib.LIBPATH}').read()
    exported = set(re.findall(r'\b(vkn_instance_\w+|vkn_bits_\w+|vkn_sizeof_inst\w+|vkn_instmask\w*)\b', out))
    assert exported == set(SYMBOLS)
    # the bits entries take what their u8 twins take
    assert list(L.vkn_bits_rle_encode.argtypes) == list(L.vkn_rle_encode_u8.argtypes) and list(L.vkn_bits_mask_overlap.argtypes) == list(L.vkn_mask_overlap_u8.argtypes)
    assert L.vkn_bits_rle_workspace_bytes.argtypes == [ctypes.c_int] * 3 and L.vkn_bits_mask_overlap_workspace_bytes.argtypes == [ctypes.c_int] * 4
    assert L.vkn_instance_bits_f32.argtypes[0] is ctypes.POINTER(lib.VknInstMaskCfg) and L.vkn_instance_bits_f32.argtypes[5] is ctypes.c_float
    assert L.vkn_sizeof_inst_mask_cfg() == L.vkn_sizeof_instmask_cfg() == ctypes.sizeof(lib.VknInstMaskCfg) == 40
    assert 'knet/det/kernel_update_head.py:443-466' in full and 'v0 * w0 + v1 * w1' in full and 'Not built: polygon output' in full
    # the encoder's header no longer calls the rescale "not built"
    rle = open(os.path.join(ROOT, 'include', 'vkn_rle.h')).read()
    assert 'vkn_instmask.h' in rle and 'it stays the caller\'s' not in rle


def test_header_is_c99_on_its_own(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ VknInstMaskCfg cfg; size_t n = vkn_instance_bits_workspace_bytes(0, 1);\n'
                   '  int rc = vkn_instance_bits_f32(0, 0, 1, 0, 1, 0.5f, 0, 0, n, 0) + vkn_bits_rle_encode(0, 1, 2, 3, 0, 0, 0, 0, 0, 0, 0, vkn_bits_rle_workspace_bytes(1, 2, 3), 0)\n'
                   '    + vkn_bits_mask_overlap(0, 0, 1, 1, 2, 3, 0, 0, 0, 0, vkn_bits_mask_overlap_workspace_bytes(1, 1, 2, 3), 0);\n'
                   '  cfg.up = 4; cfg.reserved = 0;\n'
                   '  return rc == 3 * VKN_E_ARG && sizeof cfg == vkn_sizeof_instmask_cfg() && sizeof cfg == vkn_sizeof_inst_mask_cfg()\n'
                   '    && VKN_INSTMASK_MAX_K + VKN_INSTMASK_MAX_SCALED_W + VKN_INSTMASK_TILE_ROWS + VKN_INSTMASK_BATCH + VKN_INSTMASK_LDS_BYTES + VKN_INSTMASK_WS_BYTES\n'
                   '    > (int)(VKN_INSTMASK_STATUS_ROW_RANGE | VKN_INSTMASK_STATUS_FOOTPRINT) ? 0 : 1; }\n')
    _compile('c99', src)


def test_sizes_and_envelopes(vkn):
    L = vkn._lib.lib()
    nb = lambda K=5, **kw: L.vkn_instance_bits_workspace_bytes(ctypes.byref(_cfg(vkn, **kw)), K)          # noqa: E731
    assert nb() == nb(K=1) == nb(K=1024) == 16 and L.vkn_instance_bits_workspace_bytes(None, 5) == 0
    for kw in (dict(up=1, Hm=736, Wm=1280, bis=(736, 1280), img=(720, 1280), ori=(720, 1280)), dict(up=4, Hm=184, Wm=320, bis=(736, 1280), img=(720, 1280), ori=(720, 1280)),
               dict(up=4, Hm=90, Wm=160, bis=(360, 640), img=(360, 640), ori=(720, 1280)), dict(up=1, Hm=800, Wm=1344, bis=(800, 1344), img=(800, 1333), ori=(480, 640)),
               dict(up=2, Hm=512, Wm=1024, bis=(1024, 2048), img=(1024, 2048), ori=(1024, 2048)), dict(up=4, Hm=1, Wm=1, bis=(1, 1), img=(1, 1), ori=(1, 1)),
               dict(up=4, Hm=8, Wm=1024, bis=(32, 4096), img=(32, 4096), ori=(32, 4096))):
        assert nb(K=100, **kw) == 16, kw
    for K in (0, -1, 1025):
        assert nb(K=K) == 0, K
    for kw in (dict(up=0), dict(up=3), dict(up=8), dict(Hm=0), dict(Wm=0), dict(bis=(0, 80)), dict(bis=(48, 0)), dict(img=(0, 77)), dict(img=(45, 0)), dict(ori=(0, 65)),
               dict(ori=(37, 0)), dict(img=(49, 77)), dict(img=(45, 81)), dict(Wm=1025), dict(up=1, Wm=4097, bis=(48, 4097), img=(48, 4097))):
        assert nb(**kw) == 0, kw
    # an extreme down-scaling: the footprint of one 64 x 16 tile does not fit the LDS budget
    assert nb(up=1, Hm=2048, Wm=4096, bis=(2048, 4096), img=(2048, 4096), ori=(64, 64)) == 0
    assert nb(up=1, Hm=2048, Wm=4096, bis=(2048, 4096), img=(2048, 4096), ori=(1024, 2048)) == 16
    # the bits consumers: the u8 entries' workspaces without the part that held the bits
    up16 = lambda n: (n + 15) // 16 * 16          # noqa: E731
    for K, H, W in ((1, 1, 1), (3, 5, 63), (3, 5, 64), (3, 5, 65), (100, 720, 1280), (1024, 1, 1)):
        strips = (W + 63) // 64
        assert L.vkn_bits_rle_workspace_bytes(K, H, W) == L.vkn_rle_workspace_bytes(K, H, W) - up16(8 * K * strips * H) > 0
        for G in (0, 2, 70):
            assert L.vkn_bits_mask_overlap_workspace_bytes(K, G, H, W) == up16(8 * G * strips * H) == L.vkn_mask_overlap_workspace_bytes(K, G, H, W) - up16(8 * K * strips * H)
    for bad in ((0, 4, 4), (1025, 4, 4), (1, 0, 4), (1, 4, 0), (1, 1 << 16, 1 << 15)):
        assert L.vkn_bits_rle_workspace_bytes(*bad) == 0 and (L.vkn_bits_mask_overlap_workspace_bytes(bad[0], 1, *bad[1:]) == 0 or bad[0] == 0), bad      # (K = 0 is an image without detections)


def test_refusals_in_their_order_need_no_device(vkn):
    """NULL pointers / negative counts -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then the size -> VKN_E_WORKSPACE, then alignment ->
    VKN_E_ALIGN: all four are decided before the library asks the runtime anything (the pointers below are never dereferenced)."""
    L = vkn._lib.lib()
    p, odd4, odd8 = 4096, 4096 + 4, 4096 + 8
    cfg = _cfg(vkn)
    ok = dict(cfg=ctypes.byref(cfg), logits=p, N=7, rows=p, K=5, thr=0.5, bits=p, ws=p, ws_bytes=16, stream=None)

    def bits(**kw):
        return L.vkn_instance_bits_f32(*dict(ok, **kw).values())
    for k in ('cfg', 'logits', 'bits', 'ws'):
        assert bits(**{k: None}) == bits(**{k: None, 'K': 0}) == bits(**{k: None, 'ws_bytes': 0}) == bits(**{k: None, 'rows': 4098}) == E_ARG, k
    assert bits(N=-1) == bits(K=-1) == bits(K=-1, ws_bytes=0) == E_ARG
    for kw in (dict(K=0), dict(K=1025), dict(N=0), dict(rows=None, K=8), dict(cfg=ctypes.byref(_cfg(vkn, up=3))), dict(cfg=ctypes.byref(_cfg(vkn, img=(49, 77)))),
               dict(cfg=ctypes.byref(_cfg(vkn, up=1, Hm=2048, Wm=4096, bis=(2048, 4096), img=(2048, 4096), ori=(64, 64))))):
        assert bits(**kw) == bits(ws_bytes=0, **kw) == bits(bits=odd4, **kw) == E_SHAPE, kw
    for d in (-16, 16, -1, 1):
        assert bits(ws_bytes=16 + d) == bits(ws_bytes=16 + d, bits=odd4) == E_WORKSPACE, d
    for k in ('logits', 'bits', 'ws'):
        assert bits(**{k: odd4}) == bits(**{k: odd8}) == E_ALIGN, k
    assert bits(rows=4098) == E_ALIGN

    K, G, H, W = 3, 2, 37, 131
    nr = L.vkn_bits_rle_workspace_bytes(K, H, W)
    okr = dict(bits=p, K=K, H=H, W=W, records=p, runs=p, cap_runs=8, bytes=p, cap_bytes=8, status=p, ws=p, ws_bytes=nr, stream=None)

    def rle(**kw):
        return L.vkn_bits_rle_encode(*dict(okr, **kw).values())
    for k in ('bits', 'records', 'runs', 'bytes', 'status', 'ws'):
        assert rle(**{k: None}) == rle(**{k: None, 'H': 0}) == rle(**{k: None, 'ws_bytes': 0}) == E_ARG, k
    assert rle(K=-1) == rle(cap_runs=-1) == rle(cap_bytes=-1) == E_ARG
    for kw in (dict(K=0), dict(K=1025), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15)):
        assert rle(**kw) == rle(ws_bytes=0, **kw) == rle(records=odd4, **kw) == E_SHAPE, kw
    assert rle(ws_bytes=nr + 16) == rle(ws_bytes=L.vkn_rle_workspace_bytes(K, H, W)) == rle(ws_bytes=0, runs=odd4) == E_WORKSPACE
    for k in ('bits', 'records', 'runs', 'bytes', 'ws'):
        assert rle(**{k: odd4}) == E_ALIGN, k
    assert rle(status=4098) == E_ALIGN

    no = L.vkn_bits_mask_overlap_workspace_bytes(K, G, H, W)
    oko = dict(dt=p, gt=p, K=K, G=G, H=H, W=W, inter=p, area_dt=p, area_gt=p, ws=p, ws_bytes=no, stream=None)

    def ov(**kw):
        return L.vkn_bits_mask_overlap(*dict(oko, **kw).values())
    for k in ('dt', 'gt', 'inter', 'area_dt', 'area_gt', 'ws'):
        assert ov(**{k: None}) == ov(**{k: None, 'H': 0}) == ov(**{k: None, 'ws_bytes': 0}) == E_ARG, k
    assert ov(K=-1) == ov(G=-1) == ov(H=-1) == E_ARG
    for kw in (dict(K=1025), dict(G=1025), dict(H=0), dict(W=0), dict(H=1 << 16, W=1 << 15)):
        assert ov(**kw) == ov(ws_bytes=0, **kw) == ov(inter=odd4, **kw) == E_SHAPE, kw
    assert ov(ws_bytes=no + 16) == ov(ws_bytes=L.vkn_mask_overlap_workspace_bytes(K, G, H, W)) == ov(ws_bytes=0, inter=odd4) == E_WORKSPACE
    for k in ('dt', 'gt', 'inter', 'area_dt', 'area_gt', 'ws'):
        assert ov(**{k: odd4}) == ov(**{k: odd8}) == E_ALIGN, k
    # no ground truth: nothing is packed, no workspace; an empty call does nothing
    assert ov(G=0, gt=None, inter=None, area_gt=None, ws=None, ws_bytes=0, area_dt=odd4) == E_ALIGN and ov(G=0, ws_bytes=16) == E_WORKSPACE
    assert ov(K=0, G=0, dt=None, gt=None, inter=None, area_dt=None, area_gt=None, ws=None, ws_bytes=0) == 0


@pytest.mark.gpu
def test_host_pointers_are_refused_last_and_nothing_is_launched(vkn):
    L = vkn._lib.lib()
    dev = torch.device('cuda:0')
    cfg = _cfg(vkn)
    logits = torch.ones((5, 12, 20), dtype=torch.float32, device=dev)
    rows = torch.zeros((5,), dtype=torch.int32, device=dev)
    outs = {k: torch.full((n,), 0x5A, dtype=torch.uint8, device=dev) for k, n in (('bits', 8 * 5 * 2 * 37), ('ws', 16))}
    host = (ctypes.c_int * 4096)()
    hp = ctypes.addressof(host)
    hp += (-hp) % 16

    def call(ws_bytes=16, **kw):
        a = dict(logits=logits.data_ptr(), rows=rows.data_ptr(), **{k: t.data_ptr() for k, t in outs.items()})
        a.update(kw)
        return L.vkn_instance_bits_f32(ctypes.byref(cfg), a['logits'], 5, a['rows'], 5, 0.5, a['bits'], a['ws'], ws_bytes, None)
    with torch.cuda.device(dev):
        for k in ('logits', 'rows', 'bits', 'ws'):
            assert call(**{k: hp}) == E_ARG, k
        assert call(bits=hp, ws_bytes=32) == E_WORKSPACE and call(bits=hp + 4) == E_ALIGN
    torch.cuda.synchronize()
    assert all(bool((t == 0x5A).all()) for t in outs.values())
