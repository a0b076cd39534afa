"""The C ABI of the extension part include/vkn_seg_loss.h, judged as tests/test_abi_headers.py judges the five headers of `_lib.ABI_HEADERS`:
a regex reading of the argument lists, the built library's exports, a C compiler for the header and the struct layout, the size probe,
and the envelope's refusals in their order.  The extension is bound through `_lib.EXTENSION_HEADERS` / `_lib.ABI_EXT` and leaves
`_lib.ABI_HEADERS`, `_lib.ABI` and `_lib.CONSTS` as they were."""
import ctypes
import os
import re

import pytest
import torch

from test_abi_headers import HEADERS, ROOT, _compile

HEADER = 'vkn_seg_loss.h'
SYMBOLS = {'vkn_sizeof_seg_image': 0, 'vkn_seg_targets_u8': 9, 'vkn_seg_loss_state_bytes': 5, 'vkn_seg_loss_fwd_f32': 15,
           'vkn_seg_loss_bwd_f32': 14}
FIELDS = ['masks', 'sem', 'labels', 'sem_cls', 'gt_inds', 'G', 'n_sem', 'Np']
CONSTS = dict(VKN_SEG_LOSS_FOCAL=0, VKN_SEG_LOSS_CE=1, VKN_SEG_MAX_IMAGES=64, VKN_SEG_MAX_CLASSES=255, VKN_SEG_MAX_ROWS=65535)
E_ARG, E_SHAPE, E_ALIGN = -1, -2, -5


def test_the_extension_table_leaves_the_abi_table_alone(vkn):
    lib = vkn._lib
    assert lib.EXTENSION_HEADERS == (HEADER,) == tuple(lib.ABI_EXT)
    assert lib.ABI_HEADERS == HEADERS == tuple(lib.ABI)
    ext = lib.ABI_EXT[HEADER]
    assert ext.path == os.path.join(ROOT, 'include', HEADER) and ext.symbols == tuple(ext.protos) and set(ext.symbols) == set(SYMBOLS)
    assert not set(ext.symbols) & {s for h in HEADERS for s in lib.ABI[h].symbols}
    assert ext.consts == CONSTS == lib.SEG and not set(CONSTS) & set(lib.CONSTS)
    assert lib.CONSTS == {k: v for h in HEADERS for k, v in lib.ABI[h].consts.items()}
    assert list(ext.structs) == list(ext.mirrors) == ['VknSegImage'] and lib.VknSegImage is ext.mirrors['VknSegImage']
    assert 'VknSegImage' not in lib.MIRRORS and 'vkn_segloss.hip' in lib.SOURCES
    # one reading over both tables: the extension sees vkn.h's error codes through its #include
    assert lib.read_abi(os.path.join(ROOT, 'include'), lib.ABI_HEADERS + lib.EXTENSION_HEADERS)[HEADER].protos == ext.protos
    with pytest.raises(vkn.VknLibraryError):
        lib.read_abi(os.path.join(ROOT, 'include'), (HEADER,))                       # "vkn.h" is not listed before it


def test_header_is_exported_with_its_own_argument_lists(vkn):
    lib = vkn._lib
    text = re.sub(r'/\*.*?\*/', ' ', open(os.path.join(ROOT, 'include', HEADER)).read(), flags=re.S)
    declared = re.findall(r'\b(vkn_[a-z0-9_]+)\s*\(([^()]*)\)\s*;', text)
    assert [n for n, _ in declared] == list(lib.ABI_EXT[HEADER].symbols) and len(declared) == len(SYMBOLS)
    raw, L = ctypes.CDLL(lib.LIBPATH), lib.lib()
    for name, params in declared:
        assert getattr(raw, name) is not None
        fn = getattr(L, name)
        assert fn.restype in (ctypes.c_int, ctypes.c_size_t), name
        assert len(fn.argtypes) == (0 if params.strip() == 'void' else params.count(',') + 1) == SYMBOLS[name], name
    assert L.vkn_seg_targets_u8.argtypes[0]._type_ is lib.VknSegImage
    assert L.vkn_seg_loss_state_bytes.restype is ctypes.c_size_t and L.vkn_sizeof_seg_image.restype is ctypes.c_size_t
    assert L.vkn_seg_loss_fwd_f32.argtypes[9:12] == [ctypes.c_float] * 3 and L.vkn_seg_loss_bwd_f32.argtypes[9:11] == [ctypes.c_float] * 2
    # every entry cites the reference lines it replaces, in the header itself
    assert open(os.path.join(ROOT, 'include', HEADER)).read().count('knet/det/kernel_head.py:') >= 4


def test_header_is_c99_on_its_own_and_the_mirror_has_its_layout(vkn, tmp_path):
    src = tmp_path / 'use.c'
    src.write_text(f'#include "include/{HEADER}"\nint main(void) {{ VknSegImage im; im.G = VKN_SEG_MAX_ROWS; im.masks = 0;\n'
                   '  return im.G > VKN_SEG_MAX_CLASSES * VKN_SEG_MAX_IMAGES + VKN_SEG_LOSS_CE + VKN_SEG_LOSS_FOCAL + VKN_E_SHAPE ? 0 : 1; }\n')
    _compile('c99', src)
    m = vkn._lib.VknSegImage
    assert [f for f, _ in m._fields_] == FIELDS
    lines = ['#include <stddef.h>', f'#include "include/{HEADER}"', f'_Static_assert(sizeof(VknSegImage) == {ctypes.sizeof(m)}, "sizeof");']
    for field, _ in m._fields_:
        f = getattr(m, field)
        lines.append(f'_Static_assert(offsetof(VknSegImage, {field}) == {f.offset}, "offsetof {field}");')
        lines.append(f'_Static_assert(sizeof(((VknSegImage*)0)->{field}) == {f.size}, "sizeof {field}");')
    assert len(lines) == 3 + 2 * 8
    lay = tmp_path / 'layout.c'
    lay.write_text('\n'.join(lines) + '\n')
    _compile('c11', lay)
    assert vkn._lib.lib().vkn_sizeof_seg_image() == ctypes.sizeof(m) == 56


def test_state_bytes_and_refusals_that_need_no_device(vkn):
    """NULL pointers / negative counts -> VKN_E_ARG, then the envelope -> VKN_E_SHAPE, then alignment -> VKN_E_ALIGN: all three are decided
    before the library asks the runtime anything, so a machine without a GPU sees them (the pointers below are never dereferenced)."""
    lib = vkn._lib
    L = lib.lib()
    sb = L.vkn_seg_loss_state_bytes
    assert sb(0, 1, 1, 1, 1) == 64 + 16 and sb(1, 1, 1, 1, 1) == 64 + 16 + 8            # header, one fp64 partial (padded), (max, log-sum)
    assert sb(1, 2, 90, 160, 4) - sb(0, 2, 90, 160, 4) == 2 * 360 * 640 * 8
    assert sb(0, 1, 8, 8, 3) == 0 and sb(2, 1, 8, 8, 2) == 0 and sb(0, 65, 8, 8, 2) == 0 and sb(0, 0, 8, 8, 2) == 0 and sb(0, 1, 0, 8, 2) == 0
    fwd, bwd, tg = L.vkn_seg_loss_fwd_f32, L.vkn_seg_loss_bwd_f32, L.vkn_seg_targets_u8
    p, odd = 4096, 4096 + 2                                      # non-NULL, 16-byte aligned / misaligned; never dereferenced
    ok = dict(low=p, tgt=p, dense_pos=p, mode=0, B=1, ncls=19, h=8, w=8, S=2, alpha=0.25, gamma=2.0, loss_weight=1.0, loss=p, state=p, stream=None)

    def call_fwd(**kw):
        a = dict(ok, **kw)
        return fwd(*[a[k] for k in ok])
    for k in ('low', 'tgt', 'dense_pos', 'loss', 'state'):
        assert call_fwd(**{k: None}) == E_ARG, k
    assert call_fwd(dense_pos=None, mode=1, S=3) == E_SHAPE         # CE reads no dense_pos: the next check speaks
    for kw in (dict(S=3), dict(S=8), dict(S=0), dict(ncls=0), dict(ncls=256), dict(B=0), dict(B=65), dict(h=0), dict(w=0), dict(mode=2),
               dict(ncls=255, h=2048, w=1040), dict(h=3 * 65535 + 1, w=1, ncls=1)):
        assert call_fwd(**kw) == E_SHAPE, kw
        assert call_fwd(low=None, **kw) == E_ARG and call_fwd(low=odd, **kw) == E_SHAPE, kw          # the order
    for k in ('low', 'dense_pos', 'loss', 'state'):
        assert call_fwd(**{k: odd}) == E_ALIGN, k
    okb = dict(low=p, tgt=p, gout=p, mode=1, B=1, ncls=19, h=8, w=8, S=4, alpha=0.0, gamma=0.0, state=p, grad_low=p, stream=None)

    def call_bwd(**kw):
        a = dict(okb, **kw)
        return bwd(*[a[k] for k in okb])
    for k in ('low', 'tgt', 'gout', 'state', 'grad_low'):
        assert call_bwd(**{k: None}) == E_ARG, k
    for kw in (dict(S=3), dict(ncls=256), dict(B=65), dict(mode=-1)):
        assert call_bwd(**kw) == E_SHAPE and call_bwd(gout=None, **kw) == E_ARG and call_bwd(grad_low=odd, **kw) == E_SHAPE, kw
    for k in ('low', 'gout', 'state', 'grad_low'):
        assert call_bwd(**{k: odd}) == E_ALIGN, k
    imgs = (lib.VknSegImage * 2)(lib.VknSegImage(p, p, p, p, p, 3, 2, 12), lib.VknSegImage(None, None, None, None, None, 0, 0, 0))

    def call_tg(imgs=imgs, B=2, H=16, W=16, ncls=19, tgt=p, dense_pos=p, status=p):
        return tg(imgs, B, H, W, ncls, tgt, dense_pos, status, None)
    assert call_tg(imgs=None) == call_tg(tgt=None) == call_tg(dense_pos=None) == call_tg(status=None) == call_tg(B=-1) == E_ARG
    assert call_tg(B=0) == call_tg(B=65) == E_SHAPE                                  # before imgs[b] is indexed
    for bad in (lib.VknSegImage(None, p, p, p, p, 3, 2, 12), lib.VknSegImage(p, p, None, p, p, 3, 2, 12), lib.VknSegImage(p, p, p, None, p, 3, 2, 12),
                lib.VknSegImage(p, p, p, p, None, 3, 2, 12), lib.VknSegImage(p, p, p, p, p, -1, 2, 12), lib.VknSegImage(p, p, p, p, p, 3, 2, -1)):
        assert call_tg(imgs=(lib.VknSegImage * 1)(bad), B=1) == E_ARG
        assert call_tg(imgs=(lib.VknSegImage * 1)(bad), B=1, ncls=256) == E_ARG      # the order
    for kw in (dict(ncls=0), dict(ncls=256), dict(H=0), dict(W=0), dict(H=4 * 65535 + 1, W=1), dict(H=65536, W=32768)):
        assert call_tg(**kw) == E_SHAPE and call_tg(dense_pos=odd, **kw) == E_SHAPE, kw
    for big in (lib.VknSegImage(p, p, p, p, p, 65536, 2, 12), lib.VknSegImage(p, p, p, p, p, 3, 2, 65536)):
        assert call_tg(imgs=(lib.VknSegImage * 1)(big), B=1) == E_SHAPE
    assert call_tg(dense_pos=odd) == call_tg(status=odd) == E_ALIGN
    assert call_tg(imgs=(lib.VknSegImage * 1)(lib.VknSegImage(odd, p, p, p, p, 3, 2, 12)), B=1) == E_ALIGN


@pytest.mark.gpu
def test_host_pointers_are_refused_last_and_nothing_is_launched(vkn):
    """With a device present: a HOST pointer where device memory is expected is VKN_E_ARG, after shape and alignment had their say."""
    lib = vkn._lib
    L = lib.lib()
    dev = torch.device('cuda:0')
    B, ncls, h, w, S = 1, 5, 4, 6, 2
    low = torch.zeros((B, ncls, h, w), device=dev)
    tgt = torch.full((B, S * h, S * w), 77, dtype=torch.uint8, device=dev)
    dp, status = torch.full((1,), 123, dtype=torch.int32, device=dev), torch.zeros((1,), dtype=torch.int32, device=dev)
    loss, grad = torch.full((1,), 5.0, device=dev), torch.full_like(low, 7.0)
    state = torch.zeros((L.vkn_seg_loss_state_bytes(0, B, h, w, S),), dtype=torch.uint8, device=dev)
    host = (ctypes.c_float * 1024)()
    hp = ctypes.addressof(host)
    hp += (-hp) % 16
    d = lambda t: t.data_ptr()          # noqa: E731
    with torch.cuda.device(dev):
        assert L.vkn_seg_loss_fwd_f32(hp, d(tgt), d(dp), 0, B, ncls, h, w, S, 0.25, 2.0, 1.0, d(loss), d(state), None) == E_ARG
        assert L.vkn_seg_loss_fwd_f32(hp, d(tgt), d(dp), 0, B, ncls, h, w, 3, 0.25, 2.0, 1.0, d(loss), d(state), None) == E_SHAPE
        assert L.vkn_seg_loss_fwd_f32(hp, d(tgt), d(dp), 0, B, ncls, h, w, S, 0.25, 2.0, 1.0, d(loss) + 2, d(state), None) == E_ALIGN
        assert L.vkn_seg_loss_fwd_f32(d(low), d(tgt), d(dp), 0, B, ncls, h, w, S, 0.25, 2.0, 1.0, hp, d(state), None) == E_ARG
        assert L.vkn_seg_loss_bwd_f32(d(low), d(tgt), hp, 0, B, ncls, h, w, S, 0.25, 2.0, d(state), d(grad), None) == E_ARG
        assert L.vkn_seg_loss_bwd_f32(d(low), d(tgt), d(loss), 0, B, ncls, h, w, S, 0.25, 2.0, d(state), hp, None) == E_ARG
        imgs = (lib.VknSegImage * 1)(lib.VknSegImage(None, None, None, None, hp, 0, 0, 4))
        assert L.vkn_seg_targets_u8(imgs, 1, S * h, S * w, ncls, d(tgt), d(dp), d(status), None) == E_ARG
        imgs = (lib.VknSegImage * 1)(lib.VknSegImage(None, None, None, None, None, 0, 0, 0))
        assert L.vkn_seg_targets_u8(imgs, 1, S * h, S * w, ncls, hp, d(dp), d(status), None) == E_ARG
    torch.cuda.synchronize()
    assert bool((tgt == 77).all()) and int(dp) == 123 and float(loss) == 5.0 and bool((grad == 7.0).all()) and int(status) == 0
