"""GPU: the split weight tile images (csrc/vkn_wimage.h, written by csrc/vkn_wimage.hip) byte for byte against their numpy restatement
tests/wimage_ref.py, through every ABI writer: vkn_split_weight_f32, vkn_split_weight_t_f32, vkn_split_weights_batch_f32.  The
matrices are seeded and non-integer (`wimage_ref.matrix`): their middle and low planes are full, which the integer-valued operands of
tests/test_gpu_exact.py never are, and tests/test_gpu_abi_contract.py compares the writers only with each other.  Every output buffer
is pre-filled with a byte pattern, so a byte the writer leaves out shows.  (The two-plane fp16 writer has no ABI entry of its own.)"""
import numpy as np
import pytest
import torch

import wimage_ref as wr

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
FILL = 0xA5


def _stream():
    return torch.cuda.current_stream().cuda_stream


def _out(nbytes):
    return torch.full((nbytes,), FILL, dtype=torch.uint8, device=DEV)


def _same(name, got, want):
    got = got.cpu().numpy()
    assert got.shape == want.shape, f'{name}: {got.shape[0]} bytes, the restatement has {want.shape[0]}'
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f'{name}: {bad.size} of {want.size} bytes differ, first at byte {bad[0]}: {got[bad[0]]:#x} for {want[bad[0]]:#x}'


def _batch(vkn, items):
    """items: (device tensor holding W, element offset of W in it, ldn, ldk, Nout, K, kvalid, expected bytes) -> None; asserts"""
    I = vkn._lib.VknSplitItem
    outs = [_out(len(want)) for *_, want in items]
    arr = (I * len(items))(*[I(t.data_ptr() + 4 * off, o.data_ptr(), ldn, ldk, nout, K, kvalid, 0)
                             for (t, off, ldn, ldk, nout, K, kvalid, _), o in zip(items, outs)])
    assert vkn._lib.lib().vkn_split_weights_batch_f32(arr, len(items), _stream()) == 0
    torch.cuda.synchronize()
    for i, ((*_, want), o) in enumerate(zip(items, outs)):
        _same(f'item {i}', o, want)


@pytest.mark.parametrize('nout,k', wr.SHAPES)
def test_split_weight(vkn, nout, k):
    W = wr.matrix(nout, k, 4200 + nout)
    want = wr.images(W)
    Wd, out = torch.from_numpy(W).to(DEV), _out(len(want))
    assert vkn._lib.lib().vkn_split_weight_f32(Wd.data_ptr(), out.data_ptr(), nout, k, _stream()) == 0
    torch.cuda.synchronize()
    _same(f'vkn_split_weight_f32 ({nout}, {k})', out, want)


@pytest.mark.parametrize('nout,k', wr.SHAPES)
def test_split_weight_t(vkn, nout, k):
    """W stored [K][Nout]; the images stand for its transpose [Nout][K]"""
    Wm = wr.matrix(nout, k, 4300 + nout)
    want = wr.images(Wm)
    stored = torch.from_numpy(np.ascontiguousarray(Wm.T)).to(DEV)
    out = _out(len(want))
    assert vkn._lib.lib().vkn_split_weight_t_f32(stored.data_ptr(), out.data_ptr(), nout, k, _stream()) == 0
    torch.cuda.synchronize()
    _same(f'vkn_split_weight_t_f32 ({nout}, {k})', out, want)


def test_batch_short_contraction(vkn):
    """kvalid = 40 of K = 64, rows of 40 floats: the first k tile is whole (16-byte reads), the second takes the element-wise path and
    pads zeros from k = 40 on"""
    W = wr.matrix(300, 40, 4401)
    _batch(vkn, [(torch.from_numpy(W).to(DEV), 0, 40, 1, 300, 64, 40, wr.images(W, K=64))])


def test_batch_row_stride_65(vkn):
    """rows 65 floats apart: no row but the first starts on 16 bytes, so there is no 16-byte read path"""
    W = wr.matrix(300, 64, 4402)
    stored = np.full((300, 65), 7.5, dtype=np.float32)
    stored[:, :64] = W
    _batch(vkn, [(torch.from_numpy(stored).to(DEV), 0, 65, 1, 300, 64, 64, wr.images(W))])


def test_batch_base_off_by_one_float(vkn):
    """a base that is 4-byte but not 16-byte aligned"""
    W = wr.matrix(300, 64, 4403)
    stored = torch.from_numpy(np.concatenate([np.float32([7.5]), W.reshape(-1)])).to(DEV)
    assert stored.data_ptr() % 16 == 0
    _batch(vkn, [(stored, 1, 64, 1, 300, 64, 64, wr.images(W))])


def test_batch_negative_zero(vkn):
    W = wr.matrix(256, 32, 4404)
    W[3, 5] = -0.0
    W[200, 31] = 0.0
    want = wr.images(W)
    assert want.view(np.uint16)[wr_index(3, 5, 0, 32)] == 0x8000 and want.view(np.uint16)[wr_index(3, 5, 1, 32)] == 0
    _batch(vkn, [(torch.from_numpy(W).to(DEV), 0, 32, 1, 256, 32, 32, want)])


def wr_index(n, k, plane, K):
    return (((((n >> 8) * (K // 32) + (k >> 5)) * 3 + plane) * 4 + ((k & 31) >> 3)) * 256 + (n & 255)) * 8 + (k & 7)


def test_batch_two_items(vkn):
    """two items of different shape in one call, the second a transpose with a short contraction: the table walk"""
    A = wr.matrix(300, 64, 4405)
    Bm = wr.matrix(70, 40, 4406)            # the matrix the second item's images stand for: [Nout 70][kvalid 40], stored [40][70]
    stored = torch.from_numpy(np.ascontiguousarray(Bm.T)).to(DEV)
    _batch(vkn, [(torch.from_numpy(A).to(DEV), 0, 64, 1, 300, 64, 64, wr.images(A)),
                 (stored, 0, 1, 70, 70, 64, 40, wr.images(Bm, K=64))])


def test_misaligned_images_are_refused(vkn):
    """the images are written with 16-byte stores: a pointer that is not 16-byte aligned is VKN_E_ALIGN (-5), and nothing is written"""
    W = torch.from_numpy(wr.matrix(256, 32, 4407)).to(DEV)
    out = _out(6 * 256 * 32 + 16)
    L = vkn._lib.lib()
    assert L.vkn_split_weight_f32(W.data_ptr(), out.data_ptr() + 8, 256, 32, _stream()) == -5
    assert L.vkn_split_weight_t_f32(W.data_ptr(), out.data_ptr() + 2, 32, 256, _stream()) == -5
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
