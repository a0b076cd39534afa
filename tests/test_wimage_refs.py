"""CPU: the premises of tests/wimage_ref.py, the numpy restatement of the split weight tile image that tests/test_gpu_wimage.py holds the
library's writers to.  On the test matrices themselves: the terms add up to the value, the middle and low planes are not zeros (so the
GPU test cannot pass on images whose fine planes were lost), no plane holds a subnormal (so no flush mode of a device conversion can
enter), and the layout puts every element where the formula of the header says."""
import numpy as np
import pytest

import wimage_ref as wr

CASES = [(nout, k, 4100 + i) for i, (nout, k) in enumerate(wr.SHAPES)] + [(300, 40, 4110), (40, 300, 4111), (117, 256, 4112)]


def _subnormal(bits, exp_mask, man_mask):
    return ((bits & exp_mask) == 0) & ((bits & man_mask) != 0)


@pytest.mark.parametrize('nout,k,seed', CASES)
def test_bf16x3_terms(nout, k, seed):
    W = wr.matrix(nout, k, seed)
    assert np.all(W != np.round(W)), 'the matrices are non-integer'
    h, m, l = wr.split_bf16x3(W)
    total = wr.bf16_value(h).astype(np.float64) + wr.bf16_value(m).astype(np.float64) + wr.bf16_value(l).astype(np.float64)
    assert np.all(np.abs(total - W.astype(np.float64)) <= 2.0 ** -24 * np.abs(W.astype(np.float64)))
    assert np.count_nonzero(wr.bf16_value(m)) > W.size // 2 and np.count_nonzero(wr.bf16_value(l)) > W.size // 4
    for t in (h, m, l):
        assert not _subnormal(t, 0x7F80, 0x007F).any()
    # the rounding itself: to nearest (half an ulp of 8 significant bits is at most 2^-8 of the value), against float64
    assert np.all(np.abs(wr.bf16_value(h).astype(np.float64) - W) <= 2.0 ** -8 * np.abs(W))


@pytest.mark.parametrize('nout,k,seed', CASES)
def test_f16x2_terms_of_the_scaled_form(nout, k, seed):
    W = wr.matrix(nout, k, seed)
    s = wr.pow2_scale(W)
    assert 2.0 ** 9 <= np.abs(W).max() * s < 2.0 ** 10 and np.frexp(s)[0] == 0.5
    V = (W * s).astype(np.float32)
    assert np.array_equal(V.astype(np.float64), W.astype(np.float64) * float(s)), 'a power of two scales exactly'
    hi, lo = wr.split_f16x2(V)
    total = hi.view(np.float16).astype(np.float64) + lo.view(np.float16).astype(np.float64)
    assert np.all(np.abs(total - V) <= 2.0 ** -21 * np.abs(V).max(axis=1, keepdims=True))
    assert np.count_nonzero(lo.view(np.float16)) > W.size // 2
    for t in (hi, lo):
        assert not _subnormal(t, 0x7C00, 0x03FF).any() and np.isfinite(t.view(np.float16)).all()


def test_negative_zero_splits_to_one_negative_zero():
    h, m, l = wr.split_bf16x3(np.array([-0.0, 0.0], dtype=np.float32))
    assert h.tolist() == [0x8000, 0] and m.tolist() == [0, 0] and l.tolist() == [0, 0]


@pytest.mark.parametrize('planes', (3, 2))
def test_layout(planes):
    """every element of the image of a (300, 40 -> 64) matrix, found by the formula written out as loops"""
    nout, kvalid, K = 300, 40, 64
    W = wr.matrix(nout, kvalid, 4120)
    scale = wr.pow2_scale(W) if planes == 2 else None
    img = wr.images(W, K=K, planes=planes, scale=scale).view(np.uint16)
    assert img.size == 2 * 2 * planes * 4 * 256 * 8
    terms = wr.split_bf16x3(W) if planes == 3 else wr.split_f16x2(W * scale)
    seen = np.zeros(img.size, dtype=bool)
    for p in range(planes):
        for n in range(512):
            for k in range(K):
                at = (((((n // 256) * 2 + k // 32) * planes + p) * 4 + (k % 32) // 8) * 256 + n % 256) * 8 + k % 8
                assert not seen[at]
                seen[at] = True
                want = terms[p][n, k] if (n < nout and k < kvalid) else 0
                assert img[at] == want, (p, n, k)
    assert seen.all()
