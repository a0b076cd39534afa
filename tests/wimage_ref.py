"""The split weight tile image restated in numpy, independently of csrc/vkn_wimage.h: what tests/test_gpu_wimage.py compares the
library's writers with, byte for byte, and whose premises tests/test_wimage_refs.py checks on the CPU.

  * the split: v = p[0] + p[1] (+ p[2]), each term the rounding of what the earlier ones left, the remainders in fp32.  bf16 is
    round-to-nearest-even on the fp32 bit pattern, fp16 is `np.float16`;
  * the layout of the images of a matrix Wm [Nout][K] (K % 32 == 0): byte-wise `[nt][kt][plane][k >> 3][row][k & 7]` 2-byte elements,
    nt = n >> 8 over ceil(Nout / 256) tiles of 256 rows, kt = k >> 5 over K / 32 tiles, row = n & 255; rows >= Nout and k >= kvalid are
    zeros in every plane.
No value may be NaN / infinite (the bf16 rounding below does not handle them); the test matrices are `matrix()`.
"""
import numpy as np


def bf16_bits(x):
    """fp32 array -> the uint16 bit patterns of its round-to-nearest-even bf16"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def bf16_value(bits):
    return (bits.astype(np.uint32) << 16).view(np.float32)


def split_bf16x3(v):
    """(h, m, l) as uint16 bit patterns"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    h = bf16_bits(v)
    r1 = (v - bf16_value(h)).astype(np.float32)
    m = bf16_bits(r1)
    r2 = (r1 - bf16_value(m)).astype(np.float32)
    return h, m, bf16_bits(r2)


def split_f16x2(v):
    """(hi, lo) as uint16 bit patterns"""
    v = np.ascontiguousarray(v, dtype=np.float32)
    hi = v.astype(np.float16)
    lo = (v - hi.astype(np.float32)).astype(np.float32).astype(np.float16)
    return hi.view(np.uint16), lo.view(np.uint16)


def pow2_scale(W):
    """the power of two that puts the matrix's largest magnitude at [2^9, 2^10) (1 for a zero matrix): the fp16 form's scale"""
    m = float(np.abs(W).max())
    return np.float32(1.0) if m == 0.0 else np.float32(2.0 ** (10 - np.frexp(m)[1]))


def images(Wm, K=None, planes=3, scale=None):
    """The images (uint8 array) of the matrix Wm [Nout][kvalid] fp32, zero-padded to K >= kvalid columns (K % 32 == 0).
    planes = 3: bf16; planes = 2: fp16 of Wm * scale."""
    Wm = np.asarray(Wm, dtype=np.float32)
    nout, kvalid = Wm.shape
    K = kvalid if K is None else K
    assert K % 32 == 0 and K >= kvalid and planes in (2, 3)
    nt, kt = (nout + 255) // 256, K // 32
    full = np.zeros((nt * 256, K), dtype=np.float32)
    full[:nout, :kvalid] = Wm if scale is None else (Wm * np.float32(scale)).astype(np.float32)
    terms = split_bf16x3(full) if planes == 3 else split_f16x2(full)
    n, k = np.arange(nt * 256)[:, None], np.arange(K)[None, :]
    out = np.empty(nt * kt * planes * 4 * 256 * 8, dtype=np.uint16)
    for p, t in enumerate(terms):
        out[((((((n >> 8) * kt + (k >> 5)) * planes + p) * 4 + ((k & 31) >> 3)) * 256 + (n & 255)) * 8 + (k & 7))] = t
    return out.view(np.uint8)


def matrix(nout, k, seed):
    """A seeded non-integer test matrix [nout][k]: sign * j * 2^(e - 19) with j uniform in [2^19, 2^20) and e in -3 .. 1 — twenty
    significant bits over five binades in [2^-3, 4).  Twenty bits, so that the bf16 middle and low terms (bits 9 - 16 and 17 - 20) are
    mostly nonzero, and the low fp16 term of the scaled form (a multiple of 2^-19 of the value's binade, which the scale puts at 2^5 or
    higher) is zero or at least 2^-14: no plane holds a subnormal."""
    g = np.random.default_rng(seed)
    j = g.integers(1 << 19, 1 << 20, size=(nout, k)).astype(np.float32)
    e = g.integers(-3, 2, size=(nout, k)).astype(np.float32)
    s = np.where(g.integers(0, 2, size=(nout, k)) == 0, np.float32(-1), np.float32(1))
    return (s * j * np.exp2(e - 19).astype(np.float32)).astype(np.float32)


# (Nout, K) of the single-matrix cases: two column tiles (the second with 212 dead rows) x two k tiles; exactly one tile; a single row
SHAPES = ((300, 64), (256, 32), (1, 32))
