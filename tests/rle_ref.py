"""COCO run-length encoding restated in NumPy / plain Python: the yardstick of the device encoder (include/vkn_rle.h states the format).

pycocotools is not installed here and its source is not part of the reference tree (external/ext/mask.py:3 imports it, :10-15 documents
the format), so this is a restatement from the format's description, checked by the known answers and round trips of
tests/test_rle_refs.py; a pycocotools run on real results remains the decisive check.

  counts(mask)        run lengths in column-major order, starting with the zeros
  to_string(counts)   the compressed string (bytes): 5-bit groups, deltas against counts[i-2] behind run 2
  from_string(s)      its inverse
  decode(counts, h, w) the mask, bool [h, w]
  area(mask), bbox(mask)   set pixels; [x0, y0, w, h] over them, zeros for an empty mask
  encode(mask)        {'size': [h, w], 'counts': bytes}, as pycocotools' `encode` returns it
"""
import numpy as np


def counts(mask):
    m = np.asarray(mask) != 0
    assert m.ndim == 2
    v = m.reshape(-1, order='F').astype(np.int8)                       # p = x * H + y
    pos = np.flatnonzero(np.diff(np.concatenate([np.zeros(1, np.int8), v])))      # v[p] != v[p-1], v[-1] = 0
    return [int(c) for c in np.diff(np.concatenate([[0], pos, [v.size]]))]


def to_string(cnts):
    out = bytearray()
    for i, c in enumerate(cnts):
        x = int(c)
        if i > 2:
            x -= int(cnts[i - 2])
        while True:
            c5 = x & 31
            x >>= 5                                                    # arithmetic: Python's >> floors
            more = (x != -1) if (c5 & 16) else (x != 0)
            if more:
                c5 |= 32
            out.append(c5 + 48)
            if not more:
                break
    return bytes(out)


def from_string(s):
    cnts, p = [], 0
    while p < len(s):
        x, k, more = 0, 0, True
        while more:
            c = s[p] - 48
            x |= (c & 31) << (5 * k)
            more = bool(c & 32)
            p += 1
            k += 1
            if not more and (c & 16):
                x |= -1 << (5 * k)
        if len(cnts) > 2:
            x += cnts[-2]
        cnts.append(x)
    return cnts


def decode(cnts, h, w):
    assert sum(cnts) == h * w and all(c >= 0 for c in cnts)
    flat = np.repeat(np.arange(len(cnts)) % 2 == 1, cnts)
    return flat.reshape(h, w, order='F')


def area(mask):
    return int(np.count_nonzero(mask))


def bbox(mask):
    ys, xs = np.nonzero(np.asarray(mask))
    if ys.size == 0:
        return [0, 0, 0, 0]
    return [int(xs.min()), int(ys.min()), int(xs.max() - xs.min() + 1), int(ys.max() - ys.min() + 1)]


def encode(mask):
    m = np.asarray(mask)
    return {'size': [int(m.shape[0]), int(m.shape[1])], 'counts': to_string(counts(m))}


# The 5-bit group edges of the delta code: x = counts[i] - counts[i-2] takes g bytes for -16 * 32^(g-1) <= x < 16 * 32^(g-1).
DELTA_EDGES = ((-17, 2), (-16, 1), (15, 1), (16, 2), (-513, 3), (-512, 2), (511, 2), (512, 3), (1 << 20, 5), (-(1 << 20), 5))


def delta_edge_counts(start=1200, filler=7):
    """(counts, [(run index, delta, bytes)]): a run list whose deltas hit every edge of DELTA_EDGES in turn.  The even runs carry the
    deltas (each is the even run before it plus the next delta), the odd runs are `filler` (delta 0 behind run 2); every count stays
    positive, the long run comes last but one."""
    cnts, hits = [1, filler, start], []
    for d, nbytes in DELTA_EDGES:
        cnts.append(filler)
        cnts.append(cnts[-2] + d)
        hits.append((len(cnts) - 1, d, nbytes))
    assert all(c > 0 for c in cnts)
    return cnts, hits
