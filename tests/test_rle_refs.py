"""tests/rle_ref.py, the restatement of COCO's run-length encoding that judges the device encoder (include/vkn_rle.h): known answers
computed from the format's statement, round trips through the string and the mask, and the 5-bit group edges of the delta code."""
import numpy as np
import pytest

import rle_ref as R


def _case_5x7():
    m = np.zeros((5, 7), dtype=bool)
    m[1:4, 2:5] = True
    m[0, 0] = True
    m[4, 6] = True
    return m


def test_known_answers():
    # the two 1-D examples of the reference's comment (external/ext/mask.py:10-11): a row read as W = 1 column
    assert R.counts(np.array([0, 0, 1, 1, 1, 0, 1])[:, None]) == [2, 3, 1, 1]
    assert R.counts(np.array([1, 1, 1, 1, 1, 1, 0])[:, None]) == [0, 6, 1]
    assert R.counts(np.zeros((2, 2))) == [4] and R.encode(np.zeros((2, 2)))['counts'] == b'4'
    assert R.counts(np.ones((2, 2))) == [0, 4] and R.encode(np.ones((2, 2)))['counts'] == b'04'
    assert R.to_string([1080 * 1920]) == b'PPYo1' and R.to_string([0, 720 * 1280]) == b'0PPTl0'
    m = _case_5x7()
    assert R.counts(m) == [0, 1, 10, 3, 2, 3, 2, 3, 10, 1] and R.encode(m) == {'size': [5, 7], 'counts': b'01:2H0008N'}
    assert R.area(m) == 11 and R.bbox(m) == [0, 0, 7, 5] and R.bbox(np.zeros((3, 4))) == [0, 0, 0, 0]
    big = [5, 2 ** 31 - 10, 1, 3]
    assert R.to_string(big) == b'5fooooo11]PPPPPN' and R.from_string(b'5fooooo11]PPPPPN') == big
    for s in (b'4', b'04', b'PPYo1', b'0PPTl0', b'01:2H0008N'):
        assert R.to_string(R.from_string(s)) == s


def test_column_major_order_and_bbox():
    m = np.zeros((3, 4), dtype=bool)
    m[2, 1] = True                                                     # p = 1 * 3 + 2
    assert R.counts(m) == [5, 1, 6] and R.bbox(m) == [1, 2, 1, 1] and R.area(m) == 1
    m[0, 2] = True                                                     # p = 6: the last pixel of column 1 and the first of column 2 are one run
    assert R.counts(m) == [5, 2, 5] and R.bbox(m) == [1, 0, 2, 3]


def test_round_trips_on_random_masks():
    rng = np.random.default_rng(20240611)
    for _ in range(400):
        h, w = int(rng.integers(1, 41)), int(rng.integers(1, 41))
        m = rng.random((h, w)) < rng.choice([0.0, 0.02, 0.2, 0.5, 0.8, 0.98, 1.0])
        c = R.counts(m)
        assert sum(c) == h * w and all(x > 0 for x in c[1:]) and c[0] >= 0
        assert len(c) == 1 + int(np.count_nonzero(np.diff(np.concatenate([[0], m.reshape(-1, order='F').astype(np.int8)]))))
        s = R.to_string(c)
        assert R.from_string(s) == c and len(s) <= 7 * len(c)
        assert np.array_equal(R.decode(c, h, w), m) and R.counts(R.decode(R.from_string(s), h, w)) == c
        assert R.area(m) == sum(c[1::2])


@pytest.mark.parametrize('delta,nbytes', R.DELTA_EDGES)
def test_delta_code_group_edges(delta, nbytes):
    base = (1 << 20) + 100
    cnts = [3, 4, base, 9, base + delta]
    s = R.to_string(cnts)
    assert len(s) == len(R.to_string(cnts[:4])) + nbytes and R.from_string(s) == cnts
    assert len(R.to_string([1, 2, 3, 3 + 0])) == 4                     # delta 0 is one byte


def test_delta_edge_run_list_hits_every_edge_with_its_byte_count():
    cnts, hits = R.delta_edge_counts()
    assert [(d, n) for _, d, n in hits] == list(R.DELTA_EDGES) and sum(cnts) < 1 << 21
    for i, d, n in hits:
        assert i > 2 and cnts[i] - cnts[i - 2] == d
        assert len(R.to_string(cnts[:i + 1])) - len(R.to_string(cnts[:i])) == n
    m = R.decode(cnts, sum(cnts), 1)
    assert R.counts(m) == cnts and R.from_string(R.to_string(cnts)) == cnts
