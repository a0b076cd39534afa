"""CPU: the arena of tests/abi_arena.py detects what tests/test_gpu_abi_contract.py relies on it to detect — on `device='cpu'`, where a
"kernel" is a line of torch.  Without this the GPU tests could be vacuous."""
import pytest
import torch

import abi_arena as aa


def _arena():
    """three outputs and a workspace, ragged sizes: fp32 [3, 5], fp16 [7] behind an 8-but-not-16-byte-aligned start, int32 [2, 2]"""
    A = aa.Arena('cpu')
    a = A.out((3, 5), torch.float32, name='logits')
    w = A.ws(1000, name='scratch')
    h = A.out((7,), torch.float16, name='half', skew=8)
    i = A.out((2, 2), torch.int32, name='ids')
    return A, a, w, h, i


def _fill(a, h, i):
    a.t.copy_(torch.arange(15.0).view(3, 5))
    h.t.fill_(1.5)
    i.t.fill_(7)


def test_carving_is_exact_aligned_and_guarded():
    A, a, w, h, i = _arena()
    assert (a.nbytes, w.nbytes, h.nbytes, i.nbytes) == (60, 1000, 14, 16)
    assert a.addr % 16 == 0 and w.addr % 256 == 0 and h.addr % 16 == 8 and i.addr % 16 == 0
    assert a.t.shape == (3, 5) and a.t.dtype == torch.float32 and a.t.data_ptr() == a.addr and a.t.is_contiguous()
    assert h.t.dtype == torch.float16 and h.t.numel() == 7 and h.t.data_ptr() == h.addr
    order = sorted(A.ranges, key=lambda r: r.off)
    assert order[0].off >= aa.GUARD_MIN and A.total - (order[-1].off + order[-1].nbytes) >= aa.GUARD_MIN
    for p, q in zip(order, order[1:]):
        assert q.off - (p.off + p.nbytes) >= aa.GUARD_MIN
    assert aa.guard_bytes(1) == 64 << 10 and aa.guard_bytes(1 << 20) == 1 << 20 and aa.guard_bytes(1 << 30) == 4 << 20
    B = aa.Arena('cpu')
    big = B.out((300000,), torch.float32, name='plane')                    # 1.2 MB: its guards are as large as it is
    assert big.addr % 16 == 0 and big.off >= big.nbytes and B.total - big.off - big.nbytes >= big.nbytes
    assert bool((A.words == aa.SENT).all()) and A.words.view(torch.float32).isnan().all()
    with pytest.raises(AssertionError):
        A.out((1,), name='late')                                           # the tensor exists: no further range


def test_a_clean_run_passes_and_the_workspace_may_change():
    A, a, w, h, i = _arena()
    _fill(a, h, i)
    w.bytes.fill_(0xAB)
    A.check('clean')
    assert A.problems() == []
    a.t[1, 2] = float('nan')                                               # an arithmetic NaN is not the sentinel
    A.check('nan output')


@pytest.mark.parametrize('where,words,text', [('before', -1, '4 bytes before the start of out "logits"'), ('behind', 15, '0 bytes behind the end of out "logits"'),
                                              ('far', 15 + 7500, '30000 bytes behind the end of out "logits"')])
def test_a_stray_write_is_reported_with_the_ranges_name(where, words, text):
    A, a, w, h, i = _arena()
    _fill(a, h, i)
    A.words[a.off // 4 + words] = 0
    with pytest.raises(AssertionError) as e:
        A.check('call')
    assert text in str(e.value) and str(e.value).startswith('call: '), str(e.value)


def test_stray_bytes_around_a_ragged_range_and_a_workspace():
    A, a, w, h, i = _arena()
    _fill(a, h, i)
    A.u8[h.off + 14] = 0                                                   # the half-word behind 7 fp16 values
    assert any('0 bytes behind the end of out "half"' in p for p in A.problems())
    A.u8[h.off + 14] = aa.SENT_BYTES[(h.off + 14) % 4]
    A.check('restored')
    A.u8[w.off + 1000] = 1                                                 # one byte past a workspace of exactly 1000 bytes
    assert any('0 bytes behind the end of ws "scratch"' in p for p in A.problems())
    A.u8[w.off + 1000] = aa.SENT_BYTES[(w.off + 1000) % 4]
    A.u8[w.off - 1] ^= 0xFF
    assert any('1 bytes before the start of ws "scratch"' in p for p in A.problems())
    A.u8[w.off - 1] ^= 0xFF
    A.u8[0] = 0                                                            # the very first and the very last byte of the arena
    A.u8[A.total - 1] = 0
    bad = A.problems()
    assert len(bad) == 2 and 'before the start of out "logits"' in bad[0] and 'behind the end of out "ids"' in bad[1], bad


def test_an_unwritten_output_element_is_reported():
    A, a, w, h, i = _arena()
    _fill(a, h, i)
    A.words[a.off // 4 + 7] = aa.SENT                                      # element [1, 2] was skipped
    with pytest.raises(AssertionError) as e:
        A.check('call')
    assert 'out "logits": 1 of 15 words were not written, the first at byte 28' in str(e.value)
    B = aa.Arena('cpu')
    part = B.out((8,), torch.int64, name='rows', full=False)               # an output the entry may fill in part only
    part.t[:3] = 1
    B.check('partial')


def test_a_modified_frozen_input_is_reported():
    x, k = torch.arange(6.0).view(2, 3), torch.ones(4, dtype=torch.int64)
    with aa.frozen(x, None, labels=k):
        y = x * 2 + k[0]
    assert float(y[1, 2]) == 11.0
    with pytest.raises(AssertionError) as e:
        with aa.frozen(x, labels=k):
            x[1, 1] *= 0.5                                                 # a kernel that scales its operand in place
    assert 'input 0 was modified' in str(e.value)
    with pytest.raises(AssertionError) as e:
        with aa.frozen(x, labels=k):
            k[3] = 2
    assert 'labels was modified' in str(e.value)
    z = torch.zeros(3)
    with pytest.raises(AssertionError):
        with aa.frozen(z):
            z[0] = -0.0                                                    # bitwise, not by value
