"""Caller-owned memory for the C ABI, as a C caller would hand it over: plain module, runs on CPU tensors too (tests/test_abi_arena.py).

`include/vkn.h` promises that the library allocates nothing, that scratch is the caller's `ws` of `vkn_*_workspace_bytes` bytes and that
every output is caller memory of exactly the stated shape.  The Python binding cannot show a breach: `ops._workspace` only grows and
`torch.empty` rounds its blocks up.  An `Arena` is ONE int32 tensor filled with the NaN-payload sentinel 0x7FC0BEEF out of which outputs
(`out`) and workspaces (`ws`) of EXACTLY the asked size are carved, each between guards of max(64 KiB, its own size) (at most 4 MiB):
an overrun by a whole row, plane or tile still lands in a guard.  `check` then asserts
  * every output range holds no sentinel word (it was written, all of it),
  * every byte outside the carved ranges still holds the sentinel's bits (nothing else was written),
  * a workspace range may hold anything.
`frozen` asserts that the (`const`) inputs of a call are bitwise what they were.

Ranges are requested first and the tensor is allocated at the first use of one of them (`.ptr`, `.t`, `check`): the arena is as large as
its ranges and guards need, no larger."""
import contextlib
import ctypes

import torch

SENT = 0x7FC0BEEF                         # a quiet NaN with a payload no arithmetic produces (as fp32; two NaNs as fp16)
SENT_BYTES = SENT.to_bytes(4, 'little')
GUARD_MIN, GUARD_MAX = 64 << 10, 4 << 20
BASE_ALIGN = 256


def guard_bytes(nbytes):
    """the guard before and behind a range of `nbytes`: a condition on the test, not a measurement"""
    return min(max(GUARD_MIN, int(nbytes)), GUARD_MAX)


class Range:
    """one carved range: `nbytes` bytes at byte offset `off` of the arena, an output (`shape`, `dtype`) or a workspace"""

    def __init__(self, arena, kind, name, nbytes, align, skew, shape=None, dtype=None, full=True):
        assert kind in ('out', 'ws') and nbytes >= 0 and align & (align - 1) == 0 and 0 <= skew < align and BASE_ALIGN % align == 0
        self.arena, self.kind, self.name, self.nbytes, self.align, self.skew = arena, kind, name, int(nbytes), align, skew
        self.shape, self.dtype, self.full, self.off = shape, dtype, full, None

    @property
    def addr(self):
        """the range's address (0 for an empty range: an empty workspace is NULL to a C caller)"""
        self.arena._materialise()
        return self.arena.base_addr + self.off if self.nbytes else 0

    @property
    def ptr(self):
        return ctypes.c_void_p(self.addr or None)

    @property
    def bytes(self):
        self.arena._materialise()
        return self.arena.u8[self.off:self.off + self.nbytes]

    @property
    def t(self):
        """the output as a tensor of its shape and dtype: a view of the arena's memory"""
        assert self.kind == 'out'
        return self.bytes.view(self.dtype).view(self.shape)


class Arena:
    def __init__(self, device):
        self.device, self.ranges, self.buf = torch.device(device), [], None

    # ---- carving
    def _add(self, r):
        assert self.buf is None, 'carve every range before the first of them is used'
        assert all(q.name != r.name for q in self.ranges), r.name
        self.ranges.append(r)
        return r

    def out(self, shape, dtype=torch.float32, name=None, align=16, skew=0, full=True):
        """a contiguous output of exactly prod(shape) elements; its start is `align`-byte aligned, + `skew` bytes (align=16, skew=8: 8-byte
        but not 16-byte aligned).  full=False: the entry documents that it may leave part of it unwritten."""
        shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list, torch.Size)) else (shape,)))
        n = 1
        for s in shape:
            n *= s
        return self._add(Range(self, 'out', name or f'out{len(self.ranges)}', n * torch.empty((), dtype=dtype).element_size(), align, skew,
                               shape, dtype, full))

    def ws(self, nbytes, name=None, align=256, skew=0):
        """a workspace of exactly `nbytes` bytes (the size query's answer, not rounded)"""
        return self._add(Range(self, 'ws', name or f'ws{len(self.ranges)}', nbytes, align, skew))

    def _materialise(self):
        if self.buf is not None:
            return
        cur, behind = 0, 0
        for r in self.ranges:
            g = guard_bytes(r.nbytes)
            cur += max(g, behind)                               # the guard between two ranges serves both: the larger of the two
            cur += (r.skew - cur) % r.align
            r.off, cur, behind = cur, cur + r.nbytes, g
        total = cur + behind
        words = (total + 3) // 4 + BASE_ALIGN // 4
        self.buf = torch.full((words,), SENT, dtype=torch.int32, device=self.device)
        lead = (-self.buf.data_ptr()) % BASE_ALIGN                # offsets are relative to a BASE_ALIGN-aligned address
        assert lead % 4 == 0
        self.words = self.buf[lead // 4: lead // 4 + (total + 3) // 4]
        self.u8 = self.words.view(torch.uint8)
        self.base_addr, self.total = self.words.data_ptr(), total
        for r in self.ranges:
            assert (self.base_addr + r.off) % r.align == r.skew and r.off >= guard_bytes(r.nbytes) and r.off + r.nbytes + guard_bytes(r.nbytes) <= total

    # ---- checking
    def _stray(self, a, b):
        """byte offsets in [a, b) that no longer hold the sentinel's bits (sorted, the first few)"""
        a4, b4 = min(b, (a + 3) // 4 * 4), max(a, b // 4 * 4)
        bad = []
        edge = list(range(a, a4)) + list(range(max(b4, a4), b))
        if edge:
            vals = self.u8[torch.tensor(edge, device=self.device)].cpu().tolist()
            bad += [o for o, v in zip(edge, vals) if v != SENT_BYTES[o % 4]]
        if b4 > a4:
            w = self.words[a4 // 4:b4 // 4]
            idx = (w != SENT).nonzero().reshape(-1)
            if idx.numel():
                for o in sorted({a4 + 4 * int(i) for i in idx[:4].cpu().tolist() + [int(idx[-1])]}):      # the bytes of those words
                    bad += [o + j for j, v in enumerate(self.u8[o:o + 4].cpu().tolist()) if v != SENT_BYTES[j]]
        return sorted(set(bad))

    def problems(self):
        """every breach as one line; empty when the call kept the contract"""
        self._materialise()
        if self.device.type == 'cuda':
            torch.cuda.synchronize()
        out = []
        order = sorted(self.ranges, key=lambda r: r.off)
        edges = [0] + [e for r in order for e in (r.off, r.off + r.nbytes)] + [self.total]
        for i in range(0, len(edges), 2):                       # the gaps: before the first range, between ranges, behind the last
            before, behind = (order[i // 2 - 1] if i else None), (order[i // 2] if i // 2 < len(order) else None)
            for o in self._stray(edges[i], edges[i + 1])[:3]:
                d_before = o - edges[i] if before is not None else None
                d_behind = edges[i + 1] - o if behind is not None else None
                if d_behind is None or (d_before is not None and d_before < d_behind):
                    out.append(f'stray write {d_before} bytes behind the end of {before.kind} "{before.name}" ({before.nbytes} bytes)')
                else:
                    out.append(f'stray write {d_behind} bytes before the start of {behind.kind} "{behind.name}" ({behind.nbytes} bytes)')
        for r in order:
            if r.kind == 'out' and r.full and r.nbytes >= 4:
                w = r.bytes[:r.nbytes // 4 * 4].view(torch.int32)
                left = (w == SENT).nonzero().reshape(-1)
                if left.numel():
                    out.append(f'out "{r.name}": {int(left.numel())} of {w.numel()} words were not written, the first at byte {4 * int(left[0])}')
        return out

    def check(self, name):
        bad = self.problems()
        assert not bad, f'{name}: ' + '; '.join(bad)


@contextlib.contextmanager
def frozen(*tensors, **named):
    """the tensors (inputs of a call: `const` in the C ABI) are bitwise unchanged when the block ends"""
    items = [(f'input {i}', t) for i, t in enumerate(tensors) if t is not None] + [(k, t) for k, t in named.items() if t is not None]
    before = [t.detach().clone() for _, t in items]
    yield
    if any(t.is_cuda for _, t in items):
        torch.cuda.synchronize()
    for (label, t), b in zip(items, before):
        same = torch.equal(t.detach().contiguous().reshape(-1).view(torch.uint8), b.contiguous().reshape(-1).view(torch.uint8))
        assert same, f'{label} was modified by a call that takes it as const'
