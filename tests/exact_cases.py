"""Integer-valued operands and integer references for the LINEAR kernels (gather, decode, the fused pass, up-scaling, the GEMM engine,
the FPN conv): plain module, importable without a GPU.

Why integers.  With small-integer (or dyadic) operands
  * every operand is the HIGH term of the f16 hi+lo split and of the bf16x3 split (the low terms are exactly 0),
  * every product and every partial sum is an integer below 2^24, so fp32 accumulation is exact IN ANY ORDER,
  * power-of-two range management is exact, bilinear x2 / x4 weights are k/4 and k/8 (outputs are multiples of 1/64),
  * a thresholded integer logit is never within rounding of thr_logit (8.94e-8): there are no near-tie bit flips.
So a kernel must reproduce the float64 reference BIT FOR BIT at any shape; one wrong element is a hard failure that names its index.

Every case carries two checks that are evaluated on the CPU, from the actual operands, before anything is launched:
  premise      max over outputs of sum |terms| < 2^24 (fp16 outputs: every value fits an 11-bit significand).  A case that violates it
               is a bug in the TEST and fails as such (`PremiseError`).
  non-vacuity  the outputs are not all zero; thresholded cases have an ON share in [0.05, 0.95] over the whole mask, and
               `special_rows` names the rows that are deliberately all-off, all-on and single-pixel.

References are float64 (exact for these integers: every sum is far below 2^53) and written as plainly as possible: einsum, conv2d,
F.interpolate and its autograd."""
import collections
import math

import torch
import torch.nn.functional as F

TWO24 = float(1 << 24)
THR = 8.940696716308594e-08            # ops.thr_logit(0.5): sigmoid(z) > 0.5 as ATen's fp32 sigmoid evaluates it; an integer z is ON iff z >= 1

N_EDGES = (1, 31, 32, 33, 100, 117, 128, 129, 166, 256)       # 256: the largest N every [B, N, C, P] entry point accepts (include/vkn.h)
P_EDGES = (1, 2, 62, 64, 66, 126, 128, 130, 135)
P_LARGE = (7488, 32768)                                        # a KITTI-STEP frame (48 x 156), cfg2 (128 x 256): once per op
C_ALL = (32, 64, 96, 128, 160, 224, 256)
B_ALL = (1, 2, 5)
# P as 1 x P and as H x W with W odd (ragged rows): both forms of every ragged P occur in the sweep
HW_OF = {1: ((1, 1),), 2: ((1, 2),), 62: ((1, 62), (2, 31)), 64: ((1, 64), (8, 8)), 66: ((1, 66), (6, 11)), 126: ((1, 126), (14, 9)),
         128: ((1, 128), (8, 16)), 130: ((1, 130), (10, 13)), 135: ((1, 135), (9, 15)), 7488: ((48, 156),), 32768: ((128, 256),)}

Shape = collections.namedtuple('Shape', 'B N C H W seed large')


class PremiseError(AssertionError):
    """the case itself is wrong (not the kernel): its sums leave the exact range of fp32, or it checks nothing"""


def sid(s):
    return f'B{s.B}_N{s.N}_C{s.C}_{s.H}x{s.W}'


def bncp_sweep(large=True):
    """The shape sweep of the [B, N, C, H W] ops: every pair (N edge, P edge) at C = 64 and C = 256, every other C at three pairs,
    every B of B_ALL, the two large P once."""
    out, seed = [], 1000
    for C in (64, 256):
        for i, N in enumerate(N_EDGES):
            for j, P in enumerate(P_EDGES):
                hw = HW_OF[P][(i + (C == 256)) % len(HW_OF[P])]
                B = 5 if N == 1 else B_ALL[(i + j) % 3]                 # (one row: five frames, so that the ON share is no coin toss)
                seed += 1
                out.append(Shape(B, N, C, hw[0], hw[1], seed, False))
    for C in (32, 96, 128, 160, 224):
        for (B, N, hw) in ((2, 117, (9, 15)), (1, 33, (8, 8)), (5, 129, (10, 13))):
            seed += 1
            out.append(Shape(B, N, C, hw[0], hw[1], seed, False))
    if large:
        for P in P_LARGE:
            seed += 1
            out.append(Shape(1, 117, 256, HW_OF[P][0][0], HW_OF[P][0][1], seed, True))
    return out


def sweep_covers():
    """the coverage the sweep promises, as data (test_exact_premise.py asserts it)"""
    s = bncp_sweep()
    pairs = {(c.C, c.N, c.H * c.W) for c in s}
    return dict(N={c.N for c in s}, C={c.C for c in s}, P={c.H * c.W for c in s}, B={c.B for c in s}, pairs=pairs,
                forms={(c.H * c.W, c.H == 1) for c in s})


# ------------------------------------------------------------------------------------------------------------------- operands
def gen(seed):
    return torch.Generator(device='cpu').manual_seed(int(seed))


def ints(shape, lo, hi, g, denom=1):
    """uniform integers in [lo, hi] (divided by the power of two `denom`: dyadic fractions), fp32, from the CPU generator `g`"""
    assert denom & (denom - 1) == 0
    return (torch.randint(lo, hi + 1, tuple(shape), generator=g, dtype=torch.int64).double() / denom).float()


SPECIAL_MIN_N = 31      # below this many rows a frame has no special rows (they would decide the ON share)


def special_rows(N, P):
    """name -> (row, pixels ON) of the deliberately degenerate mask rows: all-off, all-on, and one pixel ON at p = 0, p = P - 1 and at
    the 64- / 128-pixel tile edges p = 63 / 64 / 127 / 128 where P allows.  Rows at both ends of the N range."""
    if N < SPECIAL_MIN_N:
        return {}
    rows = dict(all_off=(0, ()), all_on=(1, tuple(range(P))), one_p0=(2, (0,)), one_plast=(N - 1, (P - 1,)))
    for name, row, p in (('one_p63', 3, 63), ('one_p64', N - 2, 64), ('one_p127', 4, 127), ('one_p128', N - 3, 128)):
        if p < P:
            rows[name] = (row, (p,))
    return rows


def mask_logits(B, N, P, g, span=8):
    """integer mask logits [B, N, P] in [-span, span] (0 is OFF: 0 < thr_logit) with the `special_rows` in every frame"""
    z = ints((B, N, P), -span, span, g)
    for row, on in special_rows(N, P).values():
        z[:, row] = -float(span)
        for p in (on if len(on) < P else ()):
            z[:, row, p] = float(span)
        if len(on) == P:
            z[:, row] = float(span)
    if N < SPECIAL_MIN_N:                       # a one-row mask: pixel 0 ON in the even frames, OFF in the odd ones (no coin toss)
        z[0::2, 0, 0], z[1::2, 0, 0] = float(span), -float(span)
    return z


# ------------------------------------------------------------------------------------------------------------------- checks
def premise(name, *abs_sums, limit=TWO24):
    """every sum of |terms| (float64 tensors, from the actual operands) stays below 2^24"""
    for t in abs_sums:
        m = float(t.max()) if t.numel() else 0.0
        if not m < limit:
            raise PremiseError(f'{name}: max sum |terms| = {m:.6g} >= {limit:.6g}: fp32 accumulation is not exact in every order — fix the CASE')


def premise_f16(name, ref, unit):
    """fp16 outputs: every value is a multiple of `unit` (a power of two >= 2^-14) and |v| / unit < 2^11, so it fits fp16's significand"""
    q = ref.double() / unit
    if not (bool((q == q.round()).all()) and float(q.abs().max()) < 2048 and unit >= 2.0 ** -14):
        raise PremiseError(f'{name}: the reference values do not fit fp16 exactly')
    assert torch.equal(ref.double(), ref.half().double()), name


def non_vacuous(name, *outs):
    for t in outs:
        if not bool((t != 0).any()):
            raise PremiseError(f'{name}: an output is all zero: the case checks nothing')


def on_share(name, bits):
    s = float(bits.double().mean())
    if not 0.05 <= s <= 0.95:
        raise PremiseError(f'{name}: ON share {s:.3f} outside [0.05, 0.95]')
    return s


def check_special_rows(name, bits, N, P):
    """the special rows really are what their names say, in the REFERENCE mask"""
    for key, (row, on) in special_rows(N, P).items():
        want = torch.zeros(P, dtype=torch.bool)
        want[list(on)] = True
        if not bool((bits[:, row] == want).all()):
            raise PremiseError(f'{name}: special row {key} (row {row}) is not as named')


# ------------------------------------------------------------------------------------------------------------------- references
def _e(eq, a, b):
    return torch.einsum(eq, a.double(), b.double())


def gather_case(s, x_span=8, xdenom=1):
    """binarised gather: x [B, C, H, W] integers, z [B, N, H, W] integer logits -> (x, z, xraw [B, N, C], cnt [B, N]) float64"""
    g = gen(s.seed)
    P = s.H * s.W
    x = ints((s.B, s.C, P), -x_span, x_span, g, xdenom)
    z = mask_logits(s.B, s.N, P, g)
    bits = z >= THR
    xraw, cnt = _e('bnp,bcp->bnc', bits, x), bits.double().sum(-1)
    name = 'gather ' + sid(s)
    premise(name, _e('bnp,bcp->bnc', bits, x.abs()) * xdenom, cnt)
    non_vacuous(name, xraw, cnt)
    on_share(name, bits)
    check_special_rows(name, bits, s.N, P)
    return x.view(s.B, s.C, s.H, s.W), z.view(s.B, s.N, s.H, s.W), xraw, cnt


def gather_real_case(s, denom=1):
    """real-operand gather: a [B, N, P] integers / denom (denom = 16: dyadic k/16) -> (x, a, out [B, N, C], asum [B, N])"""
    g = gen(s.seed + 7)
    P = s.H * s.W
    x = ints((s.B, s.C, P), -8, 8, g)
    a = ints((s.B, s.N, P), -8 * denom, 8 * denom, g, denom)
    out, asum = _e('bnp,bcp->bnc', a, x), a.double().sum(-1)
    name = f'gather_real/{denom} ' + sid(s)
    premise(name, _e('bnp,bcp->bnc', a.abs(), x.abs()) * denom, a.double().abs().sum(-1) * denom)
    non_vacuous(name, out)
    return x.view(s.B, s.C, s.H, s.W), a.view(s.B, s.N, s.H, s.W), out, asum


def decode_case(s, bias=True, x_span=8):
    """decode: x integers, kernels [B, N, C] integers in [-8, 8], integer bias [B, N] -> (x, k, bias | None, out [B, N, H, W])"""
    g = gen(s.seed + 13)
    P = s.H * s.W
    x = ints((s.B, s.C, P), -x_span, x_span, g)
    k = ints((s.B, s.N, s.C), -8, 8, g)
    kb = ints((s.B, s.N), -64, 64, g) if bias else None
    out = _e('bnc,bcp->bnp', k, x) + (kb.double()[..., None] if bias else 0.0)
    name = 'decode ' + sid(s)
    premise(name, _e('bnc,bcp->bnp', k.abs(), x.abs()) + (kb.double().abs()[..., None] if bias else 0.0))
    non_vacuous(name, out)
    return x.view(s.B, s.C, s.H, s.W), k, kb, out.view(s.B, s.N, s.H, s.W)


def fused_case(s, x_span=8):
    """decode -> threshold -> gather: (x, k, bias, z [B, N, P], xraw [B, N, C], cnt [B, N]).  Integer bias in [-3, 3] (the logits are
    symmetric about it: ON share about one half); row 0 is all-off (zero kernel, bias -1), row 1 all-on (zero kernel, bias +1) where
    N >= SPECIAL_MIN_N."""
    g = gen(s.seed + 29)
    P = s.H * s.W
    x = ints((s.B, s.C, P), -x_span, x_span, g)
    k = ints((s.B, s.N, s.C), -8, 8, g)
    kb = ints((s.B, s.N), -3, 3, g)
    if s.N >= SPECIAL_MIN_N:
        k[:, 0:2] = 0
        kb[:, 0], kb[:, 1] = -1.0, 1.0
    else:                                       # one row: all-on in frame 0, all-off in frame 1, the other frames as drawn
        k[0:2] = 0
        kb[0], kb[1] = 1.0, -1.0
    z = _e('bnc,bcp->bnp', k, x) + kb.double()[..., None]
    bits = z >= THR
    xraw, cnt = _e('bnp,bcp->bnc', bits, x), bits.double().sum(-1)
    name = 'fused ' + sid(s)
    premise(name, _e('bnc,bcp->bnp', k.abs(), x.abs()) + kb.double().abs()[..., None], _e('bnp,bcp->bnc', bits, x.abs()), cnt)
    non_vacuous(name, xraw, cnt)
    on_share(name, bits)
    if s.N >= SPECIAL_MIN_N:
        if bool(bits[:, 0].any()) or not bool(bits[:, 1].all()):
            raise PremiseError(name + ': rows 0 / 1 are not all-off / all-on')
    return x.view(s.B, s.C, s.H, s.W), k, kb, z, xraw, cnt


# ---- up-scaling
UP_FWD = [(2, 3, 1, 1, 2), (1, 5, 2, 3, 2), (2, 2, 3, 5, 4), (1, 3, 7, 16, 2), (1, 2, 9, 15, 4), (1, 4, 12, 39, 2), (2, 3, 17, 64, 4),
          (1, 2, 33, 7, 2), (1, 1, 48, 156, 4), (1, 3, 5, 1, 4), (1, 2, 1, 6, 2), (1, 2, 16, 128, 2)]      # (B, N, H, W, S); W S % 4 != 0 among them
UP_BWD = [(B, N, H, W, S) for (B, N, H, W, _) in [(2, 3, 1, 1, 0), (1, 5, 2, 3, 0), (1, 2, 9, 15, 0), (1, 3, 7, 64, 0), (1, 2, 12, 39, 0),
                                                  (1, 1, 5, 128, 0)] for S in (1, 2, 4, 8)]
UP_PLANES = [(32768 + 5, H, W) for (H, W) in ((1, 1), (2, 3), (3, 2), (1, 2), (3, 3))]       # the launchers' second `chunk` iteration


def up_case(B, N, H, W, S, seed, f16=False):
    """F.interpolate(scale_factor=S, bilinear, align_corners=False) of integers in [-16, 16]: (m [B, N, H, W], out float64)"""
    m = ints((B, N, H, W), -16, 16, gen(seed))
    out = F.interpolate(m.double(), scale_factor=S, mode='bilinear', align_corners=False)
    name = f'up x{S} {B}x{N}x{H}x{W}'
    unit = 1.0 / (4 * S * S)                       # weights are k / (2 S) per axis: outputs are multiples of 1 / (4 S^2)
    q = out / unit
    if not bool((q == q.round()).all()):
        raise PremiseError(name + ': outputs are not multiples of 1 / (4 S^2)')
    premise(name, F.interpolate(m.double().abs(), scale_factor=S, mode='bilinear', align_corners=False) / unit)
    non_vacuous(name, out)
    if f16:
        premise_f16(name, out, unit)
    return m, out


def up_bwd_case(B, N, H, W, S, seed):
    """the adjoint, by autograd of F.interpolate in float64: (g [B, N, H S, W S] integers in [-16, 16], grad_in float64)"""
    go = ints((B, N, H * S, W * S), -16, 16, gen(seed))

    def adj(t):
        z = torch.zeros((B, N, H, W), dtype=torch.float64, requires_grad=True)
        F.interpolate(z, scale_factor=S, mode='bilinear', align_corners=False).backward(t)
        return z.grad

    out = adj(go.double())
    name = f'up_bwd x{S} {B}x{N}x{H}x{W}'
    premise(name, adj(go.double().abs()) * (4 * S * S))        # the weights are non-negative multiples of 1 / (4 S^2)
    non_vacuous(name, out)
    return go, out


# ---- GEMM engine.  A covering subset of M x K x Nout (every value of each axis at least once, the extremes together)
GEMM_M = (1, 31, 32, 33, 117, 129, 234, 468, 512, 513, 704, 936)
GEMM_K = (32, 64, 256, 512, 768, 2048)
GEMM_NOUT = (1, 19, 32, 33, 124, 256, 257, 2048)


def gemm_shapes():
    out, seen = [], set()

    def add(M, K, Nn):
        if (M, K, Nn) not in seen:
            seen.add((M, K, Nn))
            out.append((M, K, Nn))

    for i, M in enumerate(GEMM_M):                       # every M with two K and two Nout, rotating
        add(M, GEMM_K[i % 6], GEMM_NOUT[i % 8])
        add(M, GEMM_K[(i + 3) % 6], GEMM_NOUT[(i + 5) % 8])
    for K in GEMM_K:                                     # every (K, Nout) pair at a row count on a tile edge
        for j, Nn in enumerate(GEMM_NOUT):
            add((33, 117, 129)[j % 3], K, Nn)
    add(936, 2048, 2048)
    add(1, 2048, 1)
    add(513, 2048, 256)
    add(512, 768, 257)
    return out


def linear_case(M, K, Nout, seed, act=0, bias=True):
    """y = act(A W^T + b), integers in [-4, 4]: (A [M, K], W [Nout, K], b | None, y float64)"""
    g = gen(seed)
    A, W = ints((M, K), -4, 4, g), ints((Nout, K), -4, 4, g)
    b = ints((Nout,), -16, 16, g) if bias else None
    y = A.double() @ W.double().t() + (b.double() if bias else 0.0)
    if act:
        y = y.clamp_min(0)
    name = f'linear M{M} K{K} N{Nout}'
    premise(name, A.double().abs() @ W.double().abs().t() + (b.double().abs() if bias else 0.0))
    non_vacuous(name, y)
    return A, W, b, y


def linear_bwd_case(M, K, Nout, seed, act=0, wt=False):
    """forward and the three gradients of y = act(A Wm^T + b) under an integer upstream gradient dy; wt: the weight is stored
    transposed ([K, Nout], y = A W + b).  -> dict of fp32 operands and float64 references (W / dW in the STORED orientation)."""
    g = gen(seed)
    A, Wm = ints((M, K), -4, 4, g), ints((Nout, K), -4, 4, g)
    b = ints((Nout,), -16, 16, g)
    dy = ints((M, Nout), -4, 4, g)
    b[0] = 5.0 - float(A[0].double() @ Wm[0].double())      # y[0, 0] = 5 and dy[0, 0] = 3 whatever was drawn: a 1 x 1 output is no coin toss
    dy[0, 0] = 3.0
    pre = A.double() @ Wm.double().t() + b.double()
    y = pre.clamp_min(0) if act else pre
    if float((dy.double() * (pre > 0) if act else dy.double())[:, 0].sum()) == 0:
        dy[0, 0] = 4.0                                       # (... nor is the bias gradient of a one-column layer)
    dye = dy.double() * (pre > 0) if act else dy.double()
    da, dW, db = dye @ Wm.double(), dye.t() @ A.double(), dye.sum(0)
    name = f'linear_bwd M{M} K{K} N{Nout} act{act} wt{int(wt)}'
    premise(name, A.double().abs() @ Wm.double().abs().t() + b.double().abs(), dye.abs() @ Wm.double().abs(), dye.abs().t() @ A.double().abs(),
            dye.abs().sum(0))
    non_vacuous(name, y, da, dW, db)
    return dict(A=A, W=Wm.t().contiguous() if wt else Wm, b=b, dy=dy, y=y, da=da, dW=dW.t().contiguous() if wt else dW, db=db)


# ---- the weight-gradient kernels called on their own (tests/test_gpu_chain_blocks.py): strided operands, accumulate, the batch form
DW_SHAPES = [(1, 1, 1), (5, 33, 19), (117, 256, 19), (129, 64, 300), (468, 2048, 256), (3744, 256, 512)]
DW_BATCH_M = 129
DW_BATCH_ITEMS = (1, 3, 48)          # 48 = VKN_DW_MAX_ITEMS


def dw_case(M, K, Nout, seed):
    """dW = dy^T A, db = column sums of dy on integers in [-4, 4], and integer `old` values of dW / db in [-16, 16] for the accumulating
    form: (dy [M, Nout], A [M, K], old_w [Nout, K], old_b [Nout], dW float64, db float64).  Premise: every sum of |terms|, the old
    value included, stays below 2^24."""
    g = gen(seed)
    dy, A = ints((M, Nout), -4, 4, g), ints((M, K), -4, 4, g)
    old_w, old_b = ints((Nout, K), -16, 16, g), ints((Nout,), -16, 16, g)
    dy[0, 0], A[0, 0] = 3.0, 2.0
    if float((dy.double().t() @ A.double())[0, 0]) == 0 or float(dy.double()[:, 0].sum()) == 0:   # (a 1 x 1 output is no coin toss)
        dy[0, 0] = 4.0
    dW, db = dy.double().t() @ A.double(), dy.double().sum(0)
    name = f'dw M{M} K{K} N{Nout}'
    premise(name, dy.double().abs().t() @ A.double().abs() + old_w.double().abs(), dy.double().abs().sum(0) + old_b.double().abs())
    non_vacuous(name, dW, db)
    return dy, A, old_w, old_b, dW, db


def dw_batch_shapes(nitems):
    """(K, Nout) of the items of a batch launch: ragged against the 64 x 128 tiles of the batch kernel"""
    pool = [(33, 19), (64, 64), (128, 65), (1, 1), (129, 7), (256, 130), (40, 63)]
    return [pool[i % len(pool)] for i in range(nitems)]


# ---- FPN conv (the raw conv output of conv_gn; its statistics are not linear: test_gpu_semantic_fpn.py judges them per tensor,
#      test_gpu_fpn_conv_pins.py per group)
CONV_SIZES = ((1, 1), (2, 3), (3, 5), (12, 39), (47, 155), (48, 156))


def conv_shapes():
    """(B, C, H, W, ksize, stride, mode): every size x kernel x stride x mode at one C / B, every C and B at least once per kernel"""
    out, i = [], 0
    for (H, W) in CONV_SIZES:
        for ks in (1, 3):
            for stride in (1, 2):
                for mode in ('raw', 'pos'):
                    big = H * W > 1000
                    C = (32, 64) [i % 2] if big else (32, 64, 256)[i % 3]
                    out.append(((1, 2, 3)[(i // 2) % 3] if not big else (1, 2)[i % 2], C, H, W, ks, stride, mode))
                    i += 1
    out += [(1, 256, 48, 156, 3, 1, 'pos'), (2, 256, 47, 155, 3, 2, 'raw'), (1, 256, 47, 155, 1, 1, 'raw')]
    return out


def conv_case(B, C, H, W, ks, stride, mode, seed, Cout=None):
    """(x [B, C, H, W], pos [C, H, W] | None, w [Cout, C, ks, ks], out float64): conv2d(x + pos, w, stride, padding = ks // 2);
    Cout = C unless given"""
    g = gen(seed)
    Cout = C if Cout is None else Cout
    x = ints((B, C, H, W), -4, 4, g)
    pos = ints((C, H, W), -4, 4, g) if mode == 'pos' else None
    w = ints((Cout, C, ks, ks), -2, 2, g)
    xin = x.double() + (pos.double() if pos is not None else 0.0)
    out = F.conv2d(xin, w.double(), stride=stride, padding=ks // 2)
    name = f'conv B{B} C{C}->{Cout} {H}x{W} k{ks} s{stride} {mode}'
    premise(name, F.conv2d(xin.abs(), w.double().abs(), stride=stride, padding=ks // 2))
    non_vacuous(name, out)
    return x, pos, w, out


# ---- FPN conv, per element (tests/test_gpu_fpn_conv_pins.py): the on-load transforms, Cin != Cout, single-pixel probes.
# The engine works on 64-pixel runs of an output row, two 32-column MFMA blocks each; a wave owns two 32-row blocks of Cout, a grid
# slice 256 rows.  Output widths around those edges, and the (Cin, Cout) pairs that leave a wave with ONE 32-row block (Cout = 32, 96,
# 160, 288), fill both 256-row grid slices (Cout = 512) or run sixteen 32-channel chunks (Cin = 512):
FPN_WO = (1, 31, 32, 33, 63, 64, 65, 128, 129)
FPN_H = (1, 2, 3, 5)
FPN_CC = ((32, 32), (64, 96), (96, 160), (32, 288), (512, 32), (256, 512))
FPN_KS = ((3, 1), (3, 2), (1, 1))                 # (ksize, stride): a strided 1x1 conv is outside the envelope

FpnCase = collections.namedtuple('FpnCase', 'B Cin Cout H W ks stride mode in_groups low seed')   # H x W: the SOURCE map (x)


def fpn_id(c):
    return f'{c.mode}{"_low" if c.low else ""}_B{c.B}_{c.Cin}to{c.Cout}_{c.H}x{c.W}_k{c.ks}s{c.stride}_g{c.in_groups}'


def fpn_out_hw(c):
    """(Hin, Win, Ho, Wo): the conv input ('up': 2H x 2W) and the output map (3x3 pad 1 and 1x1 pad 0: ceil(n / stride))"""
    Hin, Win = (2 * c.H, 2 * c.W) if c.mode == 'up' else (c.H, c.W)
    return Hin, Win, (Hin - 1) // c.stride + 1, (Win - 1) // c.stride + 1


def _fpn_src_w(mode, Wo, stride):
    """the source width that gives output width Wo (None: impossible — 'up' at stride 1 has Wo = 2 W), and the odd / even variant"""
    if mode == 'up':
        return Wo if stride == 2 else (Wo // 2 if Wo % 2 == 0 else None)
    return Wo if stride == 1 else 2 * Wo - (Wo % 2)          # stride 2: Win = 2 Wo - 1 (odd) for odd Wo, 2 Wo (even) for even Wo


def fpn_norm_shapes(mode):
    """mode 'norm' / 'up': every (ksize, stride) at every output width of FPN_WO that the mode can produce.  The other axes rotate with
    the WIDTH index, shifted per kernel variant, so that no axis is locked to a variant: along the widths every (ksize, stride) meets
    every (Cin, Cout) pair, every in_groups form and every B (fpn_covers is the promise, test_exact_premise.py asserts it); then the
    named edge cases."""
    out, i = [], 0
    for wi, Wo in enumerate(FPN_WO):
        for ki, (ks, stride) in enumerate(FPN_KS):
            W = _fpn_src_w(mode, Wo, stride)
            if W is None:
                continue
            Cin, Cout = FPN_CC[(wi + 2 * ki) % len(FPN_CC)]
            heavy = Cin * Cout >= 512 * 256 or Wo > 65
            H = (1, 2)[(wi + ki) % 2] if heavy and mode == 'up' else FPN_H[(wi + ki) % 4]
            B = 1 if heavy else (1, 2, 3)[(wi + 2 * ki) % 3]
            out.append(FpnCase(B, Cin, Cout, H, W, ks, stride, mode, (1, 8, Cin)[(wi + ki) % 3], False, 3000 + 100 * (mode == 'up') + i))
            i += 1
    seed = 3300 + 100 * (mode == 'up')
    if mode == 'up':      # both clamps are zero at Hs = 1 / Ws = 1; a source of one pixel
        extra = [(2, 64, 96, 1, 33, 3, 1, 8), (2, 32, 32, 5, 1, 3, 1, 32), (1, 96, 160, 1, 1, 3, 2, 1), (3, 32, 288, 3, 1, 1, 1, 8),
                 (1, 512, 32, 7, 65, 3, 2, 8), (1, 256, 512, 5, 33, 3, 1, 256)]
    else:                 # stride 2 on odd and on even Hin / Win
        extra = [(2, 64, 96, 3, 5, 3, 1, 8), (1, 32, 32, 5, 129, 3, 2, 32), (3, 96, 160, 2, 130, 3, 2, 1), (1, 32, 288, 4, 66, 3, 2, 8),
                 (1, 512, 512, 2, 64, 1, 1, 512)]
    out += [FpnCase(B, Ci, Co, H, W, ks, st, mode, G, False, seed + j) for j, (B, Ci, Co, H, W, ks, st, G) in enumerate(extra)]
    return out


def fpn_low_shapes():
    """the cases whose staged activations carry bits in the LOW half of the f16 split (share >= FPN_LOW_SHARE, asserted per case; one
    mean per channel where fewer groups leave the share below it)"""
    rows = [('up', 2, 64, 96, 3, 5, 3, 1, 8), ('up', 1, 32, 160, 4, 66, 3, 2, 32), ('up', 1, 96, 32, 3, 32, 1, 1, 96),
            ('up', 1, 32, 288, 2, 65, 3, 2, 32), ('up', 3, 64, 96, 5, 3, 3, 1, 64),
            ('norm', 2, 32, 96, 3, 65, 3, 1, 8), ('norm', 1, 32, 160, 5, 129, 3, 2, 32), ('norm', 3, 32, 32, 2, 64, 1, 1, 1),
            ('norm', 1, 32, 288, 1, 33, 3, 1, 8), ('norm', 1, 32, 512, 3, 63, 3, 2, 1)]
    return [FpnCase(B, Ci, Co, H, W, ks, st, mode, G, True, 3500 + j) for j, (mode, B, Ci, Co, H, W, ks, st, G) in enumerate(rows)]


FPN_LOW_SHARE = 0.2


def fpn_covers(cases):
    """what a list of FpnCase covers, as data"""
    hw = [fpn_out_hw(c) for c in cases]
    return dict(Wo={o[3] for o in hw}, H={c.H for c in cases}, B={c.B for c in cases}, CC={(c.Cin, c.Cout) for c in cases},
                KS={(c.ks, c.stride) for c in cases}, groups={'Cin' if c.in_groups == c.Cin else c.in_groups for c in cases},
                WoKS={(o[3], c.ks, c.stride) for c, o in zip(cases, hw)},
                KS_CC={(c.ks, c.stride, c.Cin, c.Cout) for c in cases},
                KS_groups={(c.ks, c.stride, 'Cin' if c.in_groups == c.Cin else c.in_groups) for c in cases},
                KS_B={(c.ks, c.stride, c.B) for c in cases},
                s2_parity={(o[0] % 2, o[1] % 2) for c, o in zip(cases, hw) if c.stride == 2},
                one_row=any(c.H == 1 for c in cases), one_col=any(c.W == 1 for c in cases))


def fpn_chain(x, stats, gamma, beta, up):
    """what the conv's LOAD does, in x's dtype, as plain torch: GroupNorm from the given (mean, rstd) [B, G, 2] + affine + ReLU, then
    (up) F.interpolate(scale_factor=2, bilinear, align_corners=False).  The operation order is the kernel's: ((v - mean) rstd) gamma + beta."""
    B, C = x.shape[:2]
    cpg = C // stats.shape[1]
    mean = stats[..., 0].repeat_interleave(cpg, 1)[..., None, None].to(x.dtype)
    rstd = stats[..., 1].repeat_interleave(cpg, 1)[..., None, None].to(x.dtype)
    v = ((x - mean) * rstd * gamma.to(x.dtype)[None, :, None, None] + beta.to(x.dtype)[None, :, None, None]).clamp_min(0)
    return F.interpolate(v, scale_factor=2, mode='bilinear', align_corners=False) if up else v


def split_f16(v):
    """the two-term f16 split of the staged activations, restated: hi = f16(v), lo = f16(v - hi), both round-to-nearest-even"""
    v = v.float()
    hi = v.half()
    return hi, (v - hi.float()).half()


def _pow2_unit(t):
    """the largest power of two (<= 1) of which every element of the float64 tensor is a multiple"""
    u = 1.0
    while not bool((t / u == (t / u).round()).all()):
        u /= 2
        if u < 2.0 ** -30:
            raise PremiseError('the operands are not dyadic')
    return u


def fpn_case(c):
    """One 'norm' / 'up' case of dyadic operands -> dict(x, stats [B, G, 2], gamma, beta, w, xin (float64 conv input), out (float64),
    unit, clip, low_share).
      x integers in [-4, 4], mean k/4 in [-1, 1], rstd in {1/2, 1, 2}, gamma in {1/2, 1, 3/2}, beta k/4 in [-1, 1], w integers in [-2, 2]
      low: x integers in [-32, 32], rstd = gamma = 1, mean k/64 ('up') or k/1024 ('norm') in [-1, 1], beta k/4 in [0, 2]
    Every step is then exact in fp32 in any order and under any contraction.  Asserted here, from the operands: every staged value v
    splits exactly (hi + lo == v), max sum (|hi| + |lo|) |w| < 2^24 units of the finest bit (low cases: < 2^23), non-zero outputs, a ReLU clip share in [0.05, 0.95],
    and for low cases a share of staged values with lo != 0 of at least FPN_LOW_SHARE."""
    g = gen(c.seed)
    name = 'fpn ' + fpn_id(c)
    G = c.in_groups
    if c.low:
        x = ints((c.B, c.Cin, c.H, c.W), -32, 32, g)
        den = 64 if c.mode == 'up' else 1024
        mean = ints((c.B, G), -den, den, g, den)
        rstd = torch.ones(c.B, G)
        gamma = torch.ones(c.Cin)
        beta = ints((c.Cin,), 0, 8, g, 4)
    else:
        x = ints((c.B, c.Cin, c.H, c.W), -4, 4, g)
        mean = ints((c.B, G), -4, 4, g, 4)
        rstd = torch.tensor([0.5, 1.0, 2.0])[torch.randint(0, 3, (c.B, G), generator=g)]
        gamma = torch.tensor([0.5, 1.0, 1.5])[torch.randint(0, 3, (c.Cin,), generator=g)]
        beta = ints((c.Cin,), -4, 4, g, 4)
    w = ints((c.Cout, c.Cin, c.ks, c.ks), -2, 2, g)
    stats = torch.stack([mean, rstd], -1).contiguous()
    up = c.mode == 'up'
    pre = fpn_chain(x.double(), stats.double(), gamma.double(), beta.double(), False)
    xin = fpn_chain(x.double(), stats.double(), gamma.double(), beta.double(), up)
    out = F.conv2d(xin, w.double(), stride=c.stride, padding=c.ks // 2)
    unit = _pow2_unit(xin)
    hi, lo = split_f16(xin)
    halves = hi.double().abs() + lo.double().abs()          # the accumulator sees hi w and lo w as separate terms
    premise(name, F.conv2d(halves, w.double().abs(), stride=c.stride, padding=c.ks // 2) / unit, limit=TWO24 / 2 if c.low else TWO24)
    non_vacuous(name, out)
    if not torch.equal(hi.double() + lo.double(), xin):
        raise PremiseError(name + ': a staged value does not split exactly into f16 hi + lo')
    clip = float((pre == 0).double().mean())
    if not 0.05 <= clip <= 0.95:
        raise PremiseError(f'{name}: ReLU clip share {clip:.3f} outside [0.05, 0.95]')
    low_share = float((lo != 0).double().mean())
    if c.low and low_share < FPN_LOW_SHARE:
        raise PremiseError(f'{name}: only {low_share:.3f} of the staged values have a non-zero low half (< {FPN_LOW_SHARE})')
    return dict(x=x, stats=stats, gamma=gamma, beta=beta, w=w, xin=xin, out=out, unit=unit, clip=clip, low_share=low_share)


# dense raw / pos cases (conv_case) at Cin != Cout: (B, Cin, Cout, H, W, ks, stride, mode)
CONV_UNEQ = [(2, 64, 96, 3, 65, 3, 1, 'raw'), (1, 96, 160, 5, 129, 3, 2, 'pos'), (1, 256, 512, 2, 64, 3, 1, 'pos'), (1, 32, 288, 3, 33, 1, 1, 'raw'),
             (1, 512, 32, 2, 31, 3, 2, 'raw'), (3, 32, 96, 1, 1, 3, 1, 'pos'), (1, 64, 160, 3, 130, 3, 2, 'raw'), (1, 512, 512, 2, 64, 1, 1, 'pos')]

# single-pixel probes, modes raw / pos, Cin != Cout: the output is the weight stencil itself, a shifted or dropped tap names itself
FPN_PROBE = [(2, 64, 96, 3, 65, 3, 1), (1, 96, 160, 5, 129, 3, 2), (1, 256, 512, 2, 128, 3, 1), (3, 32, 288, 3, 130, 3, 2), (1, 512, 32, 1, 64, 1, 1),
             (2, 32, 512, 5, 66, 1, 1), (1, 64, 96, 1, 1, 3, 1), (1, 32, 160, 2, 257, 3, 2)]     # (B, Cin, Cout, H, W, ks, stride)


def probe_pixels(H, W, stride):
    """input pixels (y, x) under the image corners and under the first and the last output column of every 64-pixel run"""
    Wo = (W - 1) // stride + 1
    cols = {0, W - 1} | {min(ox * stride, W - 1) for t in range((Wo + 63) // 64) for ox in (64 * t, min(64 * t + 63, Wo - 1))}
    return sorted({(y, x) for y in {0, H - 1, H // 2} for x in cols})


def conv_probe_case(B, Cin, Cout, H, W, ks, stride, mode, seed):
    """(x, pos | None, w [Cout, Cin, ks, ks] integers in [-2, 2] without zeros, out float64, n_probes).  Probe i sits in frame i % B on
    input channel (5 i + 3) % Cin with value 1 + i % 3; mode 'pos': every second probe sits in `pos` instead (shared by the frames)."""
    g = gen(seed)
    x = torch.zeros(B, Cin, H, W)
    pos = torch.zeros(Cin, H, W) if mode == 'pos' else None
    w = ints((Cout, Cin, ks, ks), 1, 2, g) * (ints((Cout, Cin, ks, ks), 0, 1, g) * 2 - 1)
    px = probe_pixels(H, W, stride)
    for i, (y, xx) in enumerate(px):
        ci, v = (5 * i + 3) % Cin, float(1 + i % 3)
        if mode == 'pos' and i % 2:
            pos[ci, y, xx] += v
        else:
            x[i % B, ci, y, xx] += v
    xin = x.double() + (pos.double() if pos is not None else 0.0)
    out = F.conv2d(xin, w.double(), stride=stride, padding=ks // 2)
    name = f'conv probes B{B} {Cin}->{Cout} {H}x{W} k{ks} s{stride} {mode}'
    premise(name, F.conv2d(xin.abs(), w.double().abs(), stride=stride, padding=ks // 2))
    non_vacuous(name, out, *[out[b] for b in range(min(B, len(px)))])
    return x, pos, w, out, len(px)


# ---- autograd of gather / decode: the power-of-two scaling inside the backward must cancel exactly
def pow2_scale_of(t, target_log2=10):
    """the scale ops.pow2_scale / autograd._pow2_scale choose: 2^(target_log2 - e) with max |t| = m 2^e, m in [0.5, 1)"""
    m = float(t.abs().max())
    return 2.0 ** (target_log2 - math.frexp(m)[1]) if m > 0 else 1.0


def decode_grad_case(s):
    """Z = decode(x, K, kb) under an integer upstream gradient dZ: (x, k, kb, dz, dx, dk, dkb) — references float64.  The backward
    scales dZ by a power of two s (max |dZ| s in [512, 1024)) before it enters the f16 split: the premise holds for the SCALED sums."""
    g = gen(s.seed + 41)
    P = s.H * s.W
    x, k, kb = ints((s.B, s.C, P), -8, 8, g), ints((s.B, s.N, s.C), -8, 8, g), ints((s.B, s.N), -8, 8, g)
    dz = ints((s.B, s.N, P), -8, 8, g)
    dx, dk, dkb = _e('bnc,bnp->bcp', k, dz), _e('bnp,bcp->bnc', dz, x), dz.double().sum(-1)
    sc = pow2_scale_of(dz)
    name = 'decode_grad ' + sid(s)
    premise(name, _e('bnc,bnp->bcp', k.abs(), dz.abs()) * sc, _e('bnp,bcp->bnc', dz.abs(), x.abs()) * sc, dz.double().abs().sum(-1) * sc,
            _e('bnc,bcp->bnp', k.abs(), x.abs()) + kb.double().abs()[..., None])
    non_vacuous(name, dx, dk, dkb)
    return x.view(s.B, s.C, s.H, s.W), k, kb, dz.view(s.B, s.N, s.H, s.W), dx.view(s.B, s.C, s.H, s.W), dk, dkb


def gather_grad_case(s):
    """xraw = gather(x, bit(z)) under an integer upstream gradient: (x, z, dxraw [B, N, C], dx [B, C, H, W] float64)"""
    g = gen(s.seed + 43)
    P = s.H * s.W
    x = ints((s.B, s.C, P), -8, 8, g)
    z = mask_logits(s.B, s.N, P, g)
    d = ints((s.B, s.N, s.C), -8, 8, g)
    bits = z >= THR
    dx = _e('bnp,bnc->bcp', bits, d)
    name = 'gather_grad ' + sid(s)
    premise(name, _e('bnp,bnc->bcp', bits, d.abs()) * pow2_scale_of(d), _e('bnp,bcp->bnc', bits, x.abs()))
    non_vacuous(name, dx)
    on_share(name, bits)
    return x.view(s.B, s.C, s.H, s.W), z.view(s.B, s.N, s.H, s.W), d, dx.view(s.B, s.C, s.H, s.W)


GRAD_SHAPES = [Shape(2, 33, 64, 6, 11, 501, False), Shape(1, 117, 256, 8, 16, 502, False), Shape(1, 129, 128, 9, 15, 503, False),
               Shape(2, 100, 256, 16, 64, 504, False), Shape(1, 31, 32, 1, 2, 505, False)]


# ---- kernel-initialisation pass: the outputs that are linear, or linear -> threshold -> linear, in the operands
INIT_SHAPES = [(2, 64, 100, 19, 8, 9, 15), (1, 256, 100, 19, 2, 8, 16), (1, 128, 33, 40, 11, 8, 8), (2, 256, 100, 19, 8, 16, 64),
               (1, 32, 31, 5, 2, 1, 66), (2, 64, 20, 8, 3, 8, 8)]       # (B, C, Np, ncls, n_thing, H, W): the one-pass kernel's two row maps
                                                                         # (100 + 19 rows, everything in 32 rows) and shapes it leaves to the separate form


def init_case(B, C, Np, ncls, n_thing, H, W, seed, cat):
    """(loc, sem, init_w [Np, C], seg_w [ncls, C], seg_b, refs): refs = dict(x_feats, mask_preds [B, N, H, W], seg_preds, prop [B, N, C])
    for use_binary=True; with use_binary=False only x_feats / mask_preds / seg_preds are linear."""
    g = gen(seed)
    P = H * W
    loc, sem = ints((B, C, P), -4, 4, g), ints((B, C, P), -4, 4, g)
    iw, sw, sb = ints((Np, C), -8, 8, g), ints((ncls, C), -8, 8, g), ints((ncls,), -8, 8, g)
    xf = loc.double() + sem.double()
    mp = torch.einsum('nc,bcp->bnp', iw.double(), loc.double())
    seg = torch.einsum('nc,bcp->bnp', sw.double(), sem.double()) + sb.double()[None, :, None]
    bits = mp >= THR
    obj = torch.einsum('bnp,bcp->bnc', bits.double(), xf)
    prop = iw.double()[None] + obj
    if cat:
        mp = torch.cat([mp, seg[:, n_thing:]], 1)
        prop = torch.cat([prop, sw.double()[None, n_thing:].expand(B, -1, -1)], 1)
    name = f'init B{B} C{C} Np{Np} {H}x{W} cat{int(cat)}'
    premise(name, torch.einsum('nc,bcp->bnp', iw.double().abs(), loc.double().abs()),
            torch.einsum('nc,bcp->bnp', sw.double().abs(), sem.double().abs()) + sb.double().abs()[None, :, None],
            torch.einsum('bnp,bcp->bnc', bits.double(), xf.abs()) + iw.double().abs()[None])
    non_vacuous(name, xf, mp, seg, prop)
    on_share(name, bits)
    sh = (B, -1, H, W)
    return (loc.view(B, C, H, W), sem.view(B, C, H, W), iw, sw, sb,
            dict(x_feats=xf.view(B, C, H, W), mask_preds=mp.view(sh), seg_preds=seg.view(sh), prop=prop))


# ---- FPN backward: the two MFMA gradients of the conv alone, bit for bit (tests/test_gpu_fpn_bwd_pins.py).
# k_conv_wgrad deals nruns = B Ho ceil(Wo / 64) pixel runs to nsplit workgroups per (32 ci, 128 co) tile; split sp walks the runs
# nruns sp / nsplit .. nruns (sp + 1) / nsplit and accumulates them into the same tiles.  tests/fpn_bwd_ref.py's cases up to here give
# every split ONE run.  These give a split several: across rows, across frames, full and ragged runs alternating, at stride 2 behind the
# 64-pixel seam (ox0 = 64; dgrad: tx = 1 in both column parities), and more runs than VKN_FPN_WGRAD_MAX_SPLITS.
# shape (B, Cin, Cout, H, W, k, s) -> what the split structure must be (runs, splits, {runs of a split: how many splits}); asserted by
# tests/test_exact_premise.py against the split count READ BACK from the library's workspace size, not restated from the rule.
FPN_BWD_PINS = {
    (3, 512, 512, 3, 65, 3, 1): (18, 4, {4: 2, 5: 2}),            # two splits cross a frame boundary; full and one-pixel runs alternate
    (3, 512, 512, 5, 131, 3, 2): (18, 4, {4: 2, 5: 2}),           # -> 3 x 66: every second run is the 2-pixel run behind the seam
    (2, 512, 512, 3, 65, 1, 1): (12, 4, {3: 4}),                  # the 1x1 kernel
    (3, 256, 256, 9, 65, 3, 1): (54, 16, {3: 10, 4: 6}),          # the shipped channel count
    (1, 32, 32, 33, 65, 3, 1): (66, 64, {1: 62, 2: 2}),           # the MAX_SPLITS clamp; 33 rows in dgrad
}
FPN_BWD_LOW = ((2, 64, 96, 3, 65, 3, 1), (1, 96, 160, 5, 129, 3, 2))
FPN_BWD_LOW_VARIANTS = ('wgrad-dr', 'wgrad-x', 'dgrad-dr', 'dgrad-w')      # kernel - the WIDE operand (the other is in {-1, 0, 1})
FPN_BWD_WIDE = 8191                                               # 13 bits: two more than an f16 significand holds
WGRAD_WS_FIXED = 1536                                             # status header, the two powers of two, the max |v| partials


def fpn_bwd_id(shape, variant=None):
    B, Ci, Co, H, W, k, s = shape
    return f'{variant + "_" if variant else ""}B{B}_{Ci}to{Co}_{H}x{W}_k{k}s{s}'


def wgrad_runs(shape):
    """(nruns, runs per frame) of the weight gradient: 64-pixel runs of the output rows"""
    B, _, _, H, W, _, s = shape
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    return B * Ho * ((Wo + 63) // 64), Ho * ((Wo + 63) // 64)


def wgrad_nsplit_of(ws_bytes, shape):
    """the number of partial tiles in a vkn_conv_wgrad_workspace_bytes answer (include/vkn_fpn_train.h: behind the fixed part the
    workspace holds `splits` fp32 tiles [Cout][Cin k^2], a multiple of 256 bytes at any Cin, Cout of the envelope)"""
    _, Ci, Co, _, _, k, _ = shape
    tile = 4 * Co * Ci * k * k
    assert ws_bytes > WGRAD_WS_FIXED and (ws_bytes - WGRAD_WS_FIXED) % tile == 0, (ws_bytes, shape)
    return (ws_bytes - WGRAD_WS_FIXED) // tile


def wgrad_split_runs(nruns, nsplit):
    """[(first run, one past the last)] per split, k_conv_wgrad's own dealing"""
    return [(nruns * sp // nsplit, nruns * (sp + 1) // nsplit) for sp in range(nsplit)]


def conv_grads(x, w, dr, stride):
    """(dw, dx) of F.conv2d(x, w, padding = k // 2) under the output gradient dr: autograd, in the operands' dtype"""
    xx, ww = x.detach().clone().requires_grad_(), w.detach().clone().requires_grad_()
    dx, dw = torch.autograd.grad(F.conv2d(xx, ww, None, stride, w.shape[-1] // 2), (xx, ww), dr)
    return dw, dx


def _conv_abs_sums(x, w, dr, stride):
    """(sum |terms| of every dw element, of every dx element), float64: the same two gradients of the magnitudes"""
    pad = w.shape[-1] // 2
    return (torch.nn.grad.conv2d_weight(x.double().abs(), w.shape, dr.double().abs(), stride, pad),
            torch.nn.grad.conv2d_input(x.shape, w.double().abs(), dr.double().abs(), stride, pad))


def staged_pow2(t):
    """the power of two under which the backward (and the weight image) stages a tensor: 2^(15 - e), max |v| = f 2^e, f in [0.5, 1)
    (csrc/vkn_convtile.h: pow2_scale)"""
    m = float(t.abs().max())
    return 2.0 ** (15 - math.frexp(m)[1]) if m > 0 else 1.0


def conv_bwd_case(shape, seed, span=3):
    """x, w, dr integers in [-span, span] -> dict(x, w, dr, dw, dx): dw, dx float64 autograd of F.conv2d.  The power of two per tensor
    is exact on them and leaves every low half empty (asserted).  Premise on sum |terms| of dw and of dx, non-vacuity."""
    B, Ci, Co, H, W, k, s = shape
    g = gen(seed)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    x, w, dr = ints((B, Ci, H, W), -span, span, g), ints((Co, Ci, k, k), -span, span, g), ints((B, Co, Ho, Wo), -span, span, g)
    name = 'conv_bwd ' + fpn_bwd_id(shape)
    for t in (x, w, dr):
        if bool((split_f16(t * staged_pow2(t))[1] != 0).any()):
            raise PremiseError(name + ': a staged operand has a non-empty low half')
    premise(name, *_conv_abs_sums(x, w, dr, s))
    dw, dx = conv_grads(x.double(), w.double(), dr.double(), s)
    non_vacuous(name, dw, dx)
    return dict(x=x, w=w, dr=dr, dw=dw, dx=dx)


def conv_bwd_low_case(shape, variant, seed, wide=FPN_BWD_WIDE):
    """One of FPN_BWD_LOW_VARIANTS: the WIDE operand holds integers in [-wide, wide], its partner in the product integers in {-1, 0, 1};
    the third operand (x for dgrad, w for wgrad) is not read by the kernel under test.  The MFMA kernels drop lo * lo: with an empty low
    half on one side hi * hi + hi * lo + lo * hi is the whole product.  Asserted here, from the operands: hi + lo reproduces every staged
    value of the wide operand (v 2^(15 - e)), at least FPN_LOW_SHARE of them have lo != 0, the partner's low halves are empty, and
    max sum (|hi| + |lo|) |partner| < 2^24 in units of the wide operand's finest bit.  -> dict(x, w, dr, out float64, low_share)"""
    B, Ci, Co, H, W, k, s = shape
    kernel, which = variant.split('-')
    g = gen(seed)
    Ho, Wo = (H - 1) // s + 1, (W - 1) // s + 1
    shapes = dict(x=(B, Ci, H, W), w=(Co, Ci, k, k), dr=(B, Co, Ho, Wo))
    partner = {'wgrad': {'dr': 'x', 'x': 'dr'}, 'dgrad': {'dr': 'w', 'w': 'dr'}}[kernel][which]
    t = {n: ints(sh, -wide, wide, g) if n == which else ints(sh, -1, 1, g) for n, sh in shapes.items()}
    name = 'conv_bwd_low ' + fpn_bwd_id(shape, variant)
    sc = staged_pow2(t[which])
    staged = t[which].double() * sc
    hi, lo = split_f16(staged)
    if not torch.equal(hi.double() + lo.double(), staged):
        raise PremiseError(name + ': a staged value does not split exactly into f16 hi + lo')
    halves = (hi.double().abs() + lo.double().abs()) / sc               # the accumulator sees hi p and lo p as separate terms
    if not bool((halves == halves.round()).all()):
        raise PremiseError(name + ': a half is no multiple of the operand\'s finest bit')
    if bool((split_f16(t[partner] * staged_pow2(t[partner]))[1] != 0).any()):
        raise PremiseError(name + ': the narrow operand has a non-empty low half')
    low_share = float((lo != 0).double().mean())
    if low_share < FPN_LOW_SHARE:
        raise PremiseError(f'{name}: only {low_share:.3f} of the staged values have a non-zero low half (< {FPN_LOW_SHARE})')
    mags = {n: (halves if n == which else v.double().abs()) for n, v in t.items()}
    dw_abs, dx_abs = _conv_abs_sums(mags['x'], mags['w'], mags['dr'], s)
    dw, dx = conv_grads(t['x'].double(), t['w'].double(), t['dr'].double(), s)
    out, out_abs = (dw, dw_abs) if kernel == 'wgrad' else (dx, dx_abs)
    premise(name, out_abs)
    non_vacuous(name, out)
    return dict(x=t['x'], w=t['w'], dr=t['dr'], out=out, low_share=low_share)
