"""The backward of the Swin window-attention core (include/vkn_wattn_train.h) restated for the tests: the header's formulas written out per
window on tensors that are FORMED as tests/swin_ref.py forms them (pad, roll, partition, gathered bias, painted mask), in the dtype of the
inputs (float64 for the yardstick).  Nothing here shares the index arithmetic of csrc/vkn_swin_bwd.hip.  Also the autograd arm that the
formulas and the kernel are judged against, the seeded `dout`, and the case builder of the addressing test.

The bias gradient has two parts and they are kept apart: the part through PAD tokens (their k and v ARE the bias), which is what the
kernel's `dqkv_bias` holds and what `swin_ref.core` differentiates its `qkv_bias` argument to, and the part through real tokens, which is
the sum of the rows of `dqkv` (the `qkv` Linear's own backward)."""
import torch
import torch.nn.functional as F

import swin_ref as R


def seeded_dout(case, seed=0):
    """the gradient of the core's output: a seeded randn [B, H, W, heads 32] in fp32"""
    g = torch.Generator().manual_seed(3000 + seed + case['H'] * 131 + case['W'] * 17 + case['heads'])
    return torch.randn((case['B'], case['H'], case['W'], case['heads'] * R.HD), generator=g)


def formulas(qkv, qkv_bias, table, dout, heads, ws, shift, scale):
    """qkv [B, H, W, 3, heads, hd], qkv_bias [3 heads hd] or None, table [(2 ws - 1)^2, heads], dout [B, H, W, heads hd] ->
    dict(dqkv in qkv's shape, dbias_pad [3 heads hd] (zeros without a bias), dbias_real [3 heads hd], dtable in table's shape)"""
    B, H, W = qkv.shape[:3]
    hd = qkv.shape[-1]
    C = heads * hd
    N = ws * ws
    pad_r, pad_b = (ws - W % ws) % ws, (ws - H % ws) % ws
    x = F.pad(qkv.reshape(B, H, W, 3 * C), (0, 0, 0, pad_r, 0, pad_b))
    _, Hp, Wp, _ = x.shape
    live = F.pad(torch.ones((B, H, W, 1), dtype=qkv.dtype, device=qkv.device), (0, 0, 0, pad_r, 0, pad_b))
    if qkv_bias is not None:
        x = x + (1 - live) * qkv_bias.to(qkv.dtype).view(1, 1, 1, -1)
    do = R._windows_of(F.pad(dout, (0, 0, 0, pad_r, 0, pad_b)), ws, shift)                  # rows of pad queries: dout = 0
    win = R._windows_of(x, ws, shift).reshape(-1, N, 3, heads, hd).permute(2, 0, 3, 1, 4)     # [3, B nW, heads, N, hd]
    q, k, v = win[0] * scale, win[1], win[2]
    do = do.reshape(-1, N, heads, hd).permute(0, 2, 1, 3)                                    # [B nW, heads, N, hd]
    rel = R.rel_index(ws).to(qkv.device)
    s = q @ k.transpose(-2, -1) + table[rel.view(-1)].view(N, N, heads).permute(2, 0, 1).unsqueeze(0)
    if shift > 0:
        mask = R.painted_mask(H, W, ws, shift, qkv.dtype).to(qkv.device)
        s = (s.view(B, -1, heads, N, N) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, N, N)
    P = torch.softmax(s, dim=-1)
    dP = do @ v.transpose(-2, -1)
    delta = (P * dP).sum(-1, keepdim=True)
    dS = P * (dP - delta)
    dv = P.transpose(-2, -1) @ do
    dq = scale * (dS @ k)
    dk = dS.transpose(-2, -1) @ q
    dtable = torch.zeros_like(table).index_add_(0, rel.view(-1), dS.sum(0).permute(1, 2, 0).reshape(N * N, heads))
    dwin = torch.stack((dq, dk, dv)).permute(1, 3, 0, 2, 4).reshape(-1, N, 3 * C)            # [B nW, N, 3 C]
    live_w = R._windows_of(live, ws, shift)                                                  # [B nW, N, 1]
    dqkv = R._map_of(dwin, ws, shift, Hp, Wp, H, W).reshape(qkv.shape)
    dbias_pad = (dwin * (1 - live_w)).sum((0, 1)) if qkv_bias is not None else torch.zeros(3 * C, dtype=qkv.dtype, device=qkv.device)
    return dict(dqkv=dqkv, dbias_pad=dbias_pad, dbias_real=(dwin * live_w).sum((0, 1)), dtable=dtable)


def run_formulas(case, dout, dtype=torch.float64, device='cpu'):
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)      # noqa: E731
    return formulas(to(case['qkv']), to(case['qkv_bias']), to(case['table']), to(dout), case['heads'], case['window'], case['shift'], case['scale'])


def autograd_grads(case, dout, dtype=torch.float64, device='cpu'):
    """torch autograd on `swin_ref.core` -> dict(dqkv, dbias_pad, dbias_total, dtable) on the CPU in float64.  Two leaves stand for the
    bias: `pad` is core's `qkv_bias` (pad tokens only), `real` is added to every row of qkv as an exact zero (real - real.detach()), so
    that its gradient is the sum over the real tokens' rows without changing a value."""
    to = lambda t: None if t is None else t.to(device=device, dtype=dtype)      # noqa: E731
    qkv, table = to(case['qkv']).requires_grad_(), to(case['table']).requires_grad_()
    has_bias = case['qkv_bias'] is not None
    pad = to(case['qkv_bias']).requires_grad_() if has_bias else None
    real = torch.zeros(3 * case['heads'] * R.HD, dtype=dtype, device=device, requires_grad=True)
    rows = qkv + (real - real.detach()).view(3, case['heads'], R.HD)
    out = R.core(rows, pad, table, case['heads'], case['window'], case['shift'], case['scale'])
    (out * to(dout)).sum().backward()
    cpu = lambda t: t.detach().double().cpu()                                   # noqa: E731
    dpad = cpu(pad.grad) if has_bias else torch.zeros_like(cpu(real.grad))
    return dict(dqkv=cpu(qkv.grad), dbias_pad=dpad, dbias_total=dpad + cpu(real.grad), dtable=cpu(table.grad))


# ------------------------------------------------------------------------------------------------ the addressing cases
ADDRESSING_CASES = ('sel_nine_regions', 'sel_pad_shift', 'sel_pad_noshift', 'sel_small_map', 'sel_window4')      # the single-offset selector cases
# non-zero dv rows (one per (token, head)) of float64 autograd on each of them, every one exactly one dout row
ADDRESSING_ROWS = dict(sel_nine_regions=672, sel_pad_shift=420, sel_pad_noshift=140, sel_small_map=15, sel_window4=144)


def addressing_case(name):
    """-> (case, dout): a selector case and a seeded dout that is ZERO on undecided queries (lead < DECIDED_LEAD) and on queries whose
    winner is a pad token.  The softmax of every query left is exactly one-hot in fp32, so a real key's dv row is zero or exactly the
    dout row of the one query it wins."""
    case = R.selector_case(name)
    _, det = R.run_core(case, torch.float64, 'cpu', details=True)
    keep = (det['lead'] >= R.DECIDED_LEAD) & ~det['winner_pad']                             # [B, H, W, heads]
    dout = seeded_dout(case, seed=7).view(case['B'], case['H'], case['W'], case['heads'], R.HD) * keep.unsqueeze(-1)
    return case, dout.reshape(case['B'], case['H'], case['W'], -1).contiguous()
