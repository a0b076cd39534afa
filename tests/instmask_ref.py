"""Float64 reference of the fused instance-mask rescale (`vkn_instance_bits_f32`, include/vkn_instmask.h), the bit layout of
csrc/vkn_maskbits.h in numpy, and seeded builders of inputs whose thresholded answer is DECIDED: |p64 - thr| >= FLOOR, the project's own
number (tests/pan_joint_ref.py).  The premises — no undecided pixel in the partition cases, an undecided share under the cap in the
noise cases, torch's fp32 composition within 7e-6 of float64 — are asserted on the CPU by tests/test_instmask_refs.py.  No GPU here."""
import numpy as np
import torch
import torch.nn.functional as F

from pan_joint_ref import FLOOR

UNDECIDED_CAP = 1e-3      # share of a noise case's pixels that may be left out of a comparison: a cap, not a tolerance
K_CASE = 5

# name: (Hm, Wm, up, batch_input, img, ori)
GEOMS = {
    'base': (12, 20, 4, (48, 80), (48, 80), (48, 80)),
    'crop_down': (12, 20, 4, (48, 80), (45, 77), (37, 65)),               # crop, down-scale, one bit past a strip
    'up_scale': (12, 20, 2, (24, 40), (23, 38), (61, 130)),
    'kitti_ragged': (6, 39, 4, (24, 156), (24, 156), (24, 155)),
    'one_row': (1, 20, 4, (4, 80), (4, 80), (9, 70)),
    'strong_down': (12, 20, 1, (96, 160), (90, 150), (20, 33)),           # under a strip
    'identity': (16, 16, 1, (16, 16), (16, 16), (16, 16)),
    'anisotropic': (24, 40, 4, (96, 160), (90, 160), (45, 200)),
    'vipseg': (23, 40, 4, (92, 160), (90, 160), (180, 320)),
    'strip_64': (12, 20, 4, (48, 80), (46, 78), (40, 64)),                # Wo exactly one strip
    'strip_128': (12, 32, 4, (48, 128), (46, 126), (40, 128)),           # Wo exactly two strips
}
# the first seed of 0..11 at which the premises of tests/test_instmask_refs.py hold
PARTITION_SEED = {**{n: 0 for n in GEOMS}, 'crop_down': 1, 'vipseg': 1}
NOISE_SEED = {**{n: 0 for n in GEOMS}, 'strong_down': 1}
NOISE_THRS = (0.5, 0.3)
NOISE_SHARE = 3.1e-4      # what the seeds above reach: the undecided share of every noise case, both thresholds
F32_ERR = 7e-6            # torch's own fp32 composition against float64, every case
# Non-finite logits.  Every level of this geometry changes the size in both directions: torch's CPU kernels copy a level whose size stays
# (a NaN stays one pixel), the library evaluates v0 * w0 + v1 * w1 there too (a zero weight spreads it by one pixel, as torch's device
# kernel does), so only where every level resamples do the two agree on which pixels are NaN.
NONFINITE_GEOM = (12, 20, 2, (48, 80), (45, 77), (37, 65))


def meta_of(geom):
    _, _, _, bis, img, ori = geom
    return dict(img_shape=(img[0], img[1], 3), batch_input_shape=tuple(bis), ori_shape=(ori[0], ori[1], 3))


def chain(logits, meta, up, rows=None, dtype=torch.float64):
    """interp(interp(sigmoid(interp_up(logits[rows])), batch_input_shape)[:h, :w], ori_shape) in `dtype` on the CPU -> [K, Ho, Wo] numpy.
    The float64 chain is tests/pan_joint_ref.py's (joint_ref, the resampling chain)."""
    x = torch.as_tensor(logits).detach().cpu().to(dtype)
    if rows is not None:
        x = x[torch.as_tensor(np.asarray(rows)).long()]
    x = x[None]
    if up > 1:
        x = F.interpolate(x, scale_factor=up, mode='bilinear', align_corners=False)
    h, w = meta['img_shape'][:2]
    x = F.interpolate(x.sigmoid(), size=tuple(meta['batch_input_shape']), mode='bilinear', align_corners=False)[:, :, :h, :w]
    return F.interpolate(x, size=tuple(meta['ori_shape'][:2]), mode='bilinear', align_corners=False)[0].numpy()


def decide(p64, thr):
    """(mask, decided): the reference's `>` against the fp32 threshold, and the pixels at least FLOOR away from it.  A NaN pixel is
    not set and counts as decided: nothing rounds a NaN to a number."""
    t = float(np.float32(thr))
    with np.errstate(invalid='ignore'):
        return p64 > t, (np.abs(p64 - t) >= FLOOR) | np.isnan(p64)


# ---- the bit layout of csrc/vkn_maskbits.h: bits[K][strips][H] uint64, bit c of a word = column 64 * strip + c
def strips_of(W):
    return (W + 63) // 64


def pack_bits(masks):
    m = np.asarray(masks).astype(bool)
    K, H, W = m.shape
    NS = strips_of(W)
    pad = np.zeros((K, H, NS * 64), dtype=np.uint64)
    pad[:, :, :W] = m
    words = (pad.reshape(K, H, NS, 64) << np.arange(64, dtype=np.uint64)).sum(-1, dtype=np.uint64)      # disjoint bits: the sum is the OR
    return np.ascontiguousarray(words.transpose(0, 2, 1))


def unpack_bits(bits, W):
    """-> (masks bool [K,H,W], tail: True if any bit behind W is set)"""
    b = np.asarray(bits).view(np.uint64) if np.asarray(bits).dtype != np.uint64 else np.asarray(bits)
    K, NS, H = b.shape
    assert NS == strips_of(W)
    full = ((b.transpose(0, 2, 1)[..., None] >> np.arange(64, dtype=np.uint64)) & np.uint64(1)).astype(bool).reshape(K, H, NS * 64)
    return full[:, :, :W], bool(full[:, :, W:].any())


# ---- inputs
def partition_logits(Hm, Wm, N, seed, cell=3):
    """Every row owns cells of the low-res map: +8 in its cells, -8 elsewhere, plus uniform noise of +-0.5 (pan_joint_ref.partition_case)."""
    rng = np.random.default_rng(seed)
    ncy, ncx = -(-Hm // cell), -(-Wm // cell)
    owners = rng.integers(0, N, size=(ncy, ncx))
    own = np.repeat(np.repeat(owners, cell, 0), cell, 1)[:Hm, :Wm]
    lg = np.where(own[None] == np.arange(N)[:, None, None], 8.0, -8.0) + rng.uniform(-0.5, 0.5, size=(N, Hm, Wm))
    return torch.from_numpy(np.ascontiguousarray(lg, dtype=np.float32))


def noise_logits(Hm, Wm, N, seed):
    rng = np.random.default_rng(1000 + seed)
    return torch.from_numpy((4.0 * rng.standard_normal((N, Hm, Wm))).astype(np.float32))


def build(geom, logits, thr, rows=None, name=None):
    """The reference of one input at geometry `geom` (a name of GEOMS or a tuple): float64 probabilities, the mask, the decided pixels"""
    if isinstance(geom, str):
        name, geom = geom, GEOMS[geom]
    meta = meta_of(geom)
    p64 = chain(logits, meta, geom[2], rows)
    mask, decided = decide(p64, thr)
    return dict(name=name, geom=geom, meta=meta, up=geom[2], logits=logits, rows=rows, thr=float(thr), p64=p64, mask=mask, decided=decided,
                undecided=float(1.0 - decided.mean()))


_CACHE = {}


def partition(name, K=K_CASE):
    """A partition case: compared on EVERY pixel, so the builder asserts that none is undecided.  Built once, shared: read-only."""
    key = ('p', name, K)
    if key not in _CACHE:
        Hm, Wm = GEOMS[name][:2]
        c = build(name, partition_logits(Hm, Wm, K, PARTITION_SEED[name]), 0.5)
        assert c['decided'].all(), f'partition case {name}: {int((~c["decided"]).sum())} undecided pixels'
        _CACHE[key] = c
    return _CACHE[key]


def noise(name, thr, K=K_CASE):
    key = ('n', name, K, float(thr))
    if key not in _CACHE:
        Hm, Wm = GEOMS[name][:2]
        c = build(name, noise_logits(Hm, Wm, K, NOISE_SEED[name]), thr)
        assert c['undecided'] <= UNDECIDED_CAP, f'noise case {name} thr {thr}: undecided share {c["undecided"]:.2e} above the cap'
        _CACHE[key] = c
    return _CACHE[key]


def rows_case(N=100, seed=3):
    """N partition rows (2 x 2 cells) at the first geometry, every pixel decided, for the `rows` arms: the caller indexes p64 / mask."""
    key = ('r', N, seed)
    if key not in _CACHE:
        Hm, Wm = GEOMS['base'][:2]
        c = build('base', partition_logits(Hm, Wm, N, seed, cell=2), 0.5)
        assert c['decided'].all()
        _CACHE[key] = c
    return _CACHE[key]


def nonfinite_case():
    """Noise logits with isolated NaN, +inf and -inf entries, two of them in corners, at NONFINITE_GEOM (every level resamples).
    sigmoid(+-inf) is 1 / 0; a NaN makes every pixel that taps it NaN, and NaN > thr is False."""
    if 'nf' not in _CACHE:
        Hm, Wm = NONFINITE_GEOM[:2]
        lg = noise_logits(Hm, Wm, 3, 5).clone()
        lg[0, 5, 7], lg[0, 2, 15], lg[0, 9, 3] = float('nan'), float('inf'), float('-inf')
        lg[1, 0, 0], lg[1, 11, 19] = float('nan'), float('inf')                      # corners
        lg[2, 6, 10] = float('-inf')
        c = build(NONFINITE_GEOM, lg, 0.5, name='nonfinite')
        assert np.isnan(c['p64']).any() and c['undecided'] <= UNDECIDED_CAP
        _CACHE['nf'] = c
    return _CACHE['nf']


CASES = [('partition', n, 0.5) for n in GEOMS] + [('noise', n, t) for n in GEOMS for t in NOISE_THRS]


def get(kind, name, thr):
    return partition(name) if kind == 'partition' else noise(name, thr)
