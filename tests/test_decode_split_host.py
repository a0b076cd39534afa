"""CPU: how a decode launch splits a frame's pixels over workgroups (vkn_decode_px_per_wg, the pure host function behind the launcher and
behind vkn_mask_decode_planes_wg_f32), by default and under a workgroup budget."""
import pytest

GRAN = 512      # pixels: 8 waves x 64-px tiles
CUS = 256       # workgroups of the default persistent grid


def _default_px(B, P):
    """the launcher's rule before budgets existed: ceil(B * P / 256) pixels per workgroup, in 512-px steps"""
    ppx = -(-B * P // CUS)
    return max(GRAN, -(-ppx // GRAN) * GRAN)


def _g2(P, px):
    return -(-P // px)


BENCH_P = 128 * 256
SIZES = [(B, BENCH_P) for B in (1, 2, 4, 8, 16, 32)] + [   # every size bench.py runs the head at
    (2, 16 * 32), (2, 2048), (2, 2560),                     # the GPU tests' sizes
    (1, 23 * 40), (3, 1000), (5, 32770), (32, 32768 + 64), (7, 9 * 15 - 1), (64, BENCH_P)]   # P not a multiple of 512
BUDGETS = [0, 1, 3, 5, 160, 192, 224, 255, 256, 257, 100000]


@pytest.mark.parametrize('B,P', SIZES, ids=lambda v: str(v))
def test_split_covers_the_frame_within_the_budget(vkn, B, P):
    split = vkn.ops.decode_px_per_wg
    dflt = _default_px(B, P)
    assert split(B, P, 0) == dflt and split(B, P) == dflt
    for budget in BUDGETS:
        px = split(B, P, budget)
        g2 = _g2(P, px)
        assert px > 0 and px % GRAN == 0, (budget, px)
        assert g2 * px >= P and (g2 - 1) * px < P, (budget, px)                  # covers P, and no workgroup is empty
        if budget == 0 or budget >= B * _g2(P, dflt):
            assert px == dflt, (budget, px, dflt)                               # today's split, exactly
            continue
        if budget >= B:
            assert B * g2 <= budget, (budget, px, g2)
        else:
            assert g2 == 1, (budget, px)                                        # unsatisfiable: one workgroup per frame
        # an even split: the smallest 512-px multiple that holds an equal share of the frame's pixels for budget // B workgroups
        share = -(-P // max(1, budget // B))
        assert px == -(-share // GRAN) * GRAN, (budget, px, share)


def test_split_at_the_benchmark_sizes_under_the_link_reservation(vkn):
    """192 of 256 CUs: 6 x 5632 px per frame at 32 frames, 11 x 3072 at 16, 22 x 1536 at 8 (the 512-px steps leave 176 workgroups there)"""
    split = vkn.ops.decode_px_per_wg
    assert [split(B, BENCH_P, 192) for B in (32, 16, 8)] == [5632, 3072, 1536]
    assert [B * _g2(BENCH_P, split(B, BENCH_P, 192)) for B in (32, 16, 8)] == [192, 176, 176]
    assert [split(B, BENCH_P, 0) for B in (32, 16, 8, 4, 2, 1)] == [4096, 2048, 1024, 512, 512, 512]


def test_split_rejects_bad_arguments(vkn):
    for args in ((0, 512, 0), (1, 0, 0), (1, 512, -1)):
        with pytest.raises(vkn._lib.VknError):
            vkn.ops.decode_px_per_wg(*args)
