"""The premises of tests/test_gpu_instmask.py, on the CPU: the partition cases of tests/instmask_ref.py leave NO pixel undecided, the noise
cases leave out at most NOISE_SHARE (under the cap of 1e-3), torch's own fp32 composition stays within F32_ERR of the float64 chain and
agrees with it on every decided pixel, and the numpy bit layout round-trips with zero tail bits."""
import numpy as np
import pytest
import torch

import instmask_ref as R
import pan_joint_ref


def test_floor_is_the_projects_own_number_and_the_geometries_are_the_listed_ones():
    assert R.FLOOR == pan_joint_ref.FLOOR == 1e-4 and R.UNDECIDED_CAP == 1e-3 and R.NOISE_SHARE <= 3.1e-4 < R.UNDECIDED_CAP
    assert len(R.GEOMS) == 11 and R.GEOMS['strip_64'][5][1] == 64 and R.GEOMS['strip_128'][5][1] == 128
    assert {g[2] for g in R.GEOMS.values()} == {1, 2, 4}
    assert all(g[4][0] <= g[3][0] and g[4][1] <= g[3][1] for g in R.GEOMS.values())        # img_shape is a crop of batch_input_shape
    assert all(lv[0] != lv[1] for g in [R.NONFINITE_GEOM] for lv in ((g[0] * g[2], g[3][0]), (g[1] * g[2], g[3][1]), (g[4][0], g[5][0]), (g[4][1], g[5][1])))


@pytest.mark.parametrize('name', list(R.GEOMS))
def test_partition_cases_have_no_undecided_pixel(name):
    c = R.partition(name)
    assert c['decided'].all() and c['undecided'] == 0.0
    assert c['mask'].any() and not c['mask'].all()
    assert all(m.any() for m in c['mask']) or name == 'one_row'


@pytest.mark.parametrize('name', list(R.GEOMS))
@pytest.mark.parametrize('thr', R.NOISE_THRS)
def test_noise_cases_stay_under_the_cap(name, thr):
    c = R.noise(name, thr)
    assert c['undecided'] <= R.NOISE_SHARE, c['undecided']
    assert 0.2 < c['mask'].mean() < 0.8


@pytest.mark.parametrize('kind,name,thr', R.CASES, ids=[f'{k}-{n}-{t}' for k, n, t in R.CASES])
def test_torchs_fp32_composition_agrees_on_the_decided_pixels(vkn, kind, name, thr):
    """... and so does the head's default path, `rescale_masks(...) > thr` (on the logits that it is handed: the x`up` ones)"""
    c = R.get(kind, name, thr)
    p32 = R.chain(c['logits'], c['meta'], c['up'], dtype=torch.float32)
    err = float(np.abs(p32.astype(np.float64) - c['p64']).max())
    print(f'{kind} {name} thr {thr}: torch fp32 against float64: {err:.2e}')
    # The 7e-6 is the noise inputs' figure (6.3e-6 at 'anisotropic').  A partition input is steeper: its probabilities cross from 0 to 1
    # within one x4 pixel, a slope of 1 per pixel, so the fp32 rounding of a source coordinate near 160 (half an ulp: 7.6e-6) shows
    # in full: 7.2e-6 at 'anisotropic', whatever the seed.  There the masks are compared instead, on every pixel (all are decided).
    assert p32.dtype == np.float32 and (err <= R.F32_ERR if kind == 'noise' else err <= R.FLOOR / 10)
    assert np.array_equal((p32 > np.float32(thr))[c['decided']], c['mask'][c['decided']])
    scaled = c['logits'] if c['up'] == 1 else torch.nn.functional.interpolate(c['logits'][None], scale_factor=c['up'], mode='bilinear', align_corners=False)[0]
    default = (vkn.KernelUpdateHead.rescale_masks(None, scaled, c['meta']) > thr).numpy()
    assert np.array_equal(default[c['decided']], c['mask'][c['decided']])
    torch_path = vkn.ops.rescale_masks_torch(c['logits'], c['meta'], c['up']).numpy()
    assert np.array_equal(torch_path, p32)


def test_rows_and_nonfinite_builders():
    c = R.rows_case(100)
    assert c['decided'].all() and c['mask'].shape == (100, 48, 80)
    n = R.nonfinite_case()
    nan = np.isnan(n['p64'])
    assert nan.any() and not n['mask'][nan].any() and n['decided'][nan].all() and n['undecided'] <= R.UNDECIDED_CAP
    assert np.isfinite(n['p64'][~nan]).all()


@pytest.mark.parametrize('W', [1, 63, 64, 65, 128, 130])
def test_pack_unpack_round_trip_and_zero_tail(vkn, W):
    rng = np.random.default_rng(W)
    m = rng.random((3, 7, W)) < 0.5
    m[0, 0, W - 1] = m[1, 6, 0] = True
    b = R.pack_bits(m)
    assert b.dtype == np.uint64 and b.shape == (3, R.strips_of(W), 7)
    got, tail = R.unpack_bits(b, W)
    assert np.array_equal(got, m) and not tail
    assert int(b[0, -1, 0]) >> ((W - 1) % 64) & 1 == 1 and int(b[1, 0, 6]) & 1 == 1       # bit c of a word is column 64 * strip + c
    if W % 64:
        assert int(b[:, -1, :].max()) < 1 << (W % 64)
    spoiled = b.copy()
    if W % 64:
        spoiled[2, -1, 3] |= np.uint64(1) << np.uint64(63)
        assert R.unpack_bits(spoiled, W)[1]
    # the package's torch pack (the torch path of ops.instance_mask_bits) writes the same words
    assert np.array_equal(vkn.ops.pack_mask_bits_torch(torch.from_numpy(m)).numpy().view(np.uint64), b)
