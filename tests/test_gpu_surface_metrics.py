"""GPU checks of the validation metrics (metric/, training/validation.py, csrc/surfdist.hip) against the reference-generated fixture
tests/golden/surface_metrics.npz and the numpy restatement tests/surface_metrics_ref.py.

Bounds.  Surfel counts, voxel counts and Dice are exact.  Area sums and surface Dice: rtol 1e-9 (same table, float64 sums in another order).
Distances, both average surface distances and every percentile: rtol 1e-12 with zero exactly zero -- the distance transform is kept in
float64, where a sum of three squares plus a square root is a few units of 1e-16 and a near-tie that picks the other feature moves the
distance by no more than that; sorting preserves element-wise closeness.  Sorted area arrays are not compared element-wise (ties in distance
may be ordered differently); the percentiles cover them.
"""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import postprocess_ref as PR  # noqa: E402
import surface_metrics_ref as SR  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'surface_metrics.npz'))
NAMES = [str(n) for n in G['names']]
RTOL_D, RTOL_A = 1e-12, 1e-9


def _case(name):
    pre = f'sm_{name}_'
    shape = tuple(int(v) for v in G[pre + 'shape'])
    n = int(np.prod(shape))
    gt = np.unpackbits(G[pre + 'gt'])[:n].reshape(shape).astype(bool)
    pred = np.unpackbits(G[pre + 'pred'])[:n].reshape(shape).astype(bool)
    return gt, pred, [float(s) for s in G[pre + 'spacing']], G[pre + 'table'], pre


def _close(actual, expected, rtol, what):
    """rtol with zero exactly zero; inf and NaN must agree in place."""
    np.testing.assert_allclose(np.asarray(actual, np.float64), np.asarray(expected, np.float64), rtol=rtol, atol=0.0, equal_nan=True, err_msg=what)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.mark.parametrize('name', NAMES)
def test_fixture_case(name):
    from rsuper_amd.metric import metrics as M
    gt, pred, spacing, table, pre = _case(name)
    res, counts = M.surface_distances_stack(_dev(gt)[None], _dev(pred)[None], spacing, table)
    sd, counts = res[0], counts.cpu().numpy()[0]
    dg, dp, ag, ap = (sd[k].cpu().numpy() for k in M.KEYS)
    print(name, 'surfels', len(dg), len(dp), 'counts', counts.tolist())
    assert [len(dg), len(dp)] == G[pre + 'n'].tolist() and counts[3:].tolist() == G[pre + 'n'].tolist()
    assert counts[:3].tolist() == G[pre + 'vox'].tolist()
    assert all(sd[k].dtype == torch.float64 and sd[k].is_cuda for k in M.KEYS)
    dice = M.compute_dice_coefficient(_dev(gt), _dev(pred))
    exp_dice = float(G[pre + 'dice'][0])
    assert (np.isnan(dice) and np.isnan(exp_dice)) or dice == exp_dice
    _close([ag.sum(), ap.sum()], G[pre + 'asum'], RTOL_A, 'area sums')
    for d, key in ((dg, 'd_gp'), (dp, 'd_pg')):
        assert np.all(np.diff(d[np.isfinite(d)]) >= 0)
        sub = d[::int(G[pre + key + '_step'][0])][:len(G[pre + key])]
        fin = np.isfinite(sub)
        print(name, key, 'max rel err', float(np.max(np.abs(sub[fin] - G[pre + key][fin]) / np.maximum(G[pre + key][fin], 1e-300), initial=0.0)))
        _close(sub, G[pre + key], RTOL_D, key)
    _close(M.compute_average_surface_distance(sd), G[pre + 'asd'], RTOL_D, 'average surface distance')
    for k, pc in enumerate(G['percents']):
        hd = M.compute_robust_hausdorff(sd, float(pc))
        exp, alt = float(G[pre + 'hd'][k]), float(G[pre + 'hd_alt'][k])
        print(name, 'hd', pc, hd, exp, alt)
        assert np.isnan(alt) or name == 'voxels'        # only the fixed single-voxel geometry puts a cumulative area exactly on a percentile
        if name == 'voxels' and not np.isnan(alt) and abs(hd - exp) > RTOL_D * exp:
            exp = alt
        _close(hd, exp, RTOL_D, f'robust hausdorff {pc}')
    for k, tol in enumerate(G['tolerances']):
        _close(M.compute_surface_dice_at_tolerance(sd, float(tol)), G[pre + 'sdice'][k], RTOL_A, f'surface dice {tol}')
        og, op = M.compute_surface_overlap_at_tolerance(sd, float(tol))
        assert np.isnan(og) or 0.0 <= og <= 1.0
    if name == 'identical':
        assert not dg.any() and not dp.any() and M.compute_robust_hausdorff(sd, 95) == 0.0
        assert M.compute_surface_dice_at_tolerance(sd, 0.0) == 1.0
    if name == 'full_vs_box':
        assert len(dg) == 216
        _close(M.compute_robust_hausdorff(sd, 95), np.sqrt(5.0), RTOL_D, 'the 95th percentile of the full volume against the box')
    if name == 'both_empty':
        assert all(sd[k].numel() == 0 for k in M.KEYS) and M.compute_robust_hausdorff(sd, 95) == np.inf


def test_stack_equals_single_calls_and_repeats_bit_for_bit():
    from rsuper_amd.metric import metrics as M
    gt, pred, spacing, table, _ = _case('ct_like')
    z = np.zeros_like(gt)
    gts, preds = _dev(np.stack([gt, pred, gt, z])), _dev(np.stack([pred, gt, gt, pred]))
    res, counts = M.surface_distances_stack(gts, preds, spacing, table)
    again, counts2 = M.surface_distances_stack(gts, preds, spacing, table)
    assert torch.equal(counts, counts2)
    for p in range(4):
        one, c1 = M.surface_distances_stack(gts[p:p + 1], preds[p:p + 1], spacing, table)
        assert torch.equal(c1[0], counts[p])
        for k in M.KEYS:
            assert torch.equal(res[p][k].view(torch.int64), one[0][k].view(torch.int64)), (p, k)
            assert torch.equal(res[p][k].view(torch.int64), again[p][k].view(torch.int64)), (p, k)
        assert M.compute_robust_hausdorff(res[p], 95) == M.compute_robust_hausdorff(again[p], 95)
        a, b = M.compute_average_surface_distance(res[p]), M.compute_average_surface_distance(again[p])
        assert np.array_equal(np.array(a).view(np.int64), np.array(b).view(np.int64))


def test_edt3_sub_box_matches_brute_force():
    """The transform alone, on a box that starts inside the volume: features outside the box do not count."""
    from rsuper_amd.metric import metrics as M
    r = np.random.default_rng(5)
    mask = r.random((8, 40, 70)) > 0.99
    codes = SR.neighbour_codes(mask)
    box = (1, 2, 1, 7, 37, 66)
    sub = codes[1:8, 2:39, 1:67]
    spacing = (2.5, 0.8, 0.7)
    out = M.edt3(_dev(codes), box, spacing).cpu().numpy()
    grid = np.argwhere(np.ones(sub.shape, bool))
    ref = SR.nearest_distances(grid, np.argwhere(SR.borders(sub)), spacing).reshape(sub.shape) ** 2
    _close(out, ref, RTOL_D, 'squared distances')
    empty = M.edt3(_dev(np.zeros((4, 5, 6), np.uint8)), (0, 0, 0, 4, 5, 6), spacing)
    assert bool(torch.isinf(empty).all())


def _labels(shape, seed, C):
    r = np.random.default_rng(seed)
    cs = tuple(-(-n // 4) + 1 for n in shape)
    f = tuple(n / c for n, c in zip(shape, cs))
    fields = np.stack([PR.zoom(r.standard_normal(cs), f) for _ in range(C)])
    return np.argmax(fields, 0)


def _unambiguous(sd, percent):
    for d, a in ((sd['distances_gt_to_pred'], sd['surfel_areas_gt']), (sd['distances_pred_to_gt'], sd['surfel_areas_pred'])):
        if len(d) == 0 or not np.isfinite(d).all():
            continue
        cum = np.cumsum(a) / np.sum(a)
        idx = min(int(np.searchsorted(cum, percent / 100.0)), len(d) - 1)
        if abs(cum[idx] - percent / 100.0) < 1e-9 or (idx and abs(cum[idx - 1] - percent / 100.0) < 1e-9):
            return False
    return True


def test_calculate_distance_and_dice_split_match_the_restatement():
    """A drawn 5-class case; the draw is repeated with the next seed while a cumulative area sits within 1e-9 of the percentile."""
    from rsuper_amd.metric import calculate_distance, calculate_dice, calculate_dice_split
    C, shape = 5, (10, 14, 16)
    spacing, table = [float(s) for s in G['sm_ct_like_spacing']], G['sm_ct_like_table']
    seed = 40
    while True:
        true, pred = _labels(shape, seed, C), _labels(shape, seed, C)
        flip = np.random.default_rng(seed + 1000).random(shape) < 0.15
        pred = np.where(flip, _labels(shape, seed + 2000, C), pred)
        refs = [SR.surface_distances(true == c, pred == c, spacing, table) for c in range(1, C)]
        if all(_unambiguous(sd, 95) for sd in refs):
            break
        seed += 1
    hot_t, hot_p = _dev(np.stack([true == c for c in range(C)])), _dev(np.stack([pred == c for c in range(C)]))
    ASD, HD = calculate_distance(hot_p, hot_t, torch.tensor(spacing, dtype=torch.float64), C, area_table=table)
    exp_asd = [sum(SR.average_surface_distance(sd)) / 2 for sd in refs]
    exp_hd = [SR.robust_hausdorff(sd, 95) for sd in refs]
    print('ASD', ASD, exp_asd, 'HD', HD, exp_hd)
    _close(ASD, exp_asd, RTOL_D, 'ASD')
    _close(HD, exp_hd, RTOL_D, 'HD')
    ASD2, HD2 = calculate_distance(hot_p, hot_t, spacing, C, channels=[3, 1], area_table=table)
    assert ASD2.tolist() == [ASD[2], ASD[0]] and HD2.tolist() == [HD[2], HD[0]]
    tv, pv = _dev(true.reshape(-1, 1)), _dev(pred.reshape(-1, 1))
    for got, exp in ((calculate_dice(pv, tv, C), SR.label_dice(pred, true, C)),
                     (calculate_dice_split(pv, tv, C, block_size=500), SR.label_dice(pred, true, C, block_size=500))):
        assert all(g.dtype == torch.float32 for g in got)
        assert np.array_equal(got[1].cpu().numpy(), exp[1]) and np.array_equal(got[2].cpu().numpy(), exp[2])
        np.testing.assert_allclose(got[0].cpu().numpy(), exp[0], rtol=1e-6)      # one float32 division


def test_validation_on_a_synthetic_loader():
    from oracle import unet_oracle as uo
    from rsuper_amd.model.dim3.unet import UNet
    from rsuper_amd.training.validation import validation
    classes = synth.TINY_CLASSES
    C = len(classes)
    net = UNet(1, 8, num_classes=C, block='BasicBlock', norm='in', compute_dtype='f32')
    sd = synth.fill_state_dict(uo.unet_param_shapes(1, 8, C), 3)
    net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    bias = [k for k, v in net.state_dict().items() if v.shape == (C,)][-1]
    with torch.no_grad():
        net.state_dict()[bias][C - 1] = -60.0          # the last channel is predicted empty
    net = net.to(DEV)
    shape = (32, 32, 32)
    loader = []
    for seed in (1, 2):
        gt = np.stack([PR.zoom(np.random.default_rng(10 * seed + c).standard_normal((5, 5, 5)), (6.4, 6.4, 6.4)) > 0.3 for c in range(C)])
        assert gt.reshape(C, -1).any(1).all()
        loader.append((torch.from_numpy(synth.volume(shape, seed)), torch.from_numpy(gt[None]), torch.tensor([[2.5, 0.8, 0.8]], dtype=torch.float64)))
    args = argparse.Namespace(classes=C, dimension='3d', sliding_window=True, window_size=[32, 32, 32], surface_area_table=G['sm_ct_like_table'])
    dice, ASD, HD = validation(net, loader, args)
    print('dice', dice, 'ASD', ASD, 'HD', HD)
    for v in (dice, ASD, HD):
        assert v.shape == (C,) and np.isfinite(v).all()
    assert ASD[C - 1] == 500.0 and HD[C - 1] == 500.0 and dice[C - 1] == 0.0
    assert (ASD >= 0).all() and (ASD <= 500).all() and (dice >= 0).all() and (dice <= 1).all()


def test_refusals():
    """Ill-typed and undersized inputs are refused with an error before any launch; nothing is provoked on the device."""
    from rsuper_amd.hip import lib
    from rsuper_amd.metric import metrics as M
    table = G['sm_iso_odd_table']
    m = torch.zeros((4, 5, 6), device=DEV, dtype=torch.uint8)
    with pytest.raises(lib.RSuperHipError):
        M.compute_surface_distances(m.float(), m, (1, 1, 1), table)
    with pytest.raises(lib.RSuperHipError):
        M.compute_surface_distances(m[0], m[0], (1, 1), table)                    # the 2-D contour case
    with pytest.raises(lib.RSuperHipError):
        M.compute_surface_distances(m.cpu(), m.cpu(), (1, 1, 1), table)
    with pytest.raises(lib.RSuperHipError):
        M.compute_surface_distances(m, m, (1, 1, 1))                              # no table anywhere
    codes = torch.zeros((5, 6, 7), device=DEV, dtype=torch.uint8)
    need = lib.lib().rsuper_edt3_workspace_bytes(5, 6, 7)
    assert need > 0 and lib.lib().rsuper_edt3_workspace_bytes(5, 6, 4097) == 0
    with pytest.raises(lib.RSuperHipError):
        M.edt3(codes, (0, 0, 0, 5, 6, 7), (1, 1, 1), torch.empty((need - 1,), device=DEV, dtype=torch.uint8))
    with pytest.raises(lib.RSuperHipError):
        M.edt3(codes, (0, 0, 1, 5, 6, 7), (1, 1, 1))                              # the box leaves the volume
    with pytest.raises(lib.RSuperHipError):
        M.edt3(codes.float(), (0, 0, 0, 5, 6, 7), (1, 1, 1))
    with pytest.raises(lib.RSuperHipError):
        M.edt3(codes, (0, 0, 0, 5, 6, 7), (1, 0, 1))
