"""CPU checks of the validation metrics: the numpy restatement (tests/surface_metrics_ref.py) reproduces the reference-generated fixture
tests/golden/surface_metrics.npz, the C header declares the new entry points, and the surfel area table is resolved in the documented order."""
import os
import re
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import surface_metrics_ref as SR  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'surface_metrics.npz'))
NAMES = [str(n) for n in G['names']]


def _case(name):
    pre = f'sm_{name}_'
    shape = tuple(int(v) for v in G[pre + 'shape'])
    n = int(np.prod(shape))
    gt = np.unpackbits(G[pre + 'gt'])[:n].reshape(shape).astype(bool)
    pred = np.unpackbits(G[pre + 'pred'])[:n].reshape(shape).astype(bool)
    return gt, pred, [float(s) for s in G[pre + 'spacing']], G[pre + 'table'], pre


def _close(actual, expected, rtol, what):
    np.testing.assert_allclose(np.asarray(actual, np.float64), np.asarray(expected, np.float64), rtol=rtol, atol=0.0, equal_nan=True, err_msg=what)


def test_fixture_has_the_cases_the_gpu_test_needs():
    assert set(NAMES) >= {'iso_odd', 'ct_like', 'aniso', 'slab', 'voxels', 'identical', 'full_vs_box', 'pred_empty', 'gt_empty', 'both_empty',
                          'wide', 'thin_w', 'thin_d', 'thin_h', 'mid'}
    assert tuple(G['sm_mid_shape']) == (96, 128, 160) and G['sm_mid_spacing'].tolist() == [2.5, 0.8, 0.8]
    assert tuple(G['sm_thin_w_shape']) == (3, 5, 1100) and tuple(G['sm_thin_d_shape']) == (1100, 3, 5) and tuple(G['sm_thin_h_shape']) == (3, 1100, 5)
    assert G['percents'].tolist() == [50, 75, 95, 100]
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'surface_metrics.npz')) < 600 * 1024
    assert G['sm_full_vs_box_n'].tolist()[0] == 216 and G['sm_full_vs_box_hd'][2] == np.sqrt(5.0)


@pytest.mark.parametrize('name', [n for n in NAMES if int(G[f'sm_{n}_d_gp_step'][0]) == 1])
def test_restatement_reproduces_the_fixture(name):
    gt, pred, spacing, table, pre = _case(name)
    sd = SR.surface_distances(gt, pred, spacing, table)
    dg, dp, ag, ap = (sd[k] for k in ('distances_gt_to_pred', 'distances_pred_to_gt', 'surfel_areas_gt', 'surfel_areas_pred'))
    assert [len(dg), len(dp)] == G[pre + 'n'].tolist()
    assert [int(gt.sum()), int(pred.sum()), int((gt & pred).sum())] == G[pre + 'vox'].tolist()
    _close(SR.dice(gt, pred), G[pre + 'dice'][0], 0.0, 'dice')
    _close([ag.sum(), ap.sum()], G[pre + 'asum'], 1e-12, 'area sums')
    _close(dg, G[pre + 'd_gp'], 1e-12, 'gt -> pred')
    _close(dp, G[pre + 'd_pg'], 1e-12, 'pred -> gt')
    _close(SR.average_surface_distance(sd), G[pre + 'asd'], 1e-12, 'average surface distance')
    for k, pc in enumerate(G['percents']):
        hd, exp, alt = SR.robust_hausdorff(sd, float(pc)), float(G[pre + 'hd'][k]), float(G[pre + 'hd_alt'][k])
        if not np.isnan(alt) and abs(hd - exp) > 1e-12 * exp:
            exp = alt
        _close(hd, exp, 1e-12, f'robust hausdorff {pc}')
    for k, tol in enumerate(G['tolerances']):
        _close(SR.surface_dice(sd, float(tol)), G[pre + 'sdice'][k], 1e-12, f'surface dice {tol}')


@pytest.mark.parametrize('name', [n for n in NAMES if int(G[f'sm_{n}_d_gp_step'][0]) > 1])
def test_restatement_on_the_sub_sampled_cases(name):
    """The larger cases: codes, counts, area sums and Dice in full; distances at the recorded probe corners (a full brute force over 10^5
    surfels a side is minutes of numpy)."""
    gt, pred, spacing, table, pre = _case(name)
    cg, cp = SR.neighbour_codes(gt), SR.neighbour_codes(pred)
    bg, bp = SR.borders(cg), SR.borders(cp)
    assert [int(bg.sum()), int(bp.sum())] == G[pre + 'n'].tolist()
    assert [int(gt.sum()), int(pred.sum()), int((gt & pred).sum())] == G[pre + 'vox'].tolist()
    _close(SR.dice(gt, pred), G[pre + 'dice'][0], 0.0, 'dice')
    _close([table[cg[bg]].sum(), table[cp[bp]].sum()], G[pre + 'asum'], 1e-12, 'area sums')
    every = int(G[pre + 'probe_idx'][0])
    d = SR.nearest_distances(np.argwhere(bg)[::every], np.argwhere(bp), spacing)
    _close(d, G[pre + 'probe_d'], 1e-12, 'probe distances')


def test_header_declares_the_entry_points():
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    declared = set(re.findall(r'\b(rsuper_[a-z0-9_]+)\s*\(', hdr))
    assert {'rsuper_surface_codes', 'rsuper_edt3', 'rsuper_edt3_workspace_bytes', 'rsuper_surfel_gather'} <= declared
    from rsuper_amd.hip import lib
    assert {'rsuper_surface_codes', 'rsuper_edt3', 'rsuper_edt3_workspace_bytes', 'rsuper_surfel_gather'} <= set(lib.exported_symbols())


def test_workspace_query_on_the_host():
    from rsuper_amd.hip import lib
    L = lib.lib()
    assert L.rsuper_edt3_workspace_bytes(161, 257, 257) >= 161 * 257 * 257 * 20
    assert L.rsuper_edt3_workspace_bytes(4, 5, 2049) > 0                  # lines of 2048 corners and more are supported
    assert L.rsuper_edt3_workspace_bytes(0, 5, 5) == 0 and L.rsuper_edt3_workspace_bytes(5, 5, 4097) == 0


def test_area_table_resolution_order():
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.metric import lookup_tables as LT
    assert LT.ENCODE_NEIGHBOURHOOD_3D_KERNEL.ravel().tolist() == [128, 64, 32, 16, 8, 4, 2, 1]
    given, registered, checkout = np.arange(256.0), np.arange(256.0) + 1, np.arange(256.0) + 2
    saved = {k: sys.modules.pop(k) for k in list(sys.modules) if k == 'metric' or k.startswith('metric.')}
    old = LT.set_surface_area_table_fn(None)
    try:
        with pytest.raises(RSuperHipError, match='set_surface_area_table_fn'):          # 4. nothing available
            LT.resolve_surface_area_table((1, 1, 1))
        import types
        pkg, mod = types.ModuleType('metric'), types.ModuleType('metric.lookup_tables')
        pkg.__path__ = []
        mod.create_table_neighbour_code_to_surface_area = lambda spacing: checkout * spacing[0]
        sys.modules['metric'], sys.modules['metric.lookup_tables'] = pkg, mod
        assert np.array_equal(LT.resolve_surface_area_table((2, 1, 1)), checkout * 2)     # 3. the user's checkout
        LT.set_surface_area_table_fn(lambda spacing: registered * spacing[1])
        assert np.array_equal(LT.resolve_surface_area_table((2, 3, 1)), registered * 3)   # 2. the registered function
        assert np.array_equal(LT.resolve_surface_area_table((2, 3, 1), given), given)      # 1. the argument
        with pytest.raises(RSuperHipError):
            LT.resolve_surface_area_table((1, 1, 1), np.zeros(255))
    finally:
        LT.set_surface_area_table_fn(old)
        for k in ('metric', 'metric.lookup_tables'):
            sys.modules.pop(k, None)
        sys.modules.update(saved)


def test_metrics_need_the_device():
    import torch
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.metric import compute_surface_distances, compute_dice_coefficient
    m = torch.zeros((3, 4, 5), dtype=torch.bool)
    with pytest.raises(RSuperHipError):
        compute_surface_distances(m, m, (1, 1, 1), np.zeros(256))
    with pytest.raises(RSuperHipError):
        compute_dice_coefficient(m, m)
    with pytest.raises(RSuperHipError):
        compute_surface_distances(m[0], m[0], (1, 1), np.zeros(256))
