"""Golden vectors for the validation metrics, produced on the CPU by the UNMODIFIED reference `metric/metrics.py` (scipy):

    RSUPER_REFERENCE=<checkout of the reference>/rsuper_train python tests/golden/gen_golden_surface_metrics.py

The reference's metric package is imported through a stub `metric` package whose __path__ is the reference directory (its metric/utils.py pulls
in nothing this needs), with np.Inf / np.NaN aliased in this process only (numpy 2 dropped them).

Per case `name` (keys sm_<name>_*): shape, gt / pred (bit-packed masks), spacing, table (the reference's 256 surfel areas for that spacing: a
recorded result, and the only way the tests obtain the table), n (surfel counts gt, pred), vox (|gt|, |pred|, |gt & pred|), d_gp / d_pg (the
two sorted distance arrays, strided by d_gp_step / d_pg_step with synth.subsample above 4096 entries), asum (both area sums), asd (the average
surface distance pair), hd (robust Hausdorff at PERCENTS), sdice (surface Dice at TOLERANCES), dice.  Cases whose arrays are sub-sampled also
carry probe_idx / probe_d: the reference-side distance (scipy's distance_transform_edt of the predicted borders, the call the reference makes)
at every probe_idx-th ground-truth border corner in C order, so the numpy restatement is checked there without a full brute force.

A drawn case is redrawn with the next seed when (a) a normalised cumulative area lies within 1e-9 of a tested percentile at the chosen index or
the one before while the neighbouring distance differs, or (b) a distance lies within 1e-5 (relative) of a tested tolerance: rounding on the
device then cannot pick another element or flip a surfel.  Fixed-geometry cases cannot be redrawn: where rule (a) hits one of them (eight equal
areas put the cumulative area exactly on 0.5 and 0.75), hd_alt holds the distance on the other side of the boundary (NaN elsewhere) and the
tests accept either of the two.
"""
import importlib
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import synth  # noqa: E402
import postprocess_ref as PR  # noqa: E402
import surface_metrics_ref as SR  # noqa: E402

PERCENTS = (50, 75, 95, 100)
TOLERANCES = (1.55, 3.3)
SUB = 4096


def import_reference():
    ref = os.environ.get('RSUPER_REFERENCE')
    if not ref or not os.path.isdir(os.path.join(ref, 'metric')):
        raise SystemExit('set RSUPER_REFERENCE to the reference checkout\'s rsuper_train directory')
    if not hasattr(np, 'Inf'):
        np.Inf, np.NaN = np.inf, np.nan
    pkg = types.ModuleType('metric')
    pkg.__path__ = [os.path.join(ref, 'metric')]
    sys.modules['metric'] = pkg
    return importlib.import_module('metric.metrics'), importlib.import_module('metric.lookup_tables')


def blobs(shape, seed, coarse=4, mix=0.8, level=0.25):
    """Two similar blobby masks: a coarse random grid zoomed to `shape` (the align-corners trilinear zoom of tests/postprocess_ref.py), the
    prediction from the same grid plus a second one."""
    r = np.random.default_rng(seed)
    cs = tuple(max(2, -(-n // coarse) + 1) for n in shape)
    f = tuple(n / c for n, c in zip(shape, cs))
    a, b = r.standard_normal(cs), r.standard_normal(cs)
    va, vb = PR.zoom(a, f), PR.zoom(b, f)
    assert va.shape == tuple(shape)
    return va > level, (va + mix * vb) > level


def two_ends(shape, axis):
    """A thin volume whose long axis is `axis`: ground truth at both ends of it, prediction at the low end only."""
    gt, pred = np.zeros(shape, bool), np.zeros(shape, bool)
    n = shape[axis]

    def sl(a0, a1, lo, hi):
        s = [slice(lo[0], hi[0]), slice(lo[1], hi[1])]
        s.insert(axis, slice(a0, a1))
        return tuple(s)
    gt[sl(2, 6, (0, 1), (3, 4))] = True
    gt[sl(n - 10, n - 3, (1, 1), (3, 3))] = True
    pred[sl(3, 9, (0, 0), (2, 3))] = True
    return gt, pred


def voxels(shape, a, b):
    gt, pred = np.zeros(shape, bool), np.zeros(shape, bool)
    gt[a] = True
    pred[b] = True
    return gt, pred


def full_vs_box():
    gt, pred = np.ones((5, 6, 7), bool), np.zeros((5, 6, 7), bool)
    pred[1:4, 1:5, 2:6] = True
    return gt, pred


def one_side(kind):
    def f(seed):
        g, p = blobs((8, 9, 10), seed)
        z = np.zeros_like(g)
        return {'pred_empty': (g, z), 'gt_empty': (z, p), 'both_empty': (z, z)}[kind]
    return f


# (name, spacing, drawn(seed) -> masks or None, fixed masks or None)
CASES = [
    ('iso_odd', (1.0, 1.0, 1.0), lambda s: blobs((9, 11, 13), s), None),
    ('ct_like', (2.5, 0.8, 0.8), lambda s: blobs((12, 20, 22), s), None),
    ('aniso', (1.5, 0.7, 0.9), lambda s: blobs((24, 31, 37), s), None),
    ('slab', (3.0, 1.0, 1.0), lambda s: blobs((1, 12, 14), s, coarse=3), None),
    ('voxels', (2.5, 0.8, 0.8), None, voxels((6, 10, 40), (1, 2, 3), (4, 7, 35))),
    ('identical', (1.5, 0.7, 0.9), lambda s: (blobs((10, 12, 14), s)[0],) * 2, None),
    ('full_vs_box', (1.0, 1.0, 1.0), None, full_vs_box()),
    ('pred_empty', (1.0, 1.0, 1.0), one_side('pred_empty'), None),
    ('gt_empty', (1.0, 1.0, 1.0), one_side('gt_empty'), None),
    ('both_empty', (1.0, 1.0, 1.0), one_side('both_empty'), None),
    ('wide', (3.0, 0.75, 0.75), lambda s: blobs((10, 70, 130), s, coarse=8), None),
    ('thin_w', (1.5, 0.7, 0.9), None, two_ends((3, 5, 1100), 2)),
    ('thin_d', (1.5, 0.7, 0.9), None, two_ends((1100, 3, 5), 0)),
    ('thin_h', (1.5, 0.7, 0.9), None, two_ends((3, 1100, 5), 1)),
    ('mid', (2.5, 0.8, 0.8), lambda s: blobs((96, 128, 160), s, coarse=16), None),
]


def percentile_margin(d, a, percent):
    """(chosen distance, the distance on the other side of the boundary when the cumulative area sits on the percentile, else None)."""
    if len(d) == 0:
        return np.inf, None
    cum = np.cumsum(a) / np.sum(a)
    p = percent / 100.0
    idx = min(int(np.searchsorted(cum, p)), len(d) - 1)
    if idx >= 1 and abs(cum[idx - 1] - p) < 1e-9 and d[idx - 1] != d[idx]:
        return d[idx], d[idx - 1]
    if idx + 1 < len(d) and abs(cum[idx] - p) < 1e-9 and d[idx + 1] != d[idx]:
        return d[idx], d[idx + 1]
    return d[idx], None


def near_tolerance(d):
    f = d[np.isfinite(d)]
    return any(np.any(np.abs(f - t) <= 1e-5 * t) for t in TOLERANCES)


def main():
    M, LT = import_reference()
    from scipy import ndimage
    out = {'percents': np.array(PERCENTS, np.float64), 'tolerances': np.array(TOLERANCES, np.float64)}
    names = []
    for ci, (name, spacing, drawn, fixed) in enumerate(CASES):
        seed = 100 * (ci + 1)
        while True:
            gt, pred = fixed if drawn is None else drawn(seed)
            gt, pred = np.ascontiguousarray(gt, dtype=bool), np.ascontiguousarray(pred, dtype=bool)
            sd = M.compute_surface_distances(gt, pred, spacing)
            dg, dp, ag, ap = (np.asarray(sd[k], np.float64) for k in ('distances_gt_to_pred', 'distances_pred_to_gt', 'surfel_areas_gt',
                                                                      'surfel_areas_pred'))
            amb = [[percentile_margin(dg, ag, p), percentile_margin(dp, ap, p)] for p in PERCENTS]
            bad = any(m[1] is not None for pair in amb for m in pair) or near_tolerance(dg) or near_tolerance(dp)
            degenerate = drawn is not None and name not in ('pred_empty', 'gt_empty', 'both_empty') and (not gt.any() or not pred.any())
            if drawn is None or not (bad or degenerate):
                break
            seed += 1
            if seed % 100 > 40:
                raise SystemExit(f'{name}: no admissible draw in 40 seeds')
        if drawn is None:
            assert not (near_tolerance(dg) or near_tolerance(dp)), f'{name}: a distance sits on a tested tolerance'
        with np.errstate(invalid='ignore', divide='ignore'):
            asd = M.compute_average_surface_distance(sd)
            hd = [M.compute_robust_hausdorff(sd, p) for p in PERCENTS]
            sdice = [M.compute_surface_dice_at_tolerance(sd, t) for t in TOLERANCES]
        # the other side of an exact boundary hit (fixed-geometry cases only): the Hausdorff value if a direction moved to its neighbour
        hd_alt = np.full(len(PERCENTS), np.nan)
        for k in range(len(PERCENTS)):
            sides = [[c] + ([] if o is None else [o]) for c, o in amb[k]]
            alts = {max(x, y) for x in sides[0] for y in sides[1]} - {hd[k]}
            assert len(alts) <= 1, (name, PERCENTS[k], alts)
            if alts:
                hd_alt[k] = alts.pop()
        pre = f'sm_{name}_'
        out[pre + 'shape'] = np.array(gt.shape, np.int64)
        out[pre + 'seed'] = np.array([seed], np.int64)
        out[pre + 'gt'], out[pre + 'pred'] = np.packbits(gt.ravel()), np.packbits(pred.ravel())
        out[pre + 'spacing'] = np.array(spacing, np.float64)
        out[pre + 'table'] = np.asarray(LT.create_table_neighbour_code_to_surface_area(spacing), np.float64)
        out[pre + 'n'] = np.array([len(dg), len(dp)], np.int64)
        out[pre + 'vox'] = np.array([gt.sum(), pred.sum(), (gt & pred).sum()], np.int64)
        out[pre + 'd_gp'], step_g = synth.subsample(dg, SUB)
        out[pre + 'd_pg'], step_p = synth.subsample(dp, SUB)
        out[pre + 'd_gp_step'], out[pre + 'd_pg_step'] = np.array([step_g], np.int64), np.array([step_p], np.int64)
        out[pre + 'asum'] = np.array([ag.sum(), ap.sum()], np.float64)
        out[pre + 'asd'] = np.array(asd, np.float64)
        out[pre + 'hd'], out[pre + 'hd_alt'] = np.array(hd, np.float64), hd_alt
        out[pre + 'sdice'] = np.array(sdice, np.float64)
        out[pre + 'dice'] = np.array([M.compute_dice_coefficient(gt, pred)], np.float64)
        if step_g > 1:
            cg, cp = SR.neighbour_codes(gt), SR.neighbour_codes(pred)
            dist = ndimage.distance_transform_edt(~SR.borders(cp), sampling=spacing)
            every = max(1, len(dg) // 384)
            out[pre + 'probe_idx'] = np.array([every], np.int64)
            out[pre + 'probe_d'] = dist[SR.borders(cg)][::every]
        names.append(name)
        print(f'{name:12s} seed {seed} shape {gt.shape} surfels {len(dg)}/{len(dp)} asd {asd} hd {hd} alt {hd_alt} sdice {sdice}')
    out['names'] = np.array(names)
    path = os.path.join(HERE, 'surface_metrics.npz')
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), 'bytes')


if __name__ == '__main__':
    main()
