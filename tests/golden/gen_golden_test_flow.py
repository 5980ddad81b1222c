"""Writes tests/golden/test_flow.npz and test_flow.json by IMPORTING the unmodified reference's test_with_reports.py,
calculate_sensitivity_specificity.py and calculate_sensitivity_specificity_F1_AUC.py (nibabel stubbed by an in-memory loader; scipy, pandas,
scikit-learn and filelock are the real ones).

    det cases   (shape, spacing, th, erode) on uint8 / float32 volumes with solid blobs (>= 4^3, so erosion leaves voxels) plus speckle;
                expected = test_with_reports.detection on the stubbed file.  The shapes include every row of the GPU shape list of
                tests/test_gpu_test_flow.py; masks are stored bit-packed and probability volumes as float32, so the file stays at tens of KB although
                (20, 40, 70) is larger than 24^3.
    scorers     a ground-truth table and prediction tables of 36 cases (duplicated IDs, `.npz` suffixes, a `BDMAP ID` column, kidney with a single
                class, NaN maximum probabilities) -> the CSV text evaluate_predictions and evaluate_all write, stored as bytes, and prob_auc's values.

The generator asserts: every erode case has a non-zero result; at least half of the cases differ from their erode=False result; at least two
cases hit the `c > n_in - 1` quirk of ndimage.zoom with a count that differs from the clamped-index rule; no AUROC lies within 1e-6 of a rounding
boundary of the third decimal; tests/test_flow_ref.py equals the reference on every case.
Run from the repository root: python tests/golden/gen_golden_test_flow.py
"""
import importlib
import io
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402
import test_flow_ref as fr  # noqa: E402

VOLUMES = {}


class _Image:
    def __init__(self, data):
        self.data = data

    def get_fdata(self):
        return np.asarray(self.data).astype(np.float64)


def import_reference():
    nib = types.ModuleType('nibabel')
    nib.load = lambda key: _Image(VOLUMES[key])
    sys.modules['nibabel'] = nib
    sys.path.insert(0, gg.REF)
    return (importlib.import_module('test_with_reports'), importlib.import_module('calculate_sensitivity_specificity'),
            importlib.import_module('calculate_sensitivity_specificity_F1_AUC'))


# name, shape, spacing (per array axis), th, erode, dtype
DET_CASES = [
    ('identity', (9, 17, 33), (1, 1, 1), 0.5, True, 'u8'),
    ('identity_plain', (9, 17, 33), (1, 1, 1), 0.5, False, 'u8'),
    ('quirk_x', (6, 11, 16), (1.5, 1.5, 5.0), 0.5, True, 'u8'),                 # -> (9, 16, 80): half-to-even y, x index 79 beyond the input
    ('quirk_x_plain', (6, 11, 16), (1.5, 1.5, 5.0), 0.5, False, 'u8'),
    ('half', (20, 40, 70), (0.5, 0.5, 0.5), 0.5, True, 'u8'),                   # -> (10, 20, 35)
    ('nout1', (2, 9, 9), (0.6640625, 1, 1), 0.5, False, 'u8'),                  # -> one output plane
    ('quirk_y', (20, 26, 30), (0.7, 0.9, 0.55), 0.5, True, 'u8'),               # y: 26 -> 23, 22 * (25 / 22) > 25
    ('quirk_y_f32', (20, 26, 30), (0.7, 0.9, 0.55), 0.3, True, 'f32'),
    ('ct_like', (12, 20, 22), (2.5, 0.8, 0.8), 0.5, True, 'u8'),
    ('up_f32', (10, 12, 11), (1.5, 1.25, 2.0), 0.25, True, 'f32'),              # holds values exactly equal to th
    ('up_f32_plain', (10, 12, 11), (1.5, 1.25, 2.0), 0.25, False, 'f32'),
    ('levels_u8', (12, 14, 16), (1.3, 1.0, 0.8), 1.0, True, 'u8'),              # labels 0 / 1 / 2, th = 1: only 2 is set
    ('ties', (8, 8, 8), (2.5, 2.5, 2.5), 0.5, True, 'u8'),                      # 8 -> 20: coordinates with .5 fractions
    ('th_high_f32', (16, 16, 16), (1.0, 1.2, 0.9), 0.75, True, 'f32'),
]


def make_volume(shape, spacing, dtype, th, seed):
    r = np.random.default_rng(seed)
    m = np.zeros(shape, bool)
    for _ in range(3):                                                          # solid blobs, at least 4 voxels a side where the shape allows
        size = [min(n, int(np.ceil(int(r.integers(4, 8)) / min(1.0, f)))) for n, f in zip(shape, spacing)]        # >= 4 after the zoom
        lo = [int(r.integers(0, n - s + 1)) for n, s in zip(shape, size)]
        m[lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = True
    m[..., -5:] |= r.random(shape[:2] + (min(5, shape[2]),)) < 0.6              # the last x / y samples are busy, so the quirk planes matter
    m[:, -4:, :] |= r.random((shape[0], min(4, shape[1]), shape[2])) < 0.6
    m |= r.random(shape) < 0.04                                                 # speckle that erosion removes
    m &= ~(r.random(shape) < 0.03)                                              # pin holes
    if dtype == 'u8':
        v = m.astype(np.uint8)
        if th >= 1.0:
            v = v * 2 - (m & (r.random(shape) < 0.15)).astype(np.uint8)         # 2 inside, some 1s: `> 1` drops them
        return v
    v = np.where(m, th + 0.05 + 0.5 * r.random(shape), th * r.random(shape))
    v = (np.round(v * 64) / 64).astype(np.float32)                               # 1/64 steps: exact in float32, and the file compresses
    v[r.random(shape) < 0.05] = np.float32(th)                                  # exactly th: not set
    return v


def quirk_axes(shape, spacing):
    out_shape = fr.zoom_shape(shape, spacing)
    return [a for a, (n, o) in enumerate(zip(shape, out_shape)) if not fr.nearest_axis(n, o)[1].all()]


def scorer_tables(seed=7):
    r = np.random.default_rng(seed)
    n = 36
    ids = [f'BDMAP_{i:08d}' for i in range(1, n + 1)]
    liver = r.integers(0, 3, n)
    panc = (r.random(n) < 0.4).astype(int) * r.integers(1, 4, n)
    kidney = np.zeros(n, int)                                                   # a single class: N/A sensitivity, nan AUROC
    gt_ids = list(ids)
    gt_ids[3] += '.npz'
    gt_ids[4] = ' ' + gt_ids[4] + ' '
    gt_rows = [(gt_ids[i], liver[i], panc[i], kidney[i]) for i in range(n)]
    gt_rows.append((ids[5], 1 - min(1, liver[5]), panc[5], 0))                  # a duplicated ID with another label: the last one is kept
    gt = 'BDMAP ID,number of liver lesion instances,number of pancreatic lesion instances,number of kidney lesion instances\n'
    gt += ''.join(f'{a},{b},{c},{d}\n' for a, b, c, d in gt_rows)

    def volumes(lab, scale):
        v = np.where(lab > 0, r.gamma(2.0, scale, n), r.gamma(0.6, scale / 12, n))
        return np.round(v).astype(int)

    def prob(lab):
        p = np.clip(np.where(lab > 0, 0.55, 0.3) + 0.3 * r.standard_normal(n), 0.0, 1.0)
        p = np.round(p, 2)                                                      # ties between positives and negatives
        p[r.random(n) < 0.1] = np.nan
        return p

    cols = ['BDMAP_ID'] + [f'{o} tumor {k}' for o in ('kidney', 'liver', 'pancreatic') for k in ('maximum probability', 'volume predicted')]
    pl, pp, pk = prob(liver), prob(panc), prob(kidney)
    pred_ids = list(ids)
    pred_ids[7] += '.npz'
    preds = {}
    for t in range(1, 10):
        shrink = 1.0 - 0.08 * (t - 1)
        vl, vp, vk = volumes(liver, 900 * shrink), volumes(panc, 500 * shrink), volumes(kidney, 300 * shrink)
        lines = [','.join(cols)]
        for i in list(range(n)) + [9, 9]:                                      # duplicated rows
            f = lambda x: '' if np.isnan(x) else repr(float(x))
            lines.append(f'{pred_ids[i]},{f(pk[i])},{vk[i]},{f(pl[i])},{vl[i]},{f(pp[i])},{vp[i]}')
        preds[t / 10] = '\n'.join(lines) + '\n'
    return gt, preds


def main():
    T, S, F = import_reference()
    import pandas as pd
    from sklearn.metrics import roc_auc_score
    out, meta = {}, {'det': []}
    differs, quirks = 0, 0
    for k, (name, shape, spacing, th, erode, dt) in enumerate(DET_CASES):
        q = quirk_axes(shape, spacing)
        seed = 300 + k
        while True:                                                             # redrawn until the case shows what it is there for
            v = make_volume(shape, spacing, dt, th, seed)
            VOLUMES[name] = v
            exp = int(T.detection(name, None, spacing, th=th, erode=erode))
            plain = int(T.detection(name, None, spacing, th=th, erode=False))
            clamped = fr.detection_binary(v, spacing, th, erode, clamp=True)
            if (exp > 0 or not erode) and (clamped != exp or not q):
                break
            seed += 1000
        assert exp == fr.detection_binary(v, spacing, th, erode), name
        assert plain == fr.detection_binary(v, spacing, th, False), name
        assert (clamped != exp) == bool(q), name
        differs += exp != plain
        quirks += bool(q)
        if dt == 'u8' and v.max() <= 1:
            out[f'det_{name}_bits'] = np.packbits(v.ravel())
        else:
            out[f'det_{name}_x'] = v
        meta['det'].append({'name': name, 'shape': list(shape), 'spacing': list(spacing), 'th': th, 'erode': erode, 'dtype': dt,
                            'expected': exp, 'plain': plain, 'clamped': clamped, 'quirk_axes': q,
                            'out_shape': list(fr.zoom_shape(shape, spacing))})
        print(f'{name}: {shape} -> {fr.zoom_shape(shape, spacing)} th {th} erode {erode}: {exp} (plain {plain}, clamped {clamped}, quirk {q})')
    erode_cases = sum(1 for c in DET_CASES if c[4])
    assert len(DET_CASES) >= 12 and 2 * differs >= len(DET_CASES), (differs, len(DET_CASES))
    assert quirks >= 2 and erode_cases >= 8

    gt, preds = scorer_tables()
    with tempfile.TemporaryDirectory() as d:
        gp = os.path.join(d, 'gt.csv')
        open(gp, 'w').write(gt)
        for t, text in preds.items():
            open(os.path.join(d, f'tumor_detection_results_th{t}.csv'), 'w').write(text)
        pred_csv = os.path.join(d, 'tumor_detection_results_th0.5.csv')
        S.evaluate_predictions(gp, pred_csv, os.path.join(d, 'sens_spec.csv'))
        F.evaluate_all(gp, d)
        out['csv_gt'] = np.frombuffer(gt.encode(), np.uint8)
        out['csv_sens_spec'] = np.frombuffer(open(os.path.join(d, 'sens_spec.csv'), 'rb').read(), np.uint8)
        for t, text in preds.items():
            out[f'csv_pred_th{t}'] = np.frombuffer(text.encode(), np.uint8)
            out[f'csv_metrics_th{t}'] = np.frombuffer(open(os.path.join(d, f'metrics_th{t}.csv'), 'rb').read(), np.uint8)
        g = F.load_ground_truth(gp)
        p0 = pd.read_csv(io.StringIO(preds[0.1])).drop_duplicates(subset='BDMAP_ID')
        auc = F.prob_auc(g, p0)
        merged = pd.merge(g, p0, on='BDMAP_ID', how='inner')
        for organ in F.ORGANS:
            y, p = merged[f'gt_{organ}'], merged[f'{organ} tumor maximum probability']
            keep = ~(y.isna() | p.isna())
            if y[keep].nunique() < 2:
                assert np.isnan(auc[organ])
                continue
            raw = roc_auc_score(y[keep].astype(float), p[keep].astype(float))
            frac = raw * 1000 - np.floor(raw * 1000)
            assert abs(frac - 0.5) > 1e-3, f'{organ}: AUROC {raw} sits on a rounding boundary'
            assert (p[keep].to_numpy()[y[keep].to_numpy() == 1][:, None] == p[keep].to_numpy()[y[keep].to_numpy() == 0][None, :]).any(), 'no tie'
        meta['auc'] = {o: (None if np.isnan(a) else float(a)) for o, a in auc.items()}
        assert sum(v is None for v in meta['auc'].values()) == 1
    path = os.path.join(HERE, 'test_flow.npz')
    np.savez_compressed(path, **out)
    with open(os.path.join(HERE, 'test_flow.json'), 'w') as f:
        json.dump(meta, f, indent=1)
        f.write('\n')
    print(f'wrote {path}: {os.path.getsize(path)} bytes, {len(out)} arrays; auc {meta["auc"]}')


if __name__ == '__main__':
    main()
