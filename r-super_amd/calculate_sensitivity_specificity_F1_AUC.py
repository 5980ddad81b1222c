"""python -m rsuper_amd.calculate_sensitivity_specificity_F1_AUC: one metrics_thX.csv per confidence threshold X (0.1 ... 0.9) with sensitivity,
specificity, F1 and the maximum-probability AUROC per organ -- a restatement of rsuper_train/calculate_sensitivity_specificity_F1_AUC.py whose CSV
text is byte-identical.  Host code; the AUROC is the Mann-Whitney count (ties at one half), so scikit-learn is not needed."""
import argparse
import glob
import os
import re

import numpy as np
import pandas as pd

from .calculate_sensitivity_specificity import ORGANS, THRESHOLDS_VOL, format_metric as pct_string

THRESHOLDS_CONF = [i / 10 for i in range(1, 10)]


def auroc(y_true, y_score):
    """Area under the ROC curve = P(score of a positive > score of a negative) + P(equal) / 2, from integer counts: (2 * greater + ties) /
    (2 * positives * negatives).  One division; nan without both classes."""
    y_true = np.asarray(y_true).astype(bool)
    s = np.asarray(y_score, dtype=np.float64)
    pos, neg = np.sort(s[y_true]), np.sort(s[~y_true])
    if pos.size == 0 or neg.size == 0:
        return float('nan')
    below = np.searchsorted(neg, pos, side='left')               # negatives strictly below each positive
    upto = np.searchsorted(neg, pos, side='right')               # negatives below or equal
    numer = 2 * int(below.sum()) + int((upto - below).sum())
    return numer / (2 * int(pos.size) * int(neg.size))


def load_ground_truth(path):
    """BDMAP_ID and one binary label per organ: from FELIX IDs ('PDAC'), from a Diagnosis text, or from the numeric lesion counts (>= 1)."""
    gt = pd.read_csv(path)
    if 'BDMAP ID' in gt.columns:
        gt = gt.rename(columns={'BDMAP ID': 'BDMAP_ID'})
    if 'FELIX ID' in gt.columns:
        labels = {'liver': 0, 'pancreatic': gt['FELIX ID'].str.contains('PDAC').astype(int), 'kidney': 0}
    elif 'Diagnosis' in gt.columns:
        labels = {'liver': 0, 'pancreatic': gt['Diagnosis'].str.contains(r'PDAC|lesion|PNET|cyst', regex=True).astype(int), 'kidney': 0}
    else:
        labels = {organ: (gt[f'number of {organ} lesion instances'] >= 1).astype(int) for organ in ORGANS}
    for organ in ORGANS:
        gt[f'gt_{organ}'] = labels[organ]
    return gt[['BDMAP_ID'] + [f'gt_{organ}' for organ in ORGANS]]


def prob_auc(gt, preds_df0):
    """{organ: AUROC of the maximum probability, rounded to 3 decimals, or nan}; rows with a NaN label or probability are dropped pairwise."""
    merged = pd.merge(gt, preds_df0[['BDMAP_ID'] + [f'{organ} tumor maximum probability' for organ in ORGANS]], on='BDMAP_ID', how='inner')
    out = {}
    for organ in ORGANS:
        y = merged[f'gt_{organ}'].to_numpy(dtype=np.float64)
        p = merged[f'{organ} tumor maximum probability'].to_numpy(dtype=np.float64)
        keep = ~(np.isnan(y) | np.isnan(p))
        y, p = y[keep], p[keep]
        if np.unique(y).size < 2:
            out[organ] = np.nan
            continue
        out[organ] = round(auroc(y == y.max(), p), 3)
    return out


def _f1(tp, fp, fn):
    d = 2 * tp + fp + fn
    return (2 * tp) / d if d else np.nan


def evaluate_all(ground_truth_csv, preds_dir):
    gt = load_ground_truth(ground_truth_csv)
    paths = sorted(glob.glob(os.path.join(preds_dir, '*results_th*.csv')))
    preds_all = {float(re.search(r'_th([0-9.]+)\.csv$', p).group(1)): pd.read_csv(p).drop_duplicates(subset='BDMAP_ID') for p in paths}
    if set(preds_all) != set(THRESHOLDS_CONF):
        raise RuntimeError('Missing some *_thX.csv files')
    auc = prob_auc(gt, preds_all[THRESHOLDS_CONF[0]])
    for conf, pred in preds_all.items():
        df = pd.merge(gt, pred, on='BDMAP_ID', how='inner')
        rows = []
        for vthr in THRESHOLDS_VOL:
            row = {'threshold': vthr}
            for organ in ORGANS:
                g = df[f'gt_{organ}'].values.astype(bool)
                p = df[f'{organ} tumor volume predicted'].values >= vthr
                tp, fn = np.logical_and(g, p).sum(), np.logical_and(g, ~p).sum()
                fp, tn = np.logical_and(~g, p).sum(), np.logical_and(~g, ~p).sum()
                f1 = _f1(tp, fp, fn)
                row[f'{organ}_sens'] = pct_string(tp, tp + fn)
                row[f'{organ}_spec'] = pct_string(tn, tn + fp)
                row[f'{organ}_f1'] = '' if np.isnan(f1) else round(f1, 3)
                row[f'{organ}_auc_prob'] = auc[organ]
            rows.append(row)
        out_csv = os.path.join(preds_dir, f'metrics_th{conf}.csv')
        pd.DataFrame(rows).to_csv(out_csv, index=False)
        print('saved', out_csv)


def get_parser():
    p = argparse.ArgumentParser(prog='rsuper_amd.calculate_sensitivity_specificity_F1_AUC')
    p.add_argument('--ground_truth_csv', required=True, help='CSV with ground-truth lesion counts / labels')
    p.add_argument('--preds_dir', required=True, help='folder with *_th0.1.csv ... *_th0.9.csv')
    return p


def main(argv=None):
    a = get_parser().parse_args(argv)
    evaluate_all(a.ground_truth_csv, a.preds_dir)


if __name__ == '__main__':
    main()
