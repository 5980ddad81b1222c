"""python -m rsuper_amd.calculate_sensitivity_specificity: per-organ sensitivity, specificity and F1 of predicted tumour volumes against report
labels at 306 volume thresholds -- a restatement of rsuper_train/calculate_sensitivity_specificity.py whose CSV text is byte-identical.  Host code."""
import argparse
import csv

import numpy as np
import pandas as pd

ORGANS = ('liver', 'pancreatic', 'kidney')
# volume thresholds (mm^3): 10 .. 90, 100 .. 990, 100 .. 9900, 1000 .. 99000 (the repeated 100 .. 900 and 1000 .. 9000 rows are the reference's)
THRESHOLDS_VOL = ([i * 10 for i in range(1, 10)] + [i * 10 for i in range(10, 100)] + [i * 100 for i in range(1, 100)]
                  + [i * 1000 for i in range(1, 100)])


def normalize_id(val):
    """str, stripped, without one trailing '.npz'."""
    s = str(val).strip()
    return s[:-4] if s.endswith('.npz') else s


def format_metric(numer, denom):
    return 'N/A (0/0)' if denom == 0 else f'{100.0 * numer / denom:.1f}% ({numer}/{denom})'


def format_f1(tp, fp, fn):
    denom = 2 * tp + fp + fn
    if denom == 0:
        return 'N/A (TP=0, FP=0, FN=0)'
    return f'{100.0 * (2 * tp) / denom:.1f}% (TP={tp}, FP={fp}, FN={fn})'


def merged_tables(ground_truth_csv, predictions_csv):
    """Ground truth (binary label per organ: #instances >= 1) and predicted volumes, IDs normalised, the last of duplicated IDs kept, inner-joined."""
    gt = pd.read_csv(ground_truth_csv)
    if 'BDMAP ID' in gt.columns:
        gt = gt.rename(columns={'BDMAP ID': 'BDMAP_ID'})
    gt['BDMAP_ID'] = gt['BDMAP_ID'].apply(normalize_id)
    for organ in ORGANS:
        gt[f'gt_{organ}'] = (gt[f'number of {organ} lesion instances'].to_numpy() >= 1).astype(int)
    gt = gt.drop_duplicates(subset=['BDMAP_ID'], keep='last')
    pred = pd.read_csv(predictions_csv)
    pred['BDMAP_ID'] = pred['BDMAP_ID'].apply(normalize_id)
    pred = pred[['BDMAP_ID'] + [f'{organ} tumor volume predicted' for organ in ORGANS]]
    pred = pred.drop_duplicates(subset=['BDMAP_ID'], keep='last')
    return pd.merge(gt, pred, on='BDMAP_ID', how='inner')


def confusion(gt_bin, volumes, threshold):
    """(TP, FP, TN, FN) as Python ints; a NaN volume is a negative prediction."""
    pred = volumes >= threshold
    tp = int(np.count_nonzero(gt_bin & pred))
    fn = int(np.count_nonzero(gt_bin & ~pred))
    fp = int(np.count_nonzero(~gt_bin & pred))
    tn = int(np.count_nonzero(~gt_bin & ~pred))
    return tp, fp, tn, fn


def evaluate_predictions(ground_truth_csv, predictions_csv, output_csv):
    df = merged_tables(ground_truth_csv, predictions_csv)
    fieldnames = ['threshold'] + [f'{organ}_{m}' for organ in ORGANS for m in ('sensitivity', 'specificity', 'f1')]
    cols = {organ: (df[f'gt_{organ}'].to_numpy() == 1, df[f'{organ} tumor volume predicted'].to_numpy(dtype=np.float64)) for organ in ORGANS}
    with open(output_csv, mode='w', newline='') as f:
        w = csv.DictWriter(f, fieldnames=fieldnames)
        w.writeheader()
        for t in THRESHOLDS_VOL:
            row = {'threshold': t}
            for organ in ORGANS:
                tp, fp, tn, fn = confusion(*cols[organ], t)
                row[f'{organ}_sensitivity'] = format_metric(tp, tp + fn)
                row[f'{organ}_specificity'] = format_metric(tn, tn + fp)
                row[f'{organ}_f1'] = format_f1(tp, fp, fn)
            w.writerow(row)
    print(f'Evaluation complete. Results saved to {output_csv}')


def get_parser():
    p = argparse.ArgumentParser(prog='rsuper_amd.calculate_sensitivity_specificity',
                                description='Evaluate predicted tumour volumes against report labels at multiple volume thresholds.')
    p.add_argument('--ground_truth_csv', type=str, required=True, help='ground truth CSV (report-based lesion counts)')
    p.add_argument('--predictions_csv', type=str, required=True, help='predictions CSV (volumes)')
    p.add_argument('--output_csv', type=str, required=True, help='where the metrics are written')
    return p


def main(argv=None):
    a = get_parser().parse_args(argv)
    evaluate_predictions(a.ground_truth_csv, a.predictions_csv, a.output_csv)


if __name__ == '__main__':
    main()
