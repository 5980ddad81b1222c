"""python -m rsuper_amd.test_with_reports: the tumour volumes of rsuper_train/test_with_reports.py over a tree of saved predictions, measured on the
device.  `python -m rsuper_amd.eval_AUC` is the same walk with the nine-threshold flow of eval_AUC.py (this module's `run(argv, 'auc')`).

The tree is `<outputs_folder>/<case>/predictions/<class>.npz` (or one packed `<case>/predictions.npz`) for the binary flow and
`<case>/predictions_raw/<class>.npz` for the probability flow -- what `python -m rsuper_amd.predict_abdomenatlas` writes, or a reference tree whose
NIfTI files were converted to `.npz`.  Spacings come from `--spacing_csv` (BDMAP_ID plus one column per ARRAY axis), 1 mm without it: there is no
NIfTI reader here.  File names and column order are the reference's: sorted keys of the first row, `tumor_detection_results.csv`, and
`tumor_detection_results_th0.1.csv` ... `_th0.9.csv`."""
import argparse
import csv
import os

import numpy as np

from .inference.scoring import column_name, normalize_id, score_case

CSV_NAME = 'tumor_detection_results.csv'
CONF = tuple(i / 10 for i in range(1, 10))


def split_into_parts(file_list, n_parts, part_index):
    """Part `part_index` of `n_parts` nearly equal consecutive parts (the first `remainder` parts hold one more); the last part runs to the end."""
    if n_parts <= 0:
        raise ValueError(f'n_parts must be positive, got {n_parts}')
    if part_index < 0 or part_index >= n_parts:
        raise ValueError(f'part_index {part_index} is outside 0 .. {n_parts - 1}')
    step, remainder = divmod(len(file_list), n_parts)
    start = part_index * step + min(part_index, remainder)
    if part_index == n_parts - 1:
        return file_list[start:]
    return file_list[start:start + step + (1 if part_index < remainder else 0)]


def write_csv_row(row, csv_columns, path):
    """Append one row under the alphabetically sorted columns; the header goes in front of the first row of a new file."""
    header = not os.path.exists(path)
    with open(path, mode='a', newline='') as f:
        w = csv.DictWriter(f, fieldnames=sorted(csv_columns))
        if header:
            w.writeheader()
        w.writerow(row)


def csv_paths(outputs_folder, flow):
    base = os.path.join(outputs_folder, CSV_NAME)
    return [base] if flow == 'binary' else [base.replace('.csv', f'_th{t}.csv') for t in CONF]


def append_rows(outputs_folder, row, rows_by_threshold, columns=None):
    """Append a case's rows to the CSVs of the flows it has (row: binary flow; rows_by_threshold: {0.1: row, ...}).  columns: {flow: column list};
    by default the sorted keys of the rows themselves."""
    if row is not None:
        write_csv_row(row, (columns or {}).get('binary') or sorted(row), csv_paths(outputs_folder, 'binary')[0])
    if rows_by_threshold is not None:
        for t, path in zip(CONF, csv_paths(outputs_folder, 'auc')):
            write_csv_row(rows_by_threshold[t], (columns or {}).get('auc') or sorted(rows_by_threshold[t]), path)


def read_ids(path):
    with open(path, newline='') as f:
        return [r['BDMAP_ID'] for r in csv.DictReader(f)]


def read_spacing_csv(path):
    """{BDMAP_ID: (s0, s1, s2)}: the columns after BDMAP_ID, in file order, are the spacings of the array axes."""
    if path is None:
        return {}
    out = {}
    with open(path, newline='') as f:
        rd = csv.DictReader(f)
        cols = [c for c in rd.fieldnames if c != 'BDMAP_ID']
        if len(cols) != 3:
            raise ValueError(f'{path}: expected BDMAP_ID and three spacing columns (one per array axis), got {rd.fieldnames}')
        for r in rd:
            out[normalize_id(r['BDMAP_ID'])] = tuple(float(r[c]) for c in cols)
    return out


def load_planes(case_dir, flow):
    """{lesion class: array} of a saved case.  Binary flow: predictions/<class>.npz, <class>.npz in the case folder, or the packed predictions.npz."""
    sub = 'predictions' if flow == 'binary' else 'predictions_raw'
    folder = os.path.join(case_dir, sub)
    if not os.path.isdir(folder):
        packed = os.path.join(case_dir, 'predictions.npz')
        if flow == 'binary' and os.path.isfile(packed):
            with np.load(packed) as z:
                names = [str(c) for c in z['classes']]
                bits = np.unpackbits(z['arr_0'], axis=0)[:len(names)]
            return {c: bits[i] for i, c in enumerate(names) if column_name(c) is not None}
        folder = case_dir
    out = {}
    for f in sorted(os.listdir(folder)):
        if f.endswith('.nii.gz'):
            raise ValueError(f'{os.path.join(folder, f)}: NIfTI predictions are not read here; convert them to .npz (INTEGRATION section 3g)')
        if f.endswith('.npz') and column_name(f[:-4]) is not None and f != 'predictions.npz':
            with np.load(os.path.join(folder, f)) as z:
                out[f[:-4]] = z['arr_0']
    return out


def process_case(case, args, flow, spacings):
    case_dir = os.path.join(args.outputs_folder, case)
    if not os.path.isdir(case_dir):
        return None
    planes = load_planes(case_dir, flow)
    spacing = spacings.get(normalize_id(case).replace('.npz', ''), (1.0, 1.0, 1.0))
    if flow == 'binary':
        return score_case(planes, None, list(planes), spacing, th=args.th, case_id=case)[0]
    return score_case({}, planes, list(planes), spacing, case_id=case)[1]


def get_parser(flow='binary'):
    p = argparse.ArgumentParser(prog='rsuper_amd.' + ('test_with_reports' if flow == 'binary' else 'eval_AUC'),
                                description='Measure saved lesion predictions on the device and append the volumes to the CSV(s).')
    p.add_argument('--outputs_folder', type=str, required=True, help='folder with one sub-folder of saved predictions per case')
    p.add_argument('--ct_folder', type=str, default=None, help='accepted for the reference command line; spacings come from --spacing_csv')
    p.add_argument('--spacing_csv', type=str, default=None, help='CSV with BDMAP_ID and one spacing column per array axis (default: 1 mm)')
    p.add_argument('--th', type=float, default=0.5, help='threshold that binarises a saved mask (binary flow)')
    p.add_argument('--workers', type=int, default=10, help='accepted for the reference command line; the device measures one case at a time')
    p.add_argument('--cases', default=None, help='CSV whose BDMAP_ID column lists the cases to evaluate')
    p.add_argument('--continuing', action='store_true', help='skip the cases already in the CSV')
    p.add_argument('--parts', type=int, default=1, help='number of parts to split the cases into')
    p.add_argument('--part', type=int, default=0, help='part to process')
    p.add_argument('--any_lesion', action='store_true', help='NOT SUPPORTED: nothing in the reference writes an any_lesion prediction')
    return p


def run(argv=None, flow='binary'):
    args = get_parser(flow).parse_args(argv)
    if args.any_lesion:
        raise SystemExit('--any_lesion is not supported: nothing in the reference writes an any_lesion prediction')
    paths = csv_paths(args.outputs_folder, flow)
    all_files = [f for f in os.listdir(args.outputs_folder) if os.path.isdir(os.path.join(args.outputs_folder, f))]
    if os.path.exists(paths[0]) and args.continuing:
        done = set(read_ids(paths[0]))
        files = [f for f in all_files if normalize_id(f) not in done]
        print(f'Resuming: skipping {len(done)} already processed items.')
    else:
        if os.path.exists(paths[0]) and (args.parts == 1 or args.part == 0):
            for p in paths:
                os.remove(p)
            print(f"Existing CSV '{paths[0]}' removed. Starting fresh.")
        files = all_files
    if not files:
        print('No new files to process. Exiting.')
        return []
    if args.cases is not None:
        ids = set(read_ids(args.cases))
        files = [f for f in files if f.replace('.nii.gz', '').replace('_0000', '') in ids]
    files = sorted(files)
    if args.parts > 1:
        files = split_into_parts(files, args.parts, args.part)
    spacings = read_spacing_csv(args.spacing_csv)
    columns, out = None, []
    for f in files:
        res = process_case(f, args, flow, spacings)
        if res is None:
            continue
        if columns is None:
            columns = sorted(res if flow == 'binary' else res[CONF[0]])
        if flow == 'binary':
            write_csv_row(res, columns, paths[0])
        else:
            for t, p in zip(CONF, paths):
                write_csv_row(res[t], columns, p)
        out.append(res)
    print('CSV file saved at:', paths[0])
    return out


def main(argv=None):
    return run(argv, 'binary')


if __name__ == '__main__':
    main()
