"""python -m rsuper_amd.tools.measure_lesions --data_root DIR --out reports.csv [--parts N --current_part i]

Report rows from per-voxel annotations: every `<id>_gt.npy` of a packed training directory (tools/pack_dataset.py, dataset_conversion/nii2packed.py;
classes: the sorted `list/label_names.yaml`) is uploaded as it is, the lesion planes are measured on the device (inference.lesion_table reads the
packed bits) and each lesion becomes one row 'BDMAP ID', 'Standardized Organ', 'Standardized Location', 'Tumor Size (mm)' -- the columns
training/dataset/reports.py reads.  The location is the organ sub-segment (classes named '<organ>_...') the lesion shares most voxels with, 'u' when
the label has none.  With such a file the report losses can be trained and ablated on annotated data without an extraction pass over free text.

Sizes are geometric measurements between voxel centres plus one voxel per extent (--pad none: without it), not a radiologist's; see
inference/lesions.py lesion_report_rows.  --spacing_csv gives the voxel spacing per case (BDMAP_ID and one column per array axis); 1 mm otherwise,
which is what the packed training directories hold.  --parts / --current_part split the sorted cases with np.array_split, as the other tools do; a
part appends to --out, so the parts of one run may share a file or write one each."""
import argparse
import csv
import os

import numpy as np

COLUMNS = ('BDMAP ID', 'Standardized Organ', 'Standardized Location', 'Tumor Size (mm)')


def get_parser():
    p = argparse.ArgumentParser(prog='rsuper_amd.tools.measure_lesions', description='Measure the annotated lesions of a packed directory into report rows')
    p.add_argument('--data_root', type=str, required=True, help='directory with <id>_gt.npy and list/label_names.yaml')
    p.add_argument('--out', type=str, required=True, help='CSV to append the report rows to')
    p.add_argument('--spacing_csv', type=str, default=None, help='CSV with BDMAP_ID and one spacing column per array axis (default: 1 mm)')
    p.add_argument('--min_voxels', type=int, default=1)
    p.add_argument('--max_lesions', type=int, default=64)
    p.add_argument('--conn', type=int, default=26, choices=(6, 26))
    p.add_argument('--pad', type=str, default='voxel', choices=('voxel', 'none'))
    p.add_argument('--parts', type=int, default=1)
    p.add_argument('--current_part', type=int, default=0)
    return p


def list_cases(data_root):
    return sorted(f[:-len('_gt.npy')] for f in os.listdir(data_root) if f.endswith('_gt.npy'))


def lesion_channels(classes):
    return [i for i, c in enumerate(classes) if 'lesion' in c]


def case_rows(case_id, label, classes, spacing, a):
    """The report rows of one case; label: PackedBits (1, P, D, H, W) of `classes`."""
    from ..inference.lesions import lesion_report_rows, lesion_table, locate_lesions, segment_classes
    from ..inference.postprocess import organ_name
    chs = lesion_channels(classes)
    if not chs:
        return []
    table = lesion_table(label, spacing=spacing, conn=a.conn, min_voxels=a.min_voxels, max_lesions=a.max_lesions, return_labels=True, channels=chs)
    rows = []
    for p, c in enumerate(chs):
        if table.count(p) == 0:
            continue
        segs = segment_classes(classes[c], classes)
        loc = None
        if segs:
            idx = [classes.index(s) for s in segs]
            loc = locate_lesions(table.plane(p), label.planes(idx)[0][idx], segs)
        for r in lesion_report_rows(table, organ_name(classes[c]), location=loc, pad=None if a.pad == 'none' else a.pad, plane=p):
            rows.append(dict({'BDMAP ID': case_id}, **r))
    return rows


def append_rows(path, rows):
    new = not os.path.exists(path)
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, 'a', newline='') as f:
        w = csv.DictWriter(f, fieldnames=list(COLUMNS), lineterminator='\n')
        if new:
            w.writeheader()
        w.writerows(rows)


def main(argv=None):
    """Returns the ids measured and the number of rows written."""
    from ..dataset_conversion.nii2packed import split_part
    from ..hip import lib
    from ..test_with_reports import read_spacing_csv
    from ..training.dataset.packed import upload_label
    from ..training.dataset.whole_ct import read_label_names
    a = get_parser().parse_args(argv)
    classes = read_label_names(a.data_root)
    cases = split_part(list_cases(a.data_root), a.parts, a.current_part)
    spacings = read_spacing_csv(a.spacing_csv)
    n = 0
    if cases:
        lib.require_device()
    for cid in cases:
        label = upload_label(np.load(os.path.join(a.data_root, cid + '_gt.npy'), mmap_mode='r'), len(classes))
        rows = case_rows(cid, label, classes, spacings.get(cid, (1.0, 1.0, 1.0)), a)
        append_rows(a.out, rows)
        n += len(rows)
        print(f'{cid}: {len(rows)} lesions')
    return cases, n


if __name__ == '__main__':
    main()
