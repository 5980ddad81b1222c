"""python -m rsuper_amd.tools.refine_pseudo_labels --input_dir DIR --metadata CSV --out_npz_dir DIR [--parts N --part i]
                                                  [--label_list YAML --organs_path DIR --tgt_path DIR [--packed]] [--device_compress]

The report-refined pseudo-label baseline (the reference's baselines/pseudo_labels/pseudo_label_report_refinement.py main, npz branch) with the
candidate extraction on the device.  --input_dir holds one folder per case, `<ID>.npz/` (or, when there is none, `<ID>.nii.gz/`), with the raw
probabilities of the lesion classes in `predictions_raw/<class>.npy | .npz (first array) | .nii.gz` and the thresholded predictions in `predictions/`.
--metadata is the report table: a `BDMAP_ID` (or `BDMAP ID`) column and one `number of <organ> lesion instances` column per organ.

A folder without probability files is copied (`predictions/` -> `<out>/<ID>/`) and counts as kept.  Every other folder goes through refine_case: it is
kept when every lesion class yields as many candidates as the report counts, and then `<out>/<ID>/<class>.npz` (key `mask`, uint8) is written for the
classes with a positive count; otherwise it is skipped.  `<out>/list/dataset.yaml` and `list/skipped.yaml` are read at the start (cases already listed
are not done again) and rebuilt from the output tree at the end.  --parts / --part split the pending folders, sorted by id, with slice_indices.

With --tgt_path (and --label_list, --organs_path) every case refined in this run is also merged with its organ labels `<organs_path>/<ID>_gt.npz`
(plane order: the sorted `<organs_path>/list/label_names.yaml`) into the training label `<tgt_path>/<ID>_gt.npz` (merge_pseudo_labels; the labels of
--label_list in sorted order), or with --packed into the bit-packed `<ID>_gt.npy` tools.pack_dataset writes; `<ID>.npz` and `list/label_names.yaml`
are written next to it.

--device_compress deflates the mask files and `<ID>_gt.npz` on the device (inference/npz_writer.py): the same keys (`mask`, `arr_0`) and arrays under
np.load, other compressed bytes.  Without it every byte written is np.savez_compressed's.

Deviations from the reference, on purpose: the id of a `<ID>.nii.gz/` folder is `<ID>` (Path.stem leaves `<ID>.nii`, which matches no metadata row);
the `list/` folder of the output tree is not listed as a case; there is no NIfTI output tree.  .nii.gz probabilities need nibabel, which this package
does not depend on: where it does not import, such a file stops the run with an error that names it.
"""
import argparse
import os
import shutil
import sys
from pathlib import Path

import numpy as np

from ..baselines.pseudo_labels.pseudo_label_report_refinement import dump_yaml, load_yaml, slice_indices

PROB_SUFFIXES = ('.nii.gz', '.npy', '.npz')


def case_id(folder):
    name = Path(folder).name
    for suffix in ('.nii.gz', '.npz'):
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def class_of(path):
    name = Path(path).name
    for suffix in PROB_SUFFIXES:
        if name.endswith(suffix):
            return name[:-len(suffix)]
    return name


def probability_files(folder):
    """The probability files under `<folder>/predictions_raw`, sorted by class name."""
    raw = Path(folder) / 'predictions_raw'
    if not raw.exists():
        return []
    return sorted((p for p in raw.rglob('*') if p.is_file() and p.name.endswith(PROB_SUFFIXES)), key=class_of)


def discover(input_dir):
    """-> (folders without probabilities, folders with), the reference's discovery: `*.npz` folders, `*.nii.gz` folders when there are none."""
    input_dir = Path(input_dir)
    folders = [p for p in input_dir.glob('*.npz') if p.is_dir()] or [p for p in input_dir.glob('*.nii.gz') if p.is_dir()]
    if not folders:
        raise ValueError(f'{input_dir}: no <ID>.npz/ or <ID>.nii.gz/ case folders')
    empty = [p for p in folders if not probability_files(p)]
    return empty, [p for p in folders if p not in empty]


def load_probability(path):
    """float32 (D, H, W) of one class; a 4-D array gives [..., 0]."""
    path = Path(path)
    if path.name.endswith('.nii.gz'):
        try:
            import nibabel as nib
        except ImportError:
            raise RuntimeError(f'{path}: reading .nii.gz probabilities needs nibabel, which is not installed; store them as .npy or .npz') from None
        a = nib.load(str(path)).get_fdata(dtype=np.float32)
    else:
        a = np.load(path)
        if path.name.endswith('.npz'):
            a = a[a.files[0]]
        a = np.asarray(a, dtype=np.float32)
    return a[..., 0] if a.ndim == 4 else a


def read_metadata(path):
    """{case id: {column: value}} of the report table; an empty cell is NaN, a numeric cell a number (what pandas.read_csv gives the reference)."""
    import csv
    with open(path, newline='') as f:
        rows = list(csv.DictReader(f))
    if not rows:
        return {}
    id_col = 'BDMAP_ID' if 'BDMAP_ID' in rows[0] else 'BDMAP ID'

    def cell(v):
        if v is None or v.strip() == '':
            return float('nan')
        try:
            return int(v)
        except ValueError:
            try:
                return float(v)
            except ValueError:
                return v

    return {r[id_col]: {k: cell(v) for k, v in r.items() if k != id_col} for r in rows}


def copy_predictions(folder, out_root):
    src, dst = Path(folder) / 'predictions', Path(out_root) / case_id(folder)
    if src.exists():
        shutil.copytree(src, dst, dirs_exist_ok=True)
    else:
        dst.mkdir(parents=True, exist_ok=True)


def process_case(folder, meta, out_root, device='cuda', device_compress=False):
    """One folder -> (id, included, {class: device mask})."""
    import torch
    from ..baselines.pseudo_labels import refine_case
    cid = case_id(folder)
    files = probability_files(folder)
    classes = [class_of(p) for p in files]
    lesion = [c if 'lesion' in c else c + '_lesion' for c in classes]           # every file of predictions_raw is a lesion class (:110-112)
    raw = torch.from_numpy(np.stack([load_probability(p) for p in files])).to(device)
    included, masks = refine_case(raw, lesion, meta.get(cid))
    masks = {classes[lesion.index(k)]: v for k, v in masks.items()}
    if included:
        dst = Path(out_root) / cid
        dst.mkdir(parents=True, exist_ok=True)
        if device_compress and masks:
            from ..inference.npz_writer import save_planes_npz
            names = list(masks)
            save_planes_npz([str(dst / (name + '.npz')) for name in names], torch.stack([masks[name].to(torch.uint8) for name in names]), key='mask',
                            table='mask')
        else:
            for name, m in masks.items():
                np.savez_compressed(str(dst / (name + '.npz')), mask=m.cpu().numpy().astype(np.uint8))
    return cid, included, masks


def write_training_label(cid, masks, a, labels, organ_names, device='cuda'):
    import torch
    from ..baselines.pseudo_labels import merge_pseudo_labels
    ct = os.path.join(a.organs_path, cid + '.npz')
    if not os.path.exists(ct):                                                  # before anything is written for the case
        raise ValueError(f'{cid}: the image {ct} is missing')
    organs = np.load(os.path.join(a.organs_path, cid + '_gt.npz'))['arr_0']
    stack = merge_pseudo_labels(torch.from_numpy(np.ascontiguousarray(organs)).to(device), organ_names, masks, labels, packed=a.packed)
    if a.packed:
        np.save(os.path.join(a.tgt_path, cid + '_gt.npy'), stack.packed[0].cpu().numpy())
    elif a.device_compress and stack.dtype in (torch.uint8, torch.int8, torch.bool):
        from ..inference.npz_writer import savez_compressed_device
        savez_compressed_device(os.path.join(a.tgt_path, cid + '_gt.npz'), stack, table='mask')
    else:
        np.savez_compressed(os.path.join(a.tgt_path, cid + '_gt.npz'), stack.cpu().numpy())
    shutil.copy(ct, os.path.join(a.tgt_path, cid + '.npz'))


def main(argv=None):
    p = argparse.ArgumentParser(description='Report-guided refinement of pseudo-labels on the device.')
    p.add_argument('--input_dir', required=True, type=Path)
    p.add_argument('--metadata', required=True, type=Path)
    p.add_argument('--out_npz_dir', required=True, type=Path)
    p.add_argument('--parts', type=int, default=1, help='split the pending cases into this many shares')
    p.add_argument('--part', type=int, default=0, help='which share this run takes, counted from 0')
    p.add_argument('--label_list', type=Path, default=None, help='YAML list of the target labels (with --tgt_path)')
    p.add_argument('--organs_path', type=Path, default=None, help='<ID>.npz, <ID>_gt.npz and list/label_names.yaml of the organ labels (with --tgt_path)')
    p.add_argument('--tgt_path', type=Path, default=None, help='also write the merged training labels here')
    p.add_argument('--packed', action='store_true', help='write the merged label bit-packed, as tools.pack_dataset does')
    p.add_argument('--device_compress', action='store_true', help='deflate the mask files and <ID>_gt.npz on the device (same arrays under np.load)')
    a = p.parse_args(argv)
    if not 0 <= a.part < a.parts:
        raise ValueError(f'--part {a.part} is outside 0 .. {a.parts - 1}')
    if a.tgt_path is not None and (a.label_list is None or a.organs_path is None):
        raise ValueError('--tgt_path needs --label_list and --organs_path')
    log = lambda m: print(m, file=sys.stderr, flush=True)  # noqa: E731

    out = a.out_npz_dir
    (out / 'list').mkdir(parents=True, exist_ok=True)
    kept_yaml, skip_yaml = out / 'list' / 'dataset.yaml', out / 'list' / 'skipped.yaml'
    kept, skipped = load_yaml(kept_yaml), load_yaml(skip_yaml)
    processed = kept | skipped
    meta = read_metadata(a.metadata)
    empty, full = discover(a.input_dir)
    log(f'Number of non-empty predictions_raw found: {len(full)}')
    for d in empty:
        if case_id(d) not in processed:
            copy_predictions(d, out)
            kept.add(case_id(d))

    todo = sorted((d for d in full if case_id(d) not in processed), key=case_id)
    if not todo:
        log('Nothing left to process.')
    else:
        from ..hip import lib as _l
        _l.require_device()
        mine = todo[slice_indices(len(todo), a.parts, a.part)]
        log(f'Total non-empty folders pending: {len(todo)}; slice {a.part}/{a.parts}: {len(mine)} folders')
        labels = organ_names = None
        if a.tgt_path is not None:
            os.makedirs(a.tgt_path / 'list', exist_ok=True)
            labels = sorted(load_yaml(a.label_list))                            # load_yaml / dump_yaml also work where PyYAML is missing
            organ_names = sorted(load_yaml(a.organs_path / 'list' / 'label_names.yaml'))
            if not labels or not organ_names:
                raise ValueError(f'{a.label_list} or {a.organs_path}/list/label_names.yaml is missing or empty')
            dump_yaml(a.tgt_path / 'list' / 'label_names.yaml', labels)
        for d in mine:
            cid, ok, masks = process_case(d, meta, out, device_compress=True) if a.device_compress else process_case(d, meta, out)
            (kept if ok else skipped).add(cid)
            if ok and a.tgt_path is not None:
                write_training_label(cid, masks, a, labels, organ_names)

    kept.update(q.name for q in out.iterdir() if q.is_dir() and q.name != 'list')
    kept.difference_update(skipped)
    dump_yaml(kept_yaml, sorted(kept))
    dump_yaml(skip_yaml, sorted(skipped))
    print(f'kept: {len(kept)}   skipped: {len(skipped)}')
    return sorted(kept), sorted(skipped)


if __name__ == '__main__':
    main()
