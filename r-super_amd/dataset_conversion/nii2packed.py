"""python -m rsuper_amd.dataset_conversion.nii2packed --src_path DIR --label_path DIR --tgt_path DIR [--label_yaml FILE] ...

An AbdomenAtlas-style tree (`<src>/<id>/ct.nii.gz` or `<src>/<id>.nii.gz`, `<label>/<id>/segmentations/<class>.nii.gz`) to the directory
`train_ddp --dataset abdomenatlas[_ufo] --data_root` reads, in one step and without SimpleITK: what the reference's dataset_conversion/abdomenatlas_3d.py
followed by dataset_conversion/nii2npz.py (and this package's tools/pack_dataset.py) produce.  The flags are those of the two reference scripts.
Per case `<tgt>/<id>.npy` (float32 image, z-scored, padded to 128) and `<tgt>/<id>_gt.npy` (the label as np.packbits(axis=0)); `<tgt>/list/label_names.yaml`
and `<tgt>/list/dataset.yaml`.  With --nnunet_labels_used the labels are one integer map per case (`<label>/<id>_0000.nii.gz`, `<id>_0000.nii.gz.nii.gz` or
`<id>.nii.gz`) and --nnunet_labels names a YAML file {class name: value or list of values}.
"""
import argparse
import csv
import os
import sys
from concurrent.futures import ThreadPoolExecutor

import numpy as np


def build_parser():
    p = argparse.ArgumentParser(description=__doc__.split('\n\n')[1])
    p.add_argument('--src_path', type=str, required=True, help='Source path for the CT images.')
    p.add_argument('--label_path', type=str, required=True, help='Label path for the segmentation masks.')
    p.add_argument('--tgt_path', type=str, required=True, help='Target path for the processed outputs.')
    p.add_argument('--parts', type=int, default=1, help='Number of parts to split the dataset into (default 1, meaning no split).')
    p.add_argument('--current_part', type=int, default=0, help='The index (0-based) of the current part to process.')
    p.add_argument('--nnunet_labels_used', action='store_true', help='The labels are nnU-Net label maps, one integer volume per case.')
    p.add_argument('--nnunet_labels', type=str, default=None, help='YAML file {class name: value or list of values} of the label maps.')
    p.add_argument('--workers', type=int, default=8, help='Reader threads (files are read and inflated ahead of the device).')
    p.add_argument('--overwrite', action='store_true', help='Overwrite already processed cases.')
    p.add_argument('--add_lesions', type=str, default=None, help='Path to a yaml file with the lesions to add to the classes list here.')
    p.add_argument('--label_yaml', type=str, default=None, help='Path to a yaml file with the label names.')
    p.add_argument('--ids', default=None, help='IDS in the dataset. path to a csv with a column BDMAP ID')
    p.add_argument('--min_size', type=int, default=128, help='Pad every shorter axis to at least this (the reference: 128).')
    return p


def _strip(name):
    return name.replace('_0000.nii.gz', '').replace('.nii.gz', '').replace('.npz', '')


def case_names(label_path, ids_csv=None, nnunet=False):
    """The entries of label_path (sorted), kept if --ids lists them (column 'BDMAP ID')."""
    names = sorted(os.listdir(label_path))
    if ids_csv is not None:
        with open(ids_csv, newline='') as f:
            keep = {row['BDMAP ID'] for row in csv.DictReader(f)}
        names = [n for n in names if n.replace('.nii.gz', '').replace('.npz', '') in keep]
    return [_strip(n) for n in names] if nnunet else names


def split_part(names, parts, current_part):
    """np.array_split(names, parts)[current_part], as both reference scripts split."""
    if parts <= 1:
        return list(names)
    splits = np.array_split(np.asarray(names, dtype=object), parts)
    if current_part < 0 or current_part >= len(splits):
        raise ValueError(f'current_part must be between 0 and {len(splits) - 1}')
    return splits[current_part].tolist()


def merge_lesions(label_names, lesions):
    """--add_lesions: extend, drop duplicates, sort (abdomenatlas_3d.py :291-298)."""
    return sorted(set(list(label_names) + list(lesions)))


def label_names_of(args, names):
    import yaml
    if args.label_yaml is not None:
        with open(args.label_yaml) as f:
            labels = list(yaml.safe_load(f))
    else:
        seg_dir = os.path.join(args.label_path, names[0], 'segmentations')
        labels = sorted(fn.replace('.nii.gz', '') for fn in os.listdir(seg_dir) if fn.endswith('.nii.gz') and 'background' not in fn)
        if not labels:
            raise ValueError(f'No .nii.gz label found in {seg_dir}')
    if args.add_lesions is not None:
        with open(args.add_lesions) as f:
            labels = merge_lesions(labels, yaml.safe_load(f))
    return labels


def find_label_map(label_path, name):
    for p in (name + '_0000.nii.gz', name + '_0000.nii.gz.nii.gz', name + '.nii.gz'):
        if os.path.exists(os.path.join(label_path, p)):
            return os.path.join(label_path, p)
    return None


def find_ct_nnunet(src_path, name):
    for p in (name + '_0000.nii.gz', name + '.nii.gz', os.path.join(name, 'ct.nii.gz')):
        if os.path.exists(os.path.join(src_path, p)):
            return os.path.join(src_path, p)
    return None


def convert(args, log=None):
    """Convert the cases of this part; the ids that were written."""
    import yaml
    from ..hip import lib as _l
    from . import nii_dataset as nd
    _l.require_device()
    log = log or (lambda m: None)
    nnunet = bool(args.nnunet_labels_used)
    names = case_names(args.label_path, args.ids, nnunet)
    log(f'Number of cases: {len(names)}')
    names = split_part(names, args.parts, args.current_part)
    if not names:
        return []
    lut = table = None
    if nnunet:
        if args.nnunet_labels is None:
            raise ValueError('--nnunet_labels_used needs --nnunet_labels YAML (class name -> value or list of values)')
        with open(args.nnunet_labels) as f:
            table = yaml.safe_load(f)
        labels = sorted(table)
        lut = nd.build_lut(labels, table)
    else:
        labels = label_names_of(args, names)
    os.makedirs(os.path.join(args.tgt_path, 'list'), exist_ok=True)
    with open(os.path.join(args.tgt_path, 'list', 'dataset.yaml'), 'w', encoding='utf-8') as f:
        yaml.dump(list(names), f)
    with open(os.path.join(args.tgt_path, 'list', 'label_names.yaml'), 'w', encoding='utf-8') as f:
        yaml.dump(list(labels), f)
    done = []
    with ThreadPoolExecutor(max_workers=max(1, int(args.workers))) as reader:
        for name in names:
            img_out, lab_out = os.path.join(args.tgt_path, name + '.npy'), os.path.join(args.tgt_path, name + '_gt.npy')
            if os.path.exists(img_out) and os.path.exists(lab_out) and not args.overwrite:
                log(f'Skipping {name}: All outputs already exist.')
                continue
            ct = find_ct_nnunet(args.src_path, name) if nnunet else nd.find_ct(args.src_path, name)
            if ct is None:
                log(f'Error processing {name}: no CT under {args.src_path}')
                continue
            if nnunet:
                masks = find_label_map(args.label_path, name)
                if masks is None:
                    log(f'Error processing {name}: no label map under {args.label_path}')
                    continue
            else:
                masks = nd.find_masks(args.label_path, name, labels, log)
            try:
                image, lab, _ = nd.convert_case(ct, masks, labels, min_size=args.min_size, lut=lut, reader=reader)
            except ValueError as e:
                log(f'Error processing {name}: {e}')
                continue
            np.save(img_out, image.cpu().numpy())
            np.save(lab_out, lab.packed[0].cpu().numpy())
            done.append(name)
            log(f'{name} processed successfully.')
    return done


def main(argv=None):
    args = build_parser().parse_args(argv)
    done = convert(args, log=lambda m: print(m, file=sys.stderr, flush=True))
    print('converted %d cases into %s' % (len(done), args.tgt_path))
    return done


if __name__ == '__main__':
    main()
