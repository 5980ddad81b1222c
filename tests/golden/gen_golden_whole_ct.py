#!/usr/bin/env python3
"""Golden vectors for training from whole CTs, produced by the UNMODIFIED reference `AbdomenAtlasDataset` (training/dataset/dim3/
dataset_abdomenatlas_UFO.py: normalize_no_lesion :26, clean_ufo :48, __init__ :125, __getitem__ :414 with save() :936) on the CPU, on the tree of
tests/whole_ct_tree.py.  Run in the authoring container only (it needs the reference, pandas and scipy):

    RSUPER_REFERENCE=<checkout of the reference>/rsuper_train python tests/golden/gen_golden_whole_ct.py

Import shims as in gen_golden_report_crop.py (SimpleITK, nibabel, torchvision).  The only function replaced is `debug_save_labels`, the NIfTI dump of
the first ten samples (out of scope, and the shims cannot write NIfTI).

Writes tests/golden/whole_ct.json (report cleaning, dataset construction, the records of the samples) and tests/golden/whole_ct.npz (the samples'
volumes).  json:
  clean     per annotated_tumors list of whole_ct_tree.CLEAN_TUMORS: healthy (normalize_no_lesion of the table's column), kept (the row labels of the
            cleaned table), ids (ids_of_interest), per_type (tumors_per_type)
  build     per configuration (whole_ct_tree-independent keyword sets, CONFIGS): the image / label lists, UFO_paths and Atlas_paths as sorted base
            names, lengths, both class lists, lesion_classes.  The reference's list ORDER depends on the string hashing of the process and is not pinned.
  samples   per entry of SAMPLES: name, root, seed, ufo, affine (the resampling branch ran), entered (crop functions entered), selected
            (tumor_in_crop), volumes, diameters, next (the next draw of the three generators), corner (un-resampled crops: the crop's corner in the
            padded volume; the image is then whole_ct_tree.image's box and is not stored), files (what save() wrote: name -> [dtype, shape] for .npy,
            the parsed content for .json, the rows for .csv); for affine samples theta, large_corner and e_ref (the reference's own distance from the
            float64 trilinear value: the bound of tests/test_gpu_augment.py is 2 * e_ref)
npz: per sample k: label_k / unk_k / mask_k = np.packbits(axis=0) of what __getitem__ returned (equal to the files save() wrote: asserted here), and
img_k for affine samples.
"""
import contextlib
import io
import json
import os
import random
import sys
import tempfile

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [HERE, os.path.dirname(HERE)]
import gen_golden_augment as GA  # noqa: E402
import gen_golden_report_crop as GR  # noqa: E402
import whole_ct_tree as T  # noqa: E402

CONFIGS = {
    'train': dict(mode='train'),
    'test': dict(mode='test'),
    'all_train': dict(mode='train', all_train=True),
    'all_train_unbalanced': dict(mode='train', all_train=True, balance_supervision=False),
    'ufo_only': dict(mode='train', all_train=True, UFO_only=True, balance_supervision=False),
    'atlas_only': dict(mode='train', all_train=True, Atlas_only=True, balance_supervision=False),
}
# (case, root, seed): the seeds were picked with `--scan` so that every branch occurs (main() asserts it)
SAMPLES = [
    ('BDMAP_00000001', 'atlas', 0), ('BDMAP_00000002', 'atlas', 5), ('BDMAP_00000003', 'atlas', 1), ('BDMAP_00000004', 'atlas', 7),
    ('BDMAP_00000005', 'atlas', 2), ('BDMAP_00000006', 'atlas', 3),
    ('BDMAP_00001001', 'ufo', 0), ('BDMAP_00001001', 'ufo', 7), ('BDMAP_00001002', 'ufo', 1), ('BDMAP_00001003', 'ufo', 0),
    ('BDMAP_00001004', 'ufo', 0),
]


def quiet():
    return contextlib.redirect_stderr(io.StringIO()), contextlib.redirect_stdout(io.StringIO())


def build_reference_dataset(refds, tree, save_destination=None, **kw):
    args = T.args_for(tree)
    random.seed(0)
    e, o = quiet()
    with e, o:
        return refds.AbdomenAtlasDataset(args, seed=0, crop_on_tumor=True, save_destination=save_destination, save_augmented=save_destination is not None,
                                         tumor_classes=list(T.TUMOR_CLASSES), **kw)


def base(paths):
    return sorted(os.path.basename(p) for p in paths)


def run_sample(refds, aug, ds, tree, name, root, seed, dest):
    path = [p for p in ds.img_list if os.path.basename(p).startswith(name) and os.path.dirname(p) == tree['data_root' if root == 'atlas' else 'UFO_root']]
    assert path, (name, root)
    idx = ds.img_list.index(path[0])
    rec = dict(name=name, root=root, seed=seed, ufo=path[0] in ds.UFO_paths, entered=[], affine=False)
    saved, large = [], []

    def spy(owner, attr, hook=None):
        orig = getattr(owner, attr)

        def f(*a, **k):
            rec['entered'].append(attr)
            if hook:
                hook(a, k)
            return orig(*a, **k)
        setattr(owner, attr, f)
        saved.append((owner, attr, orig))
    spy(ds, 'random_crop_on_tumor')
    spy(ds, 'random_crop')
    spy(aug, 'crop_foreground_3d')
    spy(aug, 'random_scale_rotate_translate_3d', lambda a, k: (rec.__setitem__('affine', True), large.append(a[0].clone())))
    for f in os.listdir(dest):
        os.remove(os.path.join(dest, f))
    random.seed(seed), np.random.seed(seed), torch.manual_seed(seed)
    cwd = os.getcwd()
    e, o = quiet()
    try:
        with tempfile.TemporaryDirectory() as tmp, e, o, GA.CaptureTheta() as cap:
            os.chdir(tmp)                                          # crop() writes zero_masks.yaml where it stands
            out = ds[idx]
            thetas = list(cap.thetas)
    finally:
        os.chdir(cwd)
        for owner, attr, orig in saved:
            if owner is ds:
                delattr(ds, attr)
            else:
                setattr(owner, attr, orig)
    rec['next'] = {'np': float(np.random.random()), 'random': random.random(), 'torch': float(torch.rand(1))}
    vols = {k: np.packbits(out[k].numpy().astype(bool), axis=0) for k in ('label', 'unk_channels', 'mask')}
    rec['volumes'], rec['diameters'] = [float(v) for v in out['volumes']], out['diameters'].float().numpy().tolist()
    img = out['image'].numpy()
    assert img.shape == (1,) + T.TRAINING_SIZE and img.dtype == np.float32
    shape = (T.ATLAS if root == 'atlas' else T.UFO)[name][0]
    full = [max(s, l) for s, l in zip(shape, T.LARGE)]
    extra = {}
    if rec['affine']:
        assert len(thetas) == 1 and len(large) == 1
        theta = thetas[0][0].numpy()
        big = large[0]
        rec['theta'], rec['large_corner'] = theta.tolist(), T.corner_of(big.numpy(), full, shape)
        f64 = GA.center(GA.trilinear_f64(big, torch.from_numpy(theta)), T.TRAINING_SIZE).numpy()
        rec['e_ref'] = float(np.abs(img.astype(np.float64) - f64.reshape(img.shape)).max())
        extra['img'] = img
    else:
        rec['corner'] = c = T.corner_of(img, full, shape)
        d, h, w = T.TRAINING_SIZE
        assert np.array_equal(img[0], T.padded(T.image(shape), full)[c[0]:c[0] + d, c[1]:c[1] + h, c[2]:c[2] + w])
    # what save() wrote
    files = {}
    for f in sorted(os.listdir(dest)):
        p = os.path.join(dest, f)
        if f.endswith('.npy'):
            a = np.load(p)
            files[f] = [str(a.dtype), list(a.shape)]
            key = {'_gt.npy': 'label', '_gt_unk.npy': 'unk_channels', '_gt_chosen_tumor_segment.npy': 'mask'}.get(f[len(name):])
            assert np.array_equal(a, vols[key] if key else img), f
        elif f.endswith('.json'):
            with open(p) as fh:
                files[f] = json.load(fh)
        else:
            with open(p) as fh:
                files[f] = fh.read()
    rec['files'] = files
    rec['selected'] = files[name + '.json']['tumor_in_crop']
    return rec, vols, extra


def scan(refds, aug, tree, dest):
    ds = build_reference_dataset(refds, tree, save_destination=dest, all_train=True, balance_supervision=False)
    for name, root in [(n, 'atlas') for n in T.ATLAS] + [(n, 'ufo') for n in T.UFO if n != 'BDMAP_00001006' and n != 'BDMAP_00000003']:
        for seed in range(12):
            rec, _, _ = run_sample(refds, aug, ds, tree, name, root, seed, dest)
            print(name, root, seed, 'affine' if rec['affine'] else 'direct', rec['entered'], rec['selected'], flush=True)


def main():
    refds, aug = GR.import_reference()
    refds.debug_save_labels = lambda *a, **k: None
    out = {}
    # ---- report cleaning
    table = T.clean_table()
    out['clean'] = []
    for tumors in T.CLEAN_TUMORS:
        e, o = quiet()
        with e, o:
            rows, ids, per_type = refds.clean_ufo(table.copy(), list(tumors))
        out['clean'].append(dict(tumors=tumors, kept=[int(i) for i in rows.index], ids=list(ids), per_type=per_type,
                                 healthy=[bool(v) for v in refds.normalize_no_lesion(table['no lesion'])]))
    with tempfile.TemporaryDirectory() as tmp:
        tree = T.build(os.path.join(tmp, 'tree'))
        dest = os.path.join(tmp, 'crops')
        os.makedirs(dest)
        if '--scan' in sys.argv:
            return scan(refds, aug, tree, dest)
        # ---- construction
        out['build'] = {}
        for key, kw in CONFIGS.items():
            ds = build_reference_dataset(refds, tree, **kw)
            out['build'][key] = dict(img_list=base(ds.img_list), lab_list=base(ds.lab_list), ufo=base(ds.UFO_paths), atlas=base(ds.Atlas_paths),
                                     n=len(ds.img_list), classes=ds.classes, classes_ufo=ds.classes_UFO, lesion_classes=ds.lesion_classes,
                                     report_ids=sorted(set(ds.reports['BDMAP_ID'])))
        # ---- samples
        ds = build_reference_dataset(refds, tree, save_destination=dest, all_train=True, balance_supervision=False)
        recs, arrays = [], {}
        for k, (name, root, seed) in enumerate(SAMPLES):
            rec, vols, extra = run_sample(refds, aug, ds, tree, name, root, seed, dest)
            recs.append(rec)
            arrays.update({'label_%d' % k: vols['label'], 'unk_%d' % k: vols['unk_channels'], 'mask_%d' % k: vols['mask']})
            arrays.update({'%s_%d' % (n, k): v for n, v in extra.items()})
            print(name, root, seed, 'affine' if rec['affine'] else 'direct', rec['entered'], rec['selected'], rec.get('corner'))
        out['samples'] = recs
    atlas, ufo = [r for r in recs if not r['ufo']], [r for r in recs if r['ufo']]
    assert len(recs) >= 8 and any(r['affine'] for r in atlas) and any(not r['affine'] for r in atlas), 'direct and affine annotated samples'
    assert all(not r['affine'] for r in ufo), 'report volumes must take un-resampled crops here (their volumes are pinned bit for bit)'
    assert any(r['selected'] not in (None, 'random') for r in ufo), 'a report crop'
    assert any(r['selected'] == 'random' and 'random_crop_on_tumor' in r['entered'] for r in ufo), 'a fallback'
    with open(os.path.join(HERE, 'whole_ct.json'), 'w') as f:
        json.dump(out, f, indent=1, sort_keys=True)
    path = os.path.join(HERE, 'whole_ct.npz')
    np.savez_compressed(path, **arrays)
    print('wrote', path, os.path.getsize(path), 'bytes and whole_ct.json', os.path.getsize(os.path.join(HERE, 'whole_ct.json')), 'bytes')


if __name__ == '__main__':
    main()
