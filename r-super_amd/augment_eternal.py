"""python -m rsuper_amd.augment_eternal --data_root DIR [--UFO_root DIR --reports CSV] --save_destination DIR [--passes N]

The device counterpart of the reference's AugmentEternal.py: walks the whole-CT dataset, crops on the device (training/dataset/whole_ct.py
WholeVolumeLoader) and writes each crop with `save_crop` in the file set of `AbdomenAtlasDataset.save` (dataset_abdomenatlas_UFO.py:936-992):
`<id>.npy`, `<id>_gt.npy`, `<id>_gt_unk.npy`, `<id>_gt_chosen_tumor_segment.npy`, `<id>.json`, `<id>_tumor_volumes.json`, `<id>_tumor_diameters.json`
and, for report-supervised cases, `<id>.csv`.  `train_ddp --load_augmented` (AugmentedCropDataset) and the reference's load_augmented_data read the
directory.  A new pass overwrites the crops of the pass before, as the reference's endless producer does; `--passes` ends it (default: endless).
`--crops_per_visit K` cuts K crops from each uploaded volume: the first keeps the reference's name, crop k > 0 is written as `<id>_v<k>` (more
samples for AugmentedCropDataset.from_directory; the reference's loader, which goes by its own case list, does not see them).
The intensity transforms are not applied (the reference skips them with save_augmented, :493): they run at training time.
"""
import argparse
import itertools
import os
import sys


def get_parser():
    p = argparse.ArgumentParser(description='write training crops from whole CTs, on the device')
    p.add_argument('--data_root', '--dataset_path', dest='data_root', required=True, help='per-voxel-annotated root')
    p.add_argument('--UFO_root', default=None, help='report-supervised root')
    p.add_argument('--reports', default=None)
    p.add_argument('--ucsf_ids', default=None)
    p.add_argument('--save_destination', required=True)
    p.add_argument('--training_size', type=int, nargs=3, default=[128, 128, 128])
    p.add_argument('--crop_size', type=int, default=None, help='cubic training_size')
    p.add_argument('--tumor_classes', nargs='+', default=None)
    p.add_argument('--crop_on_tumor', action='store_true')
    p.add_argument('--UFO_only', action='store_true')
    p.add_argument('--Atlas_only', action='store_true')
    p.add_argument('--crops_per_visit', type=int, default=1)
    p.add_argument('--passes', type=int, default=None, help='passes over the dataset (default: endless)')
    p.add_argument('--workers', '--workers_overwrite', dest='workers', type=int, default=0)
    p.add_argument('--seed', type=int, default=0)
    p.add_argument('--no_prefetch', action='store_true')
    p.add_argument('--scale', type=float, default=0.3)
    p.add_argument('--rotate', type=float, default=45)
    p.add_argument('--translate', type=float, default=0.1)
    for name in ('--dataset', '--model', '--dimension', '--batch_size', '--gpu'):       # the reference's command line: accepted, not used
        p.add_argument(name, default=None, help=argparse.SUPPRESS)
    return p


def write_batch(loader, batch, dest):
    """One save_crop per sample of the batch the loader just yielded -> the names written."""
    from .training.dataset.augmented import save_crop
    from .training.dataset.packed import PackedBits
    C, K, names = loader.dataset.num_classes, loader.crops_per_visit, []
    for j, (item, meta) in enumerate(zip(loader.last_items, loader.last_meta)):
        k = j % K
        img_path, lab_path = item['path'], item['lab_path']
        if k:
            stem = os.path.basename(img_path).split('.')[0] + '_v%d' % k
            img_path, lab_path = stem + '.npy', stem + '_gt.npy'
        one = lambda key: PackedBits(batch[key].packed[j:j + 1], C)
        ufo = meta is not None
        save_crop(dest, img_path, lab_path, batch['image'][j], one('label'), one('unk_channels'), one('mask'),
                  meta={'tumor_in_crop': meta['tumor_in_crop'] if ufo else None, 'unknown_per_voxel': meta['unknown_per_voxel'] if ufo else {}},
                  report_rows=item['report'] if ufo else None,
                  tumor_volumes=meta['volumes_host'] if ufo else [0] * 10, tumor_diameters=batch['diameters'][j])
        names.append(os.path.basename(img_path).replace('.npz', '.npy'))
    return names


def run(a, log=None):
    import random
    from .hip import lib as _l
    from .training.dataset.whole_ct import WholeVolumeDataset, WholeVolumeLoader
    _l.require_device()
    if a.crop_size is not None:
        a.training_size = [a.crop_size] * 3
    random.seed(a.seed)
    kw = {} if a.tumor_classes is None else {'tumor_classes': a.tumor_classes}
    ds = WholeVolumeDataset(a, mode='train', seed=a.seed, all_train=True, crop_on_tumor=a.crop_on_tumor, balance_supervision=False, UFO_only=a.UFO_only,
                            Atlas_only=a.Atlas_only, **kw)
    loader = WholeVolumeLoader(ds, batch_size=1, num_workers=a.workers, prefetch=not a.no_prefetch, crops_per_visit=a.crops_per_visit)
    written = 0
    for n in (itertools.count() if a.passes is None else range(a.passes)):
        for batch in loader:
            loader.prefetch_next()          # the next volume's upload and crop are queued before this one's crops are read back and written
            names = write_batch(loader, batch, a.save_destination)
            written += len(names)
            if log:
                log('pass %d: %s' % (n, ' '.join(names)))
    return written


def main(argv=None):
    a = get_parser().parse_args(argv)
    n = run(a, log=lambda m: print(m, file=sys.stderr, flush=True))
    print('wrote %d crops into %s' % (n, a.save_destination))


if __name__ == '__main__':
    main()
