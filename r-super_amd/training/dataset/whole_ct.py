"""Training from whole CTs: the file dataset and the loader that turns its volumes into device batches.

`WholeVolumeDataset` restates the construction of `AbdomenAtlasDataset` (rsuper_train/training/dataset/dim3/dataset_abdomenatlas_UFO.py:124-413: directory
scan, report cleaning, supervision balancing, split, class lists) and the file reads of its `__getitem__` (:414-470).  Its `__getitem__` runs in DataLoader
workers and touches no device: it memory-maps the image and the label AS STORED (bit-packed or unpacked) and hands them on.  Everything after the read
-- label upload (packing on the device where the file is unpacked, dataset/packed.py upload_label), padding, crop-on-tumour or report crop,
assign_labels, the two sum checks of SanityAssertOutput (:1456-1464) -- happens in the training process, in `WholeVolumeLoader`, on the kernels of
training/augmentation.py (dataset/whole_volume.py DeviceCropper).  Without a UFO root and reports the same class serves `--dataset abdomenatlas`.

Where the reference orders names through `list(set(...))` (an order that changes from process to process with string hashing) the names are sorted
first, so that the seed alone decides the split and the over-sampling.

As in the reference, the two kinds of supervision are equalised in train mode only: with balance_supervision the train and the test instance shuffle
different name lists, and a tested case may also be trained on.  With balance_supervision=False both modes split one list.

Out of scope: define_unknown_voxels, zero_masks.yaml, no_pancreas_subseg, model_genesis_pretrain, the debug NIfTI dumps, 2-D.
"""
import os
import random
import sys

import numpy as np
import torch
from torch.utils import data

ID_LEN = len('BDMAP_00000000')
MAX_WORKERS = 16
ORGANS_WITH_SIDES = ('kidney', 'adrenal_gland', 'lung', 'breast', 'femur')
_TRUE_WORDS = ('1', '1.0', 'true', 't', 'yes', 'y')
_LESION_WORDS = ('lesion', ' tumor', ' mass', 'cyst', 'pdac', 'pnet')


def _log(*a):
    print(*a, flush=True, file=sys.stderr)


def normalize_no_lesion(col):
    """The 'no lesion' column as booleans (:26-46): True = healthy.  A boolean column is returned as it is; a number (or a text that parses as one) is
    healthy when it equals 1; any other text when it is one of 1 / 1.0 / true / t / yes / y (case and blanks ignored); everything else -- NaN too -- is not."""
    import pandas as pd
    if pd.api.types.is_bool_dtype(col):
        return col
    number = pd.to_numeric(col, errors='coerce')
    numeric = number.notna()
    words = col[~numeric].astype(str).str.strip().str.lower()
    healthy = pd.Series(False, index=col.index)
    healthy[numeric] = number[numeric] == 1
    healthy[words.index[words.isin(_TRUE_WORDS)]] = True
    return healthy


def clean_ufo(reports, annotated_tumors, limit_healthy=True):
    """clean_ufo (:48-122): the report rows worth training on -> (rows, ids_of_interest, tumors_per_type).
      1. a case with a tumour size of '0', '0.0' or '0.0 x ...' (an extraction artefact) is dropped whole;
      2. tumour rows of organs outside annotated_tumors are dropped (healthy rows stay);
      3. a case is dropped whole when one of its tumour rows has no digit in its size or an 'Unknow Tumor Size' other than 'no', or names a sided organ
         (kidney, adrenal gland, lung, breast, femur) without 'left' / 'right' in its location;
      4. per organ the rows of interest have a size other than u / U / multiple, a known size and, for sided organs, a side; the healthy rows are those
         whose 'no lesion' equals True, capped (rows sampled with random_state=42) at the largest organ group's number of cases;
      5. the rows kept are those of every case that has a row of interest."""
    import pandas as pd
    size = reports['Tumor Size (mm)']
    artefact = size.astype(str).str.contains(r'^0\.0\s*x', regex=True, na=False) | (size == '0.0') | (size == '0')
    reports = reports[~reports['BDMAP_ID'].isin(reports.loc[artefact, 'BDMAP_ID'].tolist())]
    reports = reports[reports['Standardized Organ'].isin(annotated_tumors) | normalize_no_lesion(reports['no lesion'])]

    tumour = ~normalize_no_lesion(reports['no lesion'])
    no_digit = ~reports['Tumor Size (mm)'].astype(str).str.contains(r'\d', regex=True, na=False)
    size_unknown = reports['Unknow Tumor Size'].astype(str).str.strip().str.lower() != 'no'
    location = reports['Standardized Location'].astype(str).str.lower()
    unsided = reports['Standardized Organ'].isin(ORGANS_WITH_SIDES) & ~(location.str.contains('left', na=False) | location.str.contains('right', na=False))
    drop = set(reports.loc[tumour & (no_digit | size_unknown), 'BDMAP_ID'].unique()) | set(reports.loc[tumour & unsided, 'BDMAP_ID'].unique())
    reports = reports[~reports['BDMAP_ID'].isin(drop)]

    interest = {}
    for organ in annotated_tumors:
        rows = reports[reports['Standardized Organ'] == organ]
        rows = rows[~rows['Tumor Size (mm)'].isin(['u', 'U', 'multiple'])]
        rows = rows[rows['Unknow Tumor Size'] == 'no']
        if organ in ORGANS_WITH_SIDES:                 # case-sensitive here, as in the reference
            loc = rows['Standardized Location']
            rows = rows[loc.str.contains('right', na=False) | loc.str.contains('left', na=False)]
        interest[organ] = rows
    healthy = reports[reports['no lesion'] == True]    # noqa: E712  (element-wise: the number 1 counts, the text 'True' does not)
    if limit_healthy:
        cap = max(rows['BDMAP_ID'].nunique() for rows in interest.values())
        if healthy['BDMAP_ID'].nunique() > cap:
            healthy = healthy.sample(n=cap, random_state=42)
    interest['healthy'] = healthy
    tumors_per_type = {k: rows['BDMAP_ID'].unique().tolist() for k, rows in interest.items()}
    ids = pd.concat(list(interest.values())).drop_duplicates()['BDMAP_ID'].unique().tolist()
    return reports[reports['BDMAP_ID'].isin(ids)], ids, tumors_per_type


def scan_root(root):
    """Case ids of a data root that have both an image and a `_gt` file (:156-158), sorted."""
    files = [f for f in os.listdir(root) if 'BDMAP' in f]
    return sorted({f[:ID_LEN] for f in files if '_gt' in f} & {f[:ID_LEN] for f in files if '_gt' not in f})


def case_paths(root, name):
    """(<root>/<name>.npy, <root>/<name>_gt.npy), or the .npz pair where the .npy image is missing (:249-261)."""
    img, lab = os.path.join(root, name + '.npy'), os.path.join(root, name + '_gt.npy')
    if not os.path.exists(img):
        img, lab = img.replace('.npy', '.npz'), lab.replace('.npy', '.npz')
    if not os.path.exists(img):
        raise ValueError('Image %s not found in npy nor npz' % img)
    return img, lab


def read_label_names(root):
    import yaml
    with open(os.path.join(root, 'list', 'label_names.yaml')) as f:
        return sorted(yaml.load(f, Loader=yaml.SafeLoader))


def _ids_in(root):
    """The BDMAP ids that occur in the file names of a root (:360-364)."""
    out = set()
    for f in os.listdir(root):
        if 'BDMAP' in f:
            k = f.rfind('BDMAP')
            out.add(f[k:k + ID_LEN])
    return out


def load_array(path):
    """np.load(mmap_mode='r') of a .npy / the arr_0 of a .npz (:436-446); a second attempt without the map, as the reference makes."""
    try:
        a = np.load(path, mmap_mode='r', allow_pickle=False)
        return a['arr_0'] if '.npz' in path else a
    except Exception:
        a = np.load(path)
        return a['arr_0'] if '.npz' in path else a


class WholeVolumeDataset(data.Dataset):
    """See the module docstring.  args: data_root [, UFO_root, reports, ucsf_ids], training_size.  A sample is a dictionary {'image' (D, H, W),
    'label' as stored, 'path', 'lab_path', 'is_ufo', 'report' (the case's rows, or None)[, 'spacing' in mode='test']}."""
    packed = True          # train_epoch: the label volumes of the batches are PackedBits

    def __init__(self, args, mode='train', seed=0, all_train=False, crop_on_tumor=True, tumor_classes=('kidney', 'pancreas'), balance_supervision=True,
                 UFO_only=False, Atlas_only=False):
        super().__init__()
        assert mode in ('train', 'test')
        if UFO_only and Atlas_only:
            raise ValueError('You cannot use both UFO_only and Atlas_only at the same time. Please choose one or the other.')
        self.mode, self.args, self.crop_on_tumor = mode, args, crop_on_tumor
        self.tumor_classes = self.tumor_class_names = list(tumor_classes if tumor_classes is not None else ('kidney', 'pancreas'))
        ufo_root = getattr(args, 'UFO_root', None)
        reports_path = getattr(args, 'reports', None)
        if (ufo_root is None) != (reports_path is None):
            raise ValueError('report-supervised volumes need both --UFO_root and --reports')
        if UFO_only and ufo_root is None:
            raise ValueError('UFO_only needs --UFO_root and --reports')
        atlas_names = scan_root(args.data_root)
        ufo_names, self.reports, self.tumors_per_type, ids = [], None, {}, []
        if ufo_root is not None:
            import pandas as pd
            reports = pd.read_csv(reports_path)
            if 'BDMAP ID' in reports.columns:
                reports = reports.rename(columns={'BDMAP ID': 'BDMAP_ID'})
            ufo_names = scan_root(ufo_root)
            if getattr(args, 'ucsf_ids', None) is not None:
                cases = pd.read_csv(args.ucsf_ids)
                if 'BDMAP ID' in cases.columns:
                    cases = cases.rename(columns={'BDMAP ID': 'BDMAP_ID'})
                keep = set(cases['BDMAP_ID'].tolist())
                ufo_names = [n for n in ufo_names if n in keep]
            reports = reports[reports['BDMAP_ID'].isin(ufo_names)]
            self.reports, ids, self.tumors_per_type = clean_ufo(reports, self.tumor_classes)
            of_interest = set(ids)
            ufo_names = [n for n in ufo_names if n in of_interest]
        self.eligible_ufo, self.eligible_atlas = list(ufo_names), list(atlas_names)

        if mode == 'train' and balance_supervision is True and ufo_root is not None:          # :192-202, the global `random` generator
            if len(atlas_names) > len(ufo_names):
                ufo_names = ufo_names + random.choices(ufo_names, k=len(atlas_names) - len(ufo_names))
            elif len(ufo_names) > len(atlas_names):
                atlas_names = atlas_names + random.choices(atlas_names, k=len(ufo_names) - len(atlas_names))
        if UFO_only:
            names, atlas_names = ufo_names, []
        elif Atlas_only:
            names, ufo_names = atlas_names, []
        else:
            names = atlas_names + ufo_names
        names = list(names)
        random.Random(seed).shuffle(names)
        if not all_train:
            test_names = names[:min(200, len(names) // 10)]
            train_names = sorted(set(names) - set(test_names))       # the reference's set difference also drops the over-sampled repeats
        else:
            train_names, test_names = names, []
        names = train_names if mode == 'train' else test_names

        in_atlas, in_ufo = set(atlas_names), set(ufo_names)
        self.img_list, self.lab_list, self.spacing_list, self.UFO_paths, self.Atlas_paths = [], [], [], [], []
        for name in names:
            if name in in_atlas:                                     # an id of both roots is read from the annotated one
                img, lab = case_paths(args.data_root, name)
                self.Atlas_paths.append(img)
            elif name in in_ufo:
                img, lab = case_paths(ufo_root, name)
                self.UFO_paths.append(img)
            else:
                raise ValueError('Image %s not in any of the two lists' % name)
            self.img_list.append(img)
            self.lab_list.append(lab)
            self.spacing_list.append([1.0, 1.0, 1.0])
        self._ufo = set(self.UFO_paths)

        self.classes = read_label_names(args.data_root)
        self.classes_UFO = read_label_names(ufo_root) if ufo_root is not None else None
        for c in self.classes_UFO or ():
            if any(w in c.lower() for w in _LESION_WORDS):
                raise ValueError('UFO classes should not contain tumor or lesion classes: report-supervised volumes are assumed to have no lesion '
                                 'annotated per voxel. Classes found:', self.classes_UFO)
        self.num_classes = len(self.classes)
        self.num_classes_UFO = len(self.classes_UFO) if self.classes_UFO is not None else 0
        self.lesion_classes = [i for i, c in enumerate(self.classes) if 'lesion' in c.lower()
                               and c.lower().replace('_lesion', '').replace('pancreatic', 'pancreas') in self.tumor_classes]
        if self.reports is not None:
            have = set(self.reports['BDMAP_ID'].values)
            missing = [i for i in ids if i not in have]
            if missing:
                raise ValueError(f'IDs not in reports: {missing}. Length of reports: {len(self.reports)}, number of missing ids: {len(missing)}')
        if UFO_only:           # a report volume whose id also occurs in the annotated root is left out (:357-373), and the other way round
            other = _ids_in(args.data_root)
            self._keep([i for i, p in enumerate(self.img_list) if not any(o in p for o in other)])
        if Atlas_only and ufo_root is not None:
            other = _ids_in(ufo_root)
            self._keep([i for i, p in enumerate(self.img_list) if not any(o in p for o in other)])
        _log(f'Number of images in {self.mode} set:', len(self.img_list))

    def _keep(self, idx):
        # the reference filters img_list alone (:373, :390) and leaves lab_list misaligned; here the lists stay aligned
        for name in ('img_list', 'lab_list', 'spacing_list'):
            setattr(self, name, [getattr(self, name)[i] for i in idx])

    def is_ufo(self, idx):
        return self.img_list[idx % len(self.img_list)] in self._ufo

    def case_id(self, idx):
        p = self.img_list[idx]
        k = p.find('BDMAP_')
        return p[k:k + ID_LEN]

    def read_report(self, idx):
        """The report rows of a case (:394-403); a case without rows is an error."""
        i = self.case_id(idx)
        if self.reports is None or i not in self.reports['BDMAP_ID'].values:
            raise ValueError('ID is not in the reports:', i, 'Length of reports:', 0 if self.reports is None else len(self.reports))
        return self.reports[self.reports['BDMAP_ID'] == i]

    def __len__(self):
        return len(self.img_list)

    def _read(self, idx):
        img, lab = load_array(self.img_list[idx]), load_array(self.lab_list[idx])
        if data.get_worker_info() is not None:       # a worker hands tensors over (shared memory), never a pickled copy of a memory map
            img, lab = torch.from_numpy(np.array(img)), torch.from_numpy(np.array(lab))
        ufo = self.img_list[idx] in self._ufo
        out = {'image': img, 'label': lab, 'path': self.img_list[idx], 'lab_path': self.lab_list[idx], 'is_ufo': ufo,
               'report': self.read_report(idx) if ufo else None}
        if self.mode == 'test':
            out['spacing'] = np.array(self.spacing_list[idx])
        return out

    def __getitem__(self, idx):
        idx = idx % len(self.img_list)
        try:
            return self._read(idx)
        except Exception:
            # a file that cannot be read: another case, drawn from numpy's global generator, once (:423-431)
            _log('Error loading:', self.img_list[idx], self.lab_list[idx])
            idx = int(np.random.randint(len(self.img_list)))
            try:
                return self._read(idx)
            except Exception as e:
                raise ValueError('Error loading:', self.img_list[idx], self.lab_list[idx]) from e


def collate_volumes(samples):
    """Volumes differ in size: a batch is the list of its samples."""
    return list(samples)


class WholeVolumeLoader:
    """DataLoader over a WholeVolumeDataset + DeviceCropper -> the device batch dictionary train_step takes (what ingest_packed_batch(keep_packed=True)
    yields).  Per volume: upload_label, the image through a pinned buffer, DeviceCropper.crop_one; per batch the two sum checks of SanityAssertOutput
    from PackedBits.class_flags().

    prefetch: software pipelining on the training thread, no Python threads.  `prefetch_next()` -- called by the training loop once the step for batch
    n has been queued -- queues the work for batch n + 1 on a side stream; the batch is handed over with an event, and `record_stream` on the tensors
    that cross.  A consumer that never calls prefetch_next() gets the same batches (the work is then queued when the next batch is asked for).
    prefetch=False does the same work on the current stream.  Every draw of the global generators happens in sample order in `_produce`, so both
    settings give the same bytes.

    The class totals of an annotated volume are kept on the host per path after its first visit: a revisit's draws need no device-to-host read.
    crops_per_visit=K cuts K crops from each uploaded volume with K consecutive sets of draws (a batch then holds batch_size * K samples).
    mode='test' datasets yield (image (1, 1, D, H, W), label (1, C, D, H, W) uint8, spacing (1, 3)) for training/validation.py."""

    def __init__(self, dataset, batch_size=1, sampler=None, num_workers=0, prefetch=True, crops_per_visit=1, device='cuda', chunk_bytes=None,
                 scale=None, rotate=None, translate=None):
        from .whole_volume import DeviceCropper
        from . import packed as _packed
        self.dataset, self.batch_size = dataset, int(batch_size)
        self.prefetch, self.crops_per_visit = bool(prefetch), int(crops_per_visit)
        self.device = torch.device(device)
        if self.device.type == 'cuda' and self.device.index is None:
            self.device = torch.device('cuda', torch.cuda.current_device())
        self.chunk_bytes = _packed.UPLOAD_CHUNK_BYTES if chunk_bytes is None else int(chunk_bytes)
        nw = min(int(num_workers), MAX_WORKERS)
        # with workers the volumes arrive as tensors and torch's own pinning thread page-locks them: the training thread then only queues the copies
        self.loader = data.DataLoader(dataset, batch_size=self.batch_size, shuffle=False, sampler=sampler, num_workers=nw, collate_fn=collate_volumes,
                                      persistent_workers=nw > 0, pin_memory=nw > 0)
        a = dataset.args
        self.cropper = None
        if dataset.mode == 'train':
            kw = dict(scale=getattr(a, 'scale', 0.3) if scale is None else scale, rotate=getattr(a, 'rotate', 45) if rotate is None else rotate,
                      translate=getattr(a, 'translate', 0.1) if translate is None else translate)
            self.cropper = DeviceCropper(a.training_size, dataset.classes, dataset.lesion_classes, dataset.tumor_class_names,
                                         crop_on_tumor=dataset.crop_on_tumor, device=self.device, classes_ufo=dataset.classes_UFO, **kw)
        missing = set(dataset.classes) - set(dataset.classes_UFO or dataset.classes) - {'liver', 'pancreas'}
        self.known = [i for i, c in enumerate(dataset.classes) if not ('lesion' in c.lower() or c in missing)]
        self.totals = {}              # path -> host class totals of the annotated volume
        self.last_meta, self.last_items = [], []
        self._side = torch.cuda.Stream(device=self.device) if self.prefetch else None
        self._it, self._pending = None, None

    def __len__(self):
        return len(self.loader)

    # ---- one volume ---------------------------------------------------------------------------------------------------------------------------
    def upload(self, item):
        """-> (image (D, H, W) device tensor, label PackedBits (1, P, D, H, W)) on the current stream."""
        from .packed import upload_label
        img = item['image']
        if isinstance(img, torch.Tensor) and img.is_pinned():
            pin = img
        else:
            img = img.numpy() if isinstance(img, torch.Tensor) else img
            pin = torch.empty(img.shape, dtype=torch.from_numpy(np.empty(0, img.dtype)).dtype).pin_memory()
            np.copyto(pin.numpy(), img)
        C = self.dataset.num_classes_UFO if item['is_ufo'] else self.dataset.num_classes
        return pin.to(self.device, non_blocking=True), upload_label(item['label'], C, self.device, self.chunk_bytes)

    def _crops(self, item):
        from .. import augmentation
        img, lab = self.upload(item)
        out = []
        for _ in range(self.crops_per_visit):
            if item['is_ufo']:
                out.append(self.cropper.crop_one(img, lab, item['report'], report=True))
            else:
                counts = augmentation.class_counts(lab)
                if item['path'] in self.totals:
                    counts._host = [list(self.totals[item['path']])]
                out.append(self.cropper.crop_one(img, lab, counts=counts))
                self.totals[item['path']] = list(counts.host(0))
        return out

    def _produce(self, items):
        """Queue everything for one batch on the current stream -> (batch, items, meta, pinned check flags, event)."""
        if self.dataset.mode == 'test':
            from .packed import unpack_bits_device
            (item,) = items
            img, lab = self.upload(item)
            batch = (img.float()[None, None], unpack_bits_device(lab.packed, lab.C), torch.from_numpy(item['spacing'])[None])
            flags = None
        else:
            crops = [c for item in items for c in self._crops(item)]
            batch = self.cropper.assemble(crops)
            B, C = len(crops), len(self.dataset.classes)
            sums = torch.stack([batch[k].class_flags().view(B, C)[:, self.known].any() for k in ('unk_channels', 'mask')]).to(torch.uint8)
            flags = torch.empty(2, dtype=torch.uint8).pin_memory()
            flags.copy_(sums, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record()
        meta = list(self.cropper.last_meta) if self.cropper is not None else []
        return batch, [i for i in items for _ in range(self.crops_per_visit)], meta, flags, ev

    def _queue_next(self):
        try:
            items = next(self._it)
        except StopIteration:
            return None
        if not self.prefetch:
            return self._produce(items)
        self._side.wait_stream(torch.cuda.current_stream(self.device))
        with torch.cuda.stream(self._side):
            return self._produce(items)

    def prefetch_next(self):
        """Queue the next batch's work now (prefetch=True, inside an iteration, nothing queued yet); otherwise nothing happens."""
        if self.prefetch and self._it is not None and self._pending is None:
            self._pending = self._queue_next() or False

    def _hand_over(self, produced):
        batch, items, meta, flags, ev = produced
        cur = torch.cuda.current_stream(self.device)
        if self.prefetch:
            cur.wait_event(ev)
            tensors = batch.values() if isinstance(batch, dict) else batch
            for t in tensors:
                for u in (getattr(t, 'packed', t), getattr(t, '_flags', None)):      # a PackedBits: its bytes and the class flags computed above
                    if isinstance(u, torch.Tensor) and u.is_cuda:
                        u.record_stream(cur)
        if flags is not None:
            ev.synchronize()
            assert int(flags[0]) == 0, 'unknown voxels on a non-lesion class (SanityAssertOutput)'
            assert int(flags[1]) == 0, 'segment mask on a non-lesion class (SanityAssertOutput)'
        self.last_items, self.last_meta = items, meta
        return batch

    def __iter__(self):
        self._it, self._pending = iter(self.loader), None
        try:
            while True:
                produced = self._pending if self._pending is not None else (self._queue_next() or False)
                self._pending = None
                if produced is False:
                    return
                yield self._hand_over(produced)
        finally:
            self._it, self._pending = None, None
