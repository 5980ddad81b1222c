"""From a whole CT to the training crop on the device: the per-voxel-annotated branch of `AbdomenAtlasDataset.crop`
(rsuper_train/training/dataset/dim3/dataset_abdomenatlas_UFO.py:836-851), its `random_crop_on_tumor` wrapper (:580-631) and the padding of
`__getitem__` (:487), on the kernels of csrc/crop.hip (training/augmentation.py) -- the label stays bit-packed from the file to the loss.

`DeviceCropper` is called from the TRAINING process with the whole volumes a DataLoader worker read (image + np.packbits label, both still on
the host): device work inside workers would multiply the processes that hold the GPU.  It returns the batch dictionary
`ingest_packed_batch(keep_packed=True)` yields for per-voxel-annotated samples (:529-533).

The report-annotated branch of `crop()` (:852-934) is `crop_report`: the report decides the organ or sub-segment (dataset/reports.py), the
union of its classes is counted and boxed on the packed label (csrc/crop_report.hip), `augmentation.crop_foreground_3d` cuts the crop, and
`report_sample` (:523-527) turns the cropped classes_ufo label into the label, the unknown map and the chosen-segment mask of `classes` with one
rsuper_label_remap launch (`assign_labels` :1154, `get_chosen_segment_mask` :808) plus `estimate_tumor_volume`.  Device-to-host reads per report
volume: one for the chosen segment's count and box (two when the first segment is empty and a second is drawn), two more when the opening
runs, one for the crop's class totals -- 2 for a segment that fits at once, 4 with the opening.

Out of scope: define_unknown_voxels, the zero_masks.yaml side file, save() and SanityAssertOutput's dumps, the 2-D variants and the np_* twins.
"""
import numpy as np
import torch

from .. import augmentation
from . import reports
from .packed import PackedBits

MAX_TUMORS = 10
LARGE_MARGIN = (20, 40, 40)      # the large crop the affine branch cuts first: (d + 20, h + 40, w + 40) (:487, :612)


def foreground_class_names(tumor_class_names):
    """The organs a non-tumour crop may centre on (:585-596): every lesion class name mapped to its organ(s); a set in the reference, sorted here."""
    forg = []
    for c in tumor_class_names:
        if 'pancrea' in c:
            forg.append('pancreas')
        elif 'kidney' in c:
            forg.append('kidney_right')
            forg.append('kidney_left')
        elif 'gall' in c:
            forg.append('gall_bladder')
        else:
            forg.append(c)
    return sorted(set(forg))


def foreground_class_indices(tumor_class_names, classes):
    """forg as indices into `classes` (:604).  A name that is not a class raises ValueError, as list.index does in the reference."""
    return [list(classes).index(c) for c in foreground_class_names(tumor_class_names)]


def large_size(d, h, w):
    return [d + LARGE_MARGIN[0], h + LARGE_MARGIN[1], w + LARGE_MARGIN[2]]


def random_crop_on_tumor(tensor_img, tensor_lab, d, h, w, classes, lesion_classes, tumor_class_names, scale, rotate, translate, ufo=False,
                         tumor_case=None, pad=None, counts=None):
    """`AbdomenAtlasDataset.random_crop_on_tumor` (:580-631) on a device volume: forg from the lesion class names, tumor_case from the label's totals,
    then np.random.random() < 0.4 -> crop (d + 20, h + 40, w + 40) on the tumour, random affine, centre crop (one affine_center_crop launch);
    otherwise crop (d, h, w) on the tumour directly.  pad: the size `__getitem__` pads the volume to first (:487), applied without a padded copy."""
    forg = foreground_class_indices(tumor_class_names, classes)
    lesion_classes = [] if ufo else list(lesion_classes)
    if counts is None:
        counts = augmentation.class_counts(tensor_lab)
    if tumor_case is None:
        totals = counts.host(0)
        tumor_case = sum(totals[c] for c in lesion_classes) > 0
    if np.random.random() < 0.4:
        D, H, W = large_size(d, h, w)
        img, lab = augmentation.random_crop_on_tumor(tensor_img, tensor_lab, lesion_classes, D, H, W, tumor_case, foreground_classes=forg,
                                                     pad=pad, counts=counts)
        theta = augmentation.draw_affine_3d(scale, rotate, translate).unsqueeze(0)
        img, (lab,) = augmentation.affine_center_crop(img, (_bytes_of(lab),), theta, [d, h, w])
        return img, _kind_of(tensor_lab, lab)
    return augmentation.random_crop_on_tumor(tensor_img, tensor_lab, lesion_classes, d, h, w, tumor_case, foreground_classes=forg, pad=pad,
                                             counts=counts)


def _bytes_of(lab):
    return lab if hasattr(lab, 'packed') else augmentation._as_bytes(lab, 'lab')


def _kind_of(like, lab):
    return lab if hasattr(lab, 'packed') else lab.to(like.dtype)


def random_crop(tensor_img, tensor_lab, d, h, w, scale, rotate, translate, pad=None):
    """`AbdomenAtlasDataset.random_crop` (:567-578): a random (d + 20, h + 40, w + 40) crop (the whole tensor where it is smaller: the reference's
    slice simply ends early), then spatial_augment_batch's branch -- affine + centre crop with probability 0.4, else a random plain crop.
    pad: the volume counts as pad_volume_pair padded it (no padded copy is made)."""
    real = tuple(tensor_img.shape[2:])
    size = tuple(augmentation.padded_size(real, pad)[0])
    big = [min(c, s) for c, s in zip(large_size(d, h, w), size)]
    org = augmentation.crop_offsets(size, large_size(d, h, w), 'random')
    if list(real) != big:
        tensor_img, (lab,), _ = augmentation.crop_box(tensor_img, (_bytes_of(tensor_lab),), big, pad=size, origin=org)
    else:
        lab = _bytes_of(tensor_lab)
    if tensor_img.dtype != torch.float32:
        tensor_img = tensor_img.float()
    img, (lab,) = augmentation.spatial_augment_batch(tensor_img, (lab,), [d, h, w], scale, rotate, translate)
    return img, _kind_of(tensor_lab, lab)


def crop_annotated(tensor_img, tensor_lab, d, h, w, classes, lesion_classes, tumor_class_names, scale, rotate, translate, crop_on_tumor=True,
                   pad=None, counts=None):
    """The per-voxel-annotated branch of `crop()` (:837-851): random_crop_on_tumor always runs (and consumes its draws); with crop_on_tumor off its
    RESULT then goes through random_crop, as the reference's fall-through does.  The reference also swallows any exception of the first call and
    falls back to random_crop of the uncropped volume; here an error is an error and propagates."""
    img, lab = random_crop_on_tumor(tensor_img, tensor_lab, d, h, w, classes, lesion_classes, tumor_class_names, scale, rotate, translate, pad=pad,
                                    counts=counts)
    if not crop_on_tumor:
        img, lab = random_crop(img, lab, d, h, w, scale, rotate, translate)
    return img, lab


def crop_report(tensor_img, tensor_lab, report_rows, d, h, w, classes_ufo, tumor_class_names, scale, rotate, translate, pad=None):
    """The report-annotated branch of `crop()` (:852-934) on a device volume (1, 1, D, H, W) and its classes_ufo PackedBits label: the segment the
    report lets the crop be taken on (reports.plan_report_crop), its mask as a class set of the label, crop_foreground_3d around it; the 0.1 gate
    goes to random_crop and every dead end to random_crop_on_tumor(tumor_case=False, ufo=True).  -> (image crop, label crop, the selected tumour
    segment or 'random')."""
    classes_ufo = list(classes_ufo)
    plan = reports.plan_report_crop(reports.get_tumor_segment_labels(report_rows))
    known, out = {}, None
    while plan.action not in plan.FINAL:
        cset = reports.segment_class_set(plan.tumor_segment, classes_ufo)
        if plan.action == 'mask':
            known[cset], = augmentation._read_count_box(augmentation.union_bbox(tensor_lab, [cset]))
            plan.feed(known[cset][0])
        else:
            out = augmentation.crop_foreground_3d(tensor_img, tensor_lab, cset, [d, h, w], pad=pad, count_box=known.get(cset))
            plan.feed(True if isinstance(out, tuple) else out)
    if plan.action == 'done':
        return out[0], out[1], plan.tumor_segment
    if plan.action == 'random_crop':
        img, lab = random_crop(tensor_img, tensor_lab, d, h, w, scale, rotate, translate, pad=pad)
    else:
        img, lab = random_crop_on_tumor(tensor_img, tensor_lab, d, h, w, classes_ufo, [], tumor_class_names, scale, rotate, translate, ufo=True,
                                        tumor_case=False, pad=pad)
    return img, lab, plan.tumor_segment


def _present(lab, counts=None):
    """The per-class voxel totals of a (1, C, ...) label: the one device-to-host read the tables of a report sample need."""
    return (augmentation.class_counts(lab) if counts is None else counts).host(0)[:lab.C]


def assign_labels(tensor_lab, report_rows, classes, classes_ufo, present=None):
    """assign_labels (:1154-1298) on the cropped classes_ufo PackedBits -> (label PackedBits of `classes`, unk_channels dict, unknown-map PackedBits)."""
    present = _present(tensor_lab) if present is None else present
    ml, ol, mu, ou, unk = reports.assign_labels_tables(classes, classes_ufo, report_rows, present)
    label, unk_map = augmentation.label_remap(tensor_lab, len(classes), [[ml, mu]], [[ol, ou]])
    return label, unk, unk_map


def get_chosen_segment_mask(tensor_lab, tumor_segment, classes, classes_ufo=None, present=None):
    """get_chosen_segment_mask (:808-833) on the assigned label (PackedBits of `classes`) -> PackedBits: the segment's mask in the lesion channels it
    belongs to; 'random' -> all zero.  An empty segment mask is the reference's AssertionError."""
    cset, masks = reports.chosen_segment_table(classes, tumor_segment, classes_ufo)
    if tumor_segment != reports.RANDOM:
        present = _present(tensor_lab) if present is None else present
        assert any(present[c] > 0 for c in reports._bits(cset)), 'segment_mask is empty, crop is in %s' % (tumor_segment,)
    return augmentation.label_remap(tensor_lab, len(classes), [[masks]], [[0]])[0]


def report_sample(tensor_img, tensor_lab, report_rows, d, h, w, classes, classes_ufo, tumor_class_names, scale, rotate, translate, pad=None):
    """One report-annotated volume -> its training sample (`__getitem__` :489 and :523-527): crop_report, then assign_labels,
    estimate_tumor_volume and get_chosen_segment_mask.  The three volumes come from ONE label_remap launch on the cropped classes_ufo label: the
    chosen-segment table, written over the assigned label's classes, is composed with assign_labels' table.  -> {'image', 'label',
    'unk_channels', 'mask' (PackedBits of `classes`), 'volumes' (10,), 'diameters' (10, 3), 'tumor_in_crop', 'unknown_per_voxel', 'volumes_host' (estimate_tumor_volume's list, as save() writes it)}."""
    from .augmented import estimate_tumor_volume
    classes, classes_ufo = list(classes), list(classes_ufo)
    img, lab, selected = crop_report(tensor_img, tensor_lab, report_rows, d, h, w, classes_ufo, tumor_class_names, scale, rotate, translate, pad)
    present = _present(lab)
    ml, ol, mu, ou, unk = reports.assign_labels_tables(classes, classes_ufo, report_rows, present)
    volumes, diameters = estimate_tumor_volume(report_rows, selected)
    cset, chosen = reports.chosen_segment_table(classes, selected, classes_ufo)
    if selected != reports.RANDOM:                                # the assigned label's totals follow from the crop's: class j is there if a class it ORs is
        assert any(present[c] > 0 for j in reports._bits(cset) for c in reports._bits(ml[j])), 'segment_mask is empty, crop is in %s' % (selected,)
    mc = [0] * len(classes)
    for j, m in enumerate(chosen):
        for c in reports._bits(m):
            mc[j] |= ml[c]
    label, unk_map, mask = augmentation.label_remap(lab, len(classes), [[ml, mu, mc]], [[ol, ou, 0]])
    return {'image': img, 'label': label, 'unk_channels': unk_map, 'mask': mask,
            'volumes': torch.tensor(volumes).float().to(img.device), 'diameters': diameters.float().to(img.device),
            'tumor_in_crop': selected, 'unknown_per_voxel': unk, 'volumes_host': list(volumes)}


class DeviceCropper:
    """Whole volumes -> one training batch, on the device.  __call__ takes a list of (image, packed_label): image a (D, H, W) float32 or int16 array /
    tensor, packed_label the (ceil(C / 8), D, H, W) uint8 np.packbits array of the label file; volumes may differ in size.  Per volume: upload,
    pad (virtually) to training_size + (20, 40, 40), crop_annotated.  Returns {'image' (B, 1, d, h, w) f32, 'label' PackedBits, 'unk_channels' and
    'mask' all-zero PackedBits, 'volumes' (B, 10) and 'diameters' (B, 10, 3) zeros}: what ingest_packed_batch(keep_packed=True) gives for
    per-voxel-annotated samples.  One device-to-host read per volume (the class totals the draws need).

    A report-annotated volume is a triple (image, packed_label, report_rows): its label is the packbits array of `classes_ufo` (constructor
    argument) and report_rows the case's rows (a DataFrame, a list of mappings, or None for a case without tumour rows).  It goes through
    report_sample, and its rows of 'unk_channels', 'mask', 'volumes' and 'diameters' are real.  Pairs and triples may share a batch; a pair
    behaves exactly as without classes_ufo.  `last_meta` keeps each sample's 'tumor_in_crop' and 'unknown_per_voxel' (None for pairs)."""

    def __init__(self, training_size, classes, lesion_classes, tumor_class_names, scale=0.3, rotate=45, translate=0.1, crop_on_tumor=True,
                 device='cuda', classes_ufo=None):
        self.classes_ufo = None if classes_ufo is None else list(classes_ufo)
        self.last_meta = []
        self.training_size = [int(s) for s in training_size]
        self.classes, self.lesion_classes, self.tumor_class_names = list(classes), [int(c) for c in lesion_classes], list(tumor_class_names)
        self.scale, self.rotate, self.translate, self.crop_on_tumor = scale, rotate, translate, crop_on_tumor
        self.device = torch.device(device)
        foreground_class_indices(self.tumor_class_names, self.classes)       # a name that is no class fails here, not in the first batch

    def crop_one(self, image, packed_label, report_rows=None, report=False, counts=None):
        """One volume -> its crop.  image / packed_label may already be on the device (the whole-CT loader uploads them itself: packed_label is then a
        (P, D, H, W) uint8 device tensor or a one-sample PackedBits).  counts: the LabelCounts of an annotated volume when the caller has them."""
        if report and self.classes_ufo is None:
            raise ValueError('DeviceCropper: a report-annotated volume needs classes_ufo')
        C = len(self.classes_ufo) if report else len(self.classes)
        img = torch.as_tensor(image)
        lab = packed_label.packed[0] if isinstance(packed_label, PackedBits) else torch.as_tensor(packed_label)
        if img.dim() != 3 or img.dtype not in (torch.float32, torch.int16):
            raise ValueError('DeviceCropper: the image must be a float32 or int16 (D, H, W) volume, got %s %s' % (img.dtype, tuple(img.shape)))
        if lab.dim() != 4 or lab.dtype != torch.uint8 or tuple(lab.shape[1:]) != tuple(img.shape):
            raise ValueError('DeviceCropper: the label must be the uint8 (P, D, H, W) packbits array of the image grid')
        img = img.to(self.device, non_blocking=True)[None, None]
        lab = packed_label if isinstance(packed_label, PackedBits) else PackedBits(lab.to(self.device, non_blocking=True)[None], C)
        assert lab.C == C, 'the label has %d classes, expected %d' % (lab.C, C)
        d, h, w = self.training_size
        if report:
            return report_sample(img, lab, report_rows, d, h, w, self.classes, self.classes_ufo, self.tumor_class_names, self.scale, self.rotate,
                                 self.translate, pad=large_size(d, h, w))
        return crop_annotated(img, lab, d, h, w, self.classes, self.lesion_classes, self.tumor_class_names, self.scale, self.rotate, self.translate,
                              crop_on_tumor=self.crop_on_tumor, pad=large_size(d, h, w), counts=counts)

    def __call__(self, volumes):
        if not volumes:
            raise ValueError('DeviceCropper: an empty batch')
        return self.assemble([self.crop_one(*v, report=True) if len(v) == 3 else self.crop_one(*v) for v in volumes])

    def assemble(self, crops):
        """The crops of crop_one (pairs of annotated volumes, dictionaries of report volumes) -> the batch dictionary."""
        C, B = len(self.classes), len(crops)
        self.last_meta = [{k: c[k] for k in ('tumor_in_crop', 'unknown_per_voxel', 'volumes_host') if k in c} if isinstance(c, dict) else None for c in crops]
        image = torch.cat([c['image'] if isinstance(c, dict) else c[0] for c in crops], 0)
        label = torch.cat([c['label'].packed if isinstance(c, dict) else c[1].packed for c in crops], 0)
        batch = {'image': image,
                 'label': PackedBits(label, C),
                 'unk_channels': PackedBits(torch.zeros_like(label), C),
                 'mask': PackedBits(torch.zeros_like(label), C),
                 'volumes': torch.zeros((B, MAX_TUMORS), device=self.device, dtype=torch.float32),
                 'diameters': torch.zeros((B, MAX_TUMORS, 3), device=self.device, dtype=torch.float32)}
        for b, c in enumerate(crops):
            if isinstance(c, dict):
                batch['unk_channels'].packed[b], batch['mask'].packed[b] = c['unk_channels'].packed[0], c['mask'].packed[0]
                batch['volumes'][b], batch['diameters'][b] = c['volumes'], c['diameters']
        return batch
