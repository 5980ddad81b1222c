"""From a whole CT to the training crop on the device: the per-voxel-annotated branch of `AbdomenAtlasDataset.crop`
(rsuper_train/training/dataset/dim3/dataset_abdomenatlas_UFO.py:836-851), its `random_crop_on_tumor` wrapper (:580-631) and the padding of
`__getitem__` (:487), on the kernels of csrc/crop.hip (training/augmentation.py) -- the label stays bit-packed from the file to the loss.

`DeviceCropper` is called from the TRAINING process with the whole volumes a DataLoader worker read (image + np.packbits label, both still on
the host): device work inside workers would multiply the processes that hold the GPU.  It returns the batch dictionary
`ingest_packed_batch(keep_packed=True)` yields for per-voxel-annotated samples (:529-533).

Out of scope: the report-annotated branch of `crop()` (get_random_tumor_seg_mask, get_chosen_segment_mask, assign_labels,
define_unknown_voxels), crop_foreground_3d / denoise_mask, the 2-D variants and the np_* twins.
"""
import numpy as np
import torch

from .. import augmentation
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


def random_crop(tensor_img, tensor_lab, d, h, w, scale, rotate, translate):
    """`AbdomenAtlasDataset.random_crop` (:567-578): a random (d + 20, h + 40, w + 40) crop (the whole tensor where it is smaller: the reference's
    slice simply ends early), then spatial_augment_batch's branch -- affine + centre crop with probability 0.4, else a random plain crop."""
    size = tuple(tensor_img.shape[2:])
    big = [min(c, s) for c, s in zip(large_size(d, h, w), size)]
    org = augmentation.crop_offsets(size, large_size(d, h, w), 'random')
    if list(size) != big:
        tensor_img, (lab,), _ = augmentation.crop_box(tensor_img, (_bytes_of(tensor_lab),), big, origin=org)
    else:
        lab = _bytes_of(tensor_lab)
    if tensor_img.dtype != torch.float32:
        tensor_img = tensor_img.float()
    img, (lab,) = augmentation.spatial_augment_batch(tensor_img, (lab,), [d, h, w], scale, rotate, translate)
    return img, _kind_of(tensor_lab, lab)


def crop_annotated(tensor_img, tensor_lab, d, h, w, classes, lesion_classes, tumor_class_names, scale, rotate, translate, crop_on_tumor=True,
                   pad=None):
    """The per-voxel-annotated branch of `crop()` (:837-851): random_crop_on_tumor always runs (and consumes its draws); with crop_on_tumor off its
    RESULT then goes through random_crop, as the reference's fall-through does.  The reference also swallows any exception of the first call and
    falls back to random_crop of the uncropped volume; here an error is an error and propagates."""
    img, lab = random_crop_on_tumor(tensor_img, tensor_lab, d, h, w, classes, lesion_classes, tumor_class_names, scale, rotate, translate, pad=pad)
    if not crop_on_tumor:
        img, lab = random_crop(img, lab, d, h, w, scale, rotate, translate)
    return img, lab


class DeviceCropper:
    """Whole volumes -> one training batch, on the device.  __call__ takes a list of (image, packed_label): image a (D, H, W) float32 or int16 array /
    tensor, packed_label the (ceil(C / 8), D, H, W) uint8 np.packbits array of the label file; volumes may differ in size.  Per volume: upload,
    pad (virtually) to training_size + (20, 40, 40), crop_annotated.  Returns {'image' (B, 1, d, h, w) f32, 'label' PackedBits, 'unk_channels' and
    'mask' all-zero PackedBits, 'volumes' (B, 10) and 'diameters' (B, 10, 3) zeros}: what ingest_packed_batch(keep_packed=True) gives for
    per-voxel-annotated samples.  One device-to-host read per volume (the class totals the draws need)."""

    def __init__(self, training_size, classes, lesion_classes, tumor_class_names, scale=0.3, rotate=45, translate=0.1, crop_on_tumor=True,
                 device='cuda'):
        self.training_size = [int(s) for s in training_size]
        self.classes, self.lesion_classes, self.tumor_class_names = list(classes), [int(c) for c in lesion_classes], list(tumor_class_names)
        self.scale, self.rotate, self.translate, self.crop_on_tumor = scale, rotate, translate, crop_on_tumor
        self.device = torch.device(device)
        foreground_class_indices(self.tumor_class_names, self.classes)       # a name that is no class fails here, not in the first batch

    def crop_one(self, image, packed_label):
        C = len(self.classes)
        img = torch.as_tensor(image)
        lab = torch.as_tensor(packed_label)
        if img.dim() != 3 or img.dtype not in (torch.float32, torch.int16):
            raise ValueError('DeviceCropper: the image must be a float32 or int16 (D, H, W) volume, got %s %s' % (img.dtype, tuple(img.shape)))
        if lab.dim() != 4 or lab.dtype != torch.uint8 or tuple(lab.shape[1:]) != tuple(img.shape):
            raise ValueError('DeviceCropper: the label must be the uint8 (P, D, H, W) packbits array of the image grid')
        img = img.to(self.device, non_blocking=True)[None, None]
        lab = PackedBits(lab.to(self.device, non_blocking=True)[None], C)
        d, h, w = self.training_size
        return crop_annotated(img, lab, d, h, w, self.classes, self.lesion_classes, self.tumor_class_names, self.scale, self.rotate, self.translate,
                              crop_on_tumor=self.crop_on_tumor, pad=large_size(d, h, w))

    def __call__(self, volumes):
        if not volumes:
            raise ValueError('DeviceCropper: an empty batch')
        crops = [self.crop_one(image, label) for image, label in volumes]
        C, B = len(self.classes), len(crops)
        image = torch.cat([c[0] for c in crops], 0)
        label = torch.cat([c[1].packed for c in crops], 0)
        return {'image': image,
                'label': PackedBits(label, C),
                'unk_channels': PackedBits(torch.zeros_like(label), C),
                'mask': PackedBits(torch.zeros_like(label), C),
                'volumes': torch.zeros((B, MAX_TUMORS), device=self.device, dtype=torch.float32),
                'diameters': torch.zeros((B, MAX_TUMORS, 3), device=self.device, dtype=torch.float32)}
