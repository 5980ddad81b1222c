"""numpy restatement of the reference's dataset conversion chain for the tests of dataset_conversion/nii_dataset.py: what
dataset_conversion/abdomenatlas_3d.py (reorient to 'RAI', nearest-neighbour the labels onto the resampled image) followed by
dataset_conversion/nii2npz.py process_file (stack, a missing `background` as 1 - sum, clip / np.mean / np.std, pad) and the dataset's
astype(bool) + np.packbits(axis=0) leave of a case.  It imports nothing of the product; orientation and the nearest tables come from tests/nifti_ref.py.

A mask is (arr_ijk, perm, flip) -- the array as the file holds it and its orientation -- or None for a missing file.  A mask voxel counts as set when
it is not zero (the product's rule; the reference's astype(np.int8) differs only for non-zero multiples of 256)."""
import math

import numpy as np

import nifti_ref as nr

CLIP = (-991.0, 500.0)


def canonical_grid(shape_ijk, perm, pixdim):
    """((X, Y, Z), (sx, sy, sz)) of a file: canonical axis w is voxel axis perm.index(w)."""
    inv = [perm.index(w) for w in range(3)]
    return tuple(int(shape_ijk[a]) for a in inv), tuple(float(pixdim[a]) for a in inv)


def pad_widths(shape, min_size=128):
    """nii2npz.pad: ceil((min_size - n) / 2) on both sides of every axis shorter than min_size."""
    return [int(math.ceil((float(min_size) - n) / 2)) if n < min_size else 0 for n in shape]


def pad(img, lab, min_size=128):
    d = pad_widths(img.shape, min_size)
    return np.pad(img, [(k, k) for k in d]), np.pad(lab, [(0, 0)] + [(k, k) for k in d])


def gather_nearest(canon_zyx, size_xyz, spacing_xyz, target_xyz):
    """The composite of the two ResampleLabelToRef passes: out[z, y, x] = in[iz[z], iy[y], ix[x]], 0 where an axis is outside the scan."""
    ix, iy, iz = (nr.nearest_table(size_xyz[a], spacing_xyz[a], target_xyz[a]) for a in range(3))
    out = canon_zyx[np.maximum(iz, 0)][:, np.maximum(iy, 0)][:, :, np.maximum(ix, 0)].copy()
    out[iz < 0] = 0
    out[:, iy < 0] = 0
    out[:, :, ix < 0] = 0
    return out


def label_stack(class_names, masks, ct_size_xyz, ct_spacing_xyz, target_xyz=(1.0, 1.0, 1.0)):
    """The (C, Zb, Yb, Xb) int8 stack of process_file for sorted(class_names): masks {name: (arr_ijk, perm, flip) or None}.  A missing mask is a zero
    label (abdomenatlas_3d.py :131-137); a missing `background` is 1 - sum of the others (nii2npz.py :58-60), which is NOT 0 / 1 on an overlap."""
    names = sorted(class_names)
    box = tuple(nr.out_size(ct_size_xyz[a], ct_spacing_xyz[a], target_xyz[a]) for a in (2, 1, 0))
    lab, create_bkg, bkg_index = [], False, None
    for i, n in enumerate(names):
        m = masks.get(n)
        if n == 'background' and m is None:
            create_bkg, bkg_index = True, i
            continue
        if m is None:
            lab.append(np.zeros(box, np.int8))
            continue
        canon = (nr.reorient(m[0], m[1], m[2]) != 0).astype(np.int8)
        assert canon.shape == tuple(ct_size_xyz[::-1]), 'size mismatch'
        lab.append(gather_nearest(canon, ct_size_xyz, ct_spacing_xyz, target_xyz))
    lab = np.stack(lab, axis=0) if lab else np.zeros((0,) + box, np.int8)
    if create_bkg:
        background = 1 - np.sum(lab, axis=0)
        lab = np.insert(lab, bkg_index, background, axis=0)
    return lab


def label_map_stack(class_names, table, label_map_canon, ct_size_xyz, ct_spacing_xyz, target_xyz=(1.0, 1.0, 1.0)):
    """process_case_nnunet_format: class = (map == value), a joint class the union over its values; then the nearest gather."""
    lab = []
    for n in sorted(class_names):
        v = table[n]
        m = np.isin(label_map_canon, v if isinstance(v, list) else [v]).astype(np.int8)
        lab.append(gather_nearest(m, ct_size_xyz, ct_spacing_xyz, target_xyz))
    return np.stack(lab, axis=0)


def packed_labels(lab, min_size=128):
    """pad, astype(bool), packbits(axis=0): (P, Do, Ho, Wo) uint8."""
    _, lab = pad(np.zeros(lab.shape[1:], np.float32), lab, min_size)
    return np.packbits(lab.astype(bool), axis=0)


def zscore(img_zyx, min_size=128, ddof=0):
    """clip, (img - mean) / std in float64, pad: the float64 (Do, Ho, Wo) image."""
    x = np.clip(np.asarray(img_zyx, dtype=np.float64), CLIP[0], CLIP[1])
    x = (x - x.mean()) / x.std(ddof=ddof)
    d = pad_widths(x.shape, min_size)
    return np.pad(x, [(k, k) for k in d])

