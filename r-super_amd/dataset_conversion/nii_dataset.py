"""One AbdomenAtlas-style case -- a NIfTI CT plus one NIfTI mask per class, or one nnU-Net label map -- to the training case the whole-CT dataset
reads: the z-scored, padded float32 image and the bit-packed label.  The reference does this in two commands on SimpleITK:

    dataset_conversion/abdomenatlas_3d.py  ResampleImage :59-103: reorient image and labels to 'RAI', B-spline the image in x and y and nearest in z to
        1 mm, nearest-neighbour the labels onto it (two passes), write `.nii.gz`;
    dataset_conversion/nii2npz.py  process_file :32-86: clip to [-991, 500], (img - np.mean) / np.std, a missing `background` as 1 - sum of the other
        classes, pad every axis shorter than 128 by ceil((128 - n) / 2) on both sides, savez_compressed of the image and the unpacked int8 stack.

Here (csrc/nii_dataset.hip):

    image   load_nifti_device (inference/nifti_device.py: reorientation as a strided read, prefilter, B-spline resample) -> rsuper_ct_stats ->
            rsuper_ct_normalize_pop: the clip, the z-score with the POPULATION std (np.std, ddof = 0) and the pad in one write.
    label   every mask file's voxel buffer is uploaded as it lies in the file, eight classes at a time; one rsuper_label_gather_pack launch per group
            reads them through per-class strides (each mask may have its own voxel order) and the three per-axis nearest tables and writes one byte
            plane of the packed label, padding included.  The composite of the reference's two nearest passes is this single gather (a nearest pass
            along an axis that maps to itself is the identity).  No unpacked (C, D, H, W) volume exists on either side.  While the device works on a
            group a background thread reads and inflates the next group's files; the device holds one group's raw bytes plus the packed result.
            rsuper_label_background then makes a missing `background` the way the reference chain ends up with it: set where the number of other
            classes is not 1 -- no class (also in a stripe outside the scan) or an overlap (liver and liver_lesion) -- inside the resampled box only.
    label map   process_case_nnunet_format: one integer volume and a (n_values, P) byte table (build_lut); one launch writes all planes.

`torch.ops.rsuper.label_gather_pack / label_background / ct_normalize_pop` are the dispatcher entries (CUDA key only; a CPU tensor raises
RSuperHipError).  What is out of scope and what is unverified against ITK: INTEGRATION section 3i."""
import math
import os
from concurrent.futures import ThreadPoolExecutor
from dataclasses import dataclass

import numpy as np
import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library
from ..inference import nifti as _n
from ..inference import nifti_device as _nd
from ..inference import preprocess as _pp
from ..training.dataset.packed import PackedBits

CLIP = (-991.0, 500.0)                         # nii2npz.py :64
MIN_SIZE = 128                                 # nii2npz.py pad
GROUP = 8                                      # classes of a gather launch: one output byte plane
DESC_WORDS = 8                                 # RSUPER_LABEL_DESC_WORDS
_INT_NII = {2: (0, 1), 256: (1, 1), 4: (2, 2), 512: (3, 2), 8: (4, 4)}       # NIfTI-1 integer datatype -> (RSUPER_NII_* code, bytes per voxel)
_LAUNCHES = {'gather': 0, 'background': 0, 'normalize': 0}


def nii_dataset_launches():
    """Calls of the three entry points this process has made: {'gather', 'background', 'normalize'}."""
    return dict(_LAUNCHES)


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _need_device(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _l.RSuperHipError(f'{what} needs a device tensor (no CPU fallback)')


def _label_gather_pack_impl(raw, desc, nclass, lut, ix, iy, iz, src_size, dst, plane, offset):
    """raw: flat uint8 device buffer with the group's voxel buffers; desc (nclass, 8) int64 device; ix, iy, iz int32 device nearest tables of the
    resampled box; src_size (Z, Y, X) canonical; dst (P, Do, Ho, Wo) uint8 device, offset (zo, yo, xo) of the box in it.  lut None: byte plane
    `plane` of dst is written; lut (n_values, P) uint8: all P planes."""
    for t in (raw, desc, ix, iy, iz, dst) + (() if lut is None else (lut,)):
        _need_device(t, 'label_gather_pack')
    assert raw.dtype == torch.uint8 and raw.dim() == 1 and raw.is_contiguous()
    assert desc.dtype == torch.int64 and desc.is_contiguous() and tuple(desc.shape) == (nclass, DESC_WORDS)
    assert all(t.dtype == torch.int32 and t.dim() == 1 and t.is_contiguous() for t in (ix, iy, iz))
    assert dst.dtype == torch.uint8 and dst.dim() == 4 and dst.is_contiguous()
    P, Do, Ho, Wo = dst.shape
    V = Do * Ho * Wo
    if lut is None:
        assert 0 <= plane < P
        lut_ptr, n_values, planes, out_ptr = None, 0, 1, dst.data_ptr() + plane * V
    else:
        assert lut.dtype == torch.uint8 and lut.dim() == 2 and lut.is_contiguous() and lut.shape[1] == P and plane == 0
        lut_ptr, n_values, planes, out_ptr = lut.data_ptr(), lut.shape[0], P, dst.data_ptr()
    with torch.cuda.device(dst.device):
        _l.check(_l.lib().rsuper_label_gather_pack(raw.data_ptr(), raw.numel(), desc.data_ptr(), int(nclass), lut_ptr, n_values, planes, ix.data_ptr(),
                                                   iy.data_ptr(), iz.data_ptr(), int(src_size[0]), int(src_size[1]), int(src_size[2]), iz.numel(),
                                                   iy.numel(), ix.numel(), out_ptr, Do, Ho, Wo, int(offset[0]), int(offset[1]), int(offset[2]),
                                                   _stream(dst)), 'label_gather_pack')
    _LAUNCHES['gather'] += 1


def _label_background_impl(packed, bg_class, offset, box):
    """packed (P, Do, Ho, Wo) uint8 device: inside the box the bit of bg_class becomes (other classes at the voxel) != 1."""
    _need_device(packed, 'label_background')
    assert packed.dtype == torch.uint8 and packed.dim() == 4 and packed.is_contiguous()
    P, Do, Ho, Wo = packed.shape
    with torch.cuda.device(packed.device):
        _l.check(_l.lib().rsuper_label_background(packed.data_ptr(), P, int(bg_class), Do, Ho, Wo, int(offset[0]), int(offset[1]), int(offset[2]),
                                                  int(box[0]), int(box[1]), int(box[2]), _stream(packed)), 'label_background')
    _LAUNCHES['background'] += 1


def _ct_normalize_pop_impl(hu, lo, hi, out_shape, offset, workspace=None):
    """inference/preprocess.py's z-score with the population std: hu (D, H, W) int16 / float32 -> ((Do, Ho, Wo) float32, (mean, std))."""
    out = _pp._ct_normalize_impl(hu, lo, hi, out_shape, offset, workspace, pop=True)
    _LAUNCHES['normalize'] += 1
    return out


_OPS = _library.install_nii_dataset_ops(_label_gather_pack_impl, _label_background_impl, _ct_normalize_pop_impl)


@dataclass
class CaseGeometry:
    """nifti: the CT's NiftiGeometry; box (Zb, Yb, Xb): the resampled scan; offset (zo, yo, xo) of the box in the padded `shape` (Do, Ho, Wo);
    class_names: sorted, the order of the packed bits; mean_std: 2-element float32 device tensor of the clipped volume (population std)."""
    nifti: object
    box: tuple
    offset: tuple
    shape: tuple
    class_names: tuple
    mean_std: object


def pad_geometry(box, min_size=MIN_SIZE):
    """nii2npz.pad: every axis shorter than min_size gets ceil((min_size - n) / 2) voxels on BOTH sides (127 -> 129).  (padded shape, offset)."""
    d = [int(math.ceil((float(min_size) - n) / 2)) if n < min_size else 0 for n in box]
    return tuple(int(n) + 2 * k for n, k in zip(box, d)), tuple(d)


def nearest_tables(size, spacing, target_spacing):
    """The int32 nearest tables (x, y, z) of a canonical grid; the identity where the spacing equals the target (no resample runs there)."""
    if _nd.same_spacing(spacing, target_spacing):
        return tuple(np.arange(int(n), dtype=np.int32) for n in size)
    return tuple(_n.resample_axis_table(size[a], spacing[a], target_spacing[a], 'nearest') for a in range(3))


def build_lut(class_names, table):
    """The (n_values, P) uint8 table of label-map mode from {class name: value or list of values}: the byte of plane p that value v sets.  A joint
    class is several values with the same bit (liver = eight segments + hepatic vessel); a value may belong to several classes."""
    names = sorted(class_names)
    P = (len(names) + 7) // 8
    values = {n: ([int(v) for v in table[n]] if isinstance(table[n], (list, tuple)) else [int(table[n])]) for n in names}
    flat = [v for vs in values.values() for v in vs]
    if not flat or min(flat) < 0:
        raise ValueError('build_lut: every class needs at least one non-negative value')
    lut = np.zeros((max(flat) + 1, P), dtype=np.uint8)
    for c, n in enumerate(names):
        for v in values[n]:
            lut[v, c >> 3] |= 0x80 >> (c & 7)
    return lut


def _read_mask(path, ct_size):
    """(flat voxel buffer, descriptor words without the element offset) of an integer mask whose canonical size equals the CT's."""
    vol = _n.read_nifti(path)
    if vol.datatype not in _INT_NII:
        raise ValueError(f'{path}: a mask must hold integers (uint8, int8, int16, uint16, int32), this file has NIfTI datatype {vol.datatype}')
    perm, flip = _n.orientation_plan(_n.affine(vol))
    size, stride, offset, _ = _n.canonical_layout(vol.shape, perm, flip)
    if tuple(size) != tuple(ct_size):
        raise ValueError(f'{path}: the mask is {tuple(size)} voxels (x, y, z) after reorientation, the CT is {tuple(ct_size)}')
    code, esz = _INT_NII[vol.datatype]
    return vol.data.reshape(-1).view(np.uint8), [code, stride[2], stride[1], stride[0], offset, vol.data.size, 0], esz


def _load_group(paths, ct_size):
    """The masks of one group (None = absent) -> (raw uint8 host buffer, (n, 8) int64 descriptors).  Runs in the reader thread."""
    bufs, desc, pos = [], [], 0
    for p in paths:
        if p is None:
            desc.append([0, 0, 0, 0, 0, 0, 0, 1])
            continue
        data, words, esz = _read_mask(p, ct_size)
        desc.append([pos // esz] + words)
        bufs.append(data)
        pos += (data.size + 3) // 4 * 4                  # every buffer starts 4-byte aligned
    raw = np.zeros(max(pos, 4), dtype=np.uint8)
    pos = 0
    for b in bufs:
        raw[pos:pos + b.size] = b
        pos += (b.size + 3) // 4 * 4
    return raw, np.asarray(desc, dtype=np.int64).reshape(len(paths), DESC_WORDS)


def convert_case(ct_path, mask_paths_or_label_map, class_names, target_spacing=(1., 1., 1.), min_size=MIN_SIZE, lut=None, device='cuda', reader=None):
    """One case -> (image (Z, Y, X) float32 device tensor, PackedBits (1, P, Z, Y, X), CaseGeometry).

    ct_path: a `.nii` / `.nii.gz` CT (or a NiftiVolume).  mask_paths_or_label_map: {class name: path, or None for a missing file} -- a missing mask
    is a zero plane, a missing `background` is synthesised -- or, with lut, the path of one integer label map.  class_names are sorted, as
    process_file does; the bit of class c is bit 7 - (c & 7) of byte plane c >> 3.  lut: (n_values, P) uint8 from build_lut.  reader: a
    ThreadPoolExecutor that reads the mask files (one is made if None).  ValueError, naming the file, for a float mask and for a mask whose
    canonical size differs from the CT's."""
    dev = torch.device(device)
    if dev.type != 'cuda':
        raise _l.RSuperHipError('convert_case needs a device (no CPU fallback)')
    names = tuple(sorted(class_names))
    C = len(names)
    P = (C + 7) // 8
    if C < 1 or P > 8:
        raise ValueError(f'convert_case: {C} classes (1 .. 64)')
    own = reader is None
    reader = ThreadPoolExecutor(max_workers=1) if own else reader
    try:
        ct = ct_path if isinstance(ct_path, _n.NiftiVolume) else _n.read_nifti(ct_path)
        geom = _nd.geometry_of(ct)
        if lut is None:
            paths = [mask_paths_or_label_map.get(n) for n in names]
            groups = [paths[g:g + GROUP] for g in range(0, C, GROUP)]
        else:
            lut = np.ascontiguousarray(lut, dtype=np.uint8)
            if lut.ndim != 2 or lut.shape[1] != P:
                raise ValueError(f'convert_case: the lut must be (n_values, {P}) for {C} classes, got {lut.shape}')
            groups = [[mask_paths_or_label_map]]
        nxt = reader.submit(_load_group, groups[0], geom.size)          # the masks are read while the image is made
        hu, _ = _nd.load_nifti_device(ct, target_spacing, device=dev)
        box = tuple(int(v) for v in hu.shape)
        shape, offset = pad_geometry(box, min_size)
        image, ms = _OPS[2](hu, CLIP[0], CLIP[1], list(shape), list(offset), None)
        del hu
        ix, iy, iz = (torch.from_numpy(np.ascontiguousarray(t, dtype=np.int32)).to(dev) for t in nearest_tables(geom.size, geom.spacing, target_spacing))
        assert (iz.numel(), iy.numel(), ix.numel()) == box, 'the label tables and the resampled image disagree'
        packed = torch.empty((P,) + shape, device=dev, dtype=torch.uint8)
        src_size = [geom.size[2], geom.size[1], geom.size[0]]
        lut_dev = None if lut is None else torch.from_numpy(lut).to(dev)
        for g in range(len(groups)):
            raw, desc = nxt.result()
            if g + 1 < len(groups):
                nxt = reader.submit(_load_group, groups[g + 1], geom.size)
            raw_dev, desc_dev = torch.from_numpy(raw).to(dev), torch.from_numpy(desc).to(dev)
            _OPS[0](raw_dev, desc_dev, len(groups[g]), lut_dev, ix, iy, iz, src_size, packed, g, list(offset))
            del raw_dev, desc_dev                        # stream-ordered: the next group's upload may reuse the memory after this launch
        if lut is None and 'background' in names and mask_paths_or_label_map.get('background') is None:
            _OPS[1](packed, names.index('background'), list(offset), list(box))
    finally:
        if own:
            reader.shutdown(wait=True)
    return image, PackedBits(packed[None], C), CaseGeometry(geom, box, offset, shape, names, ms)


def find_ct(src_path, name):
    """<src>/<id>/ct.nii.gz, then <src>/<id>.nii.gz (process_case_bdmap_format :120-122); None if neither exists."""
    for p in (os.path.join(src_path, name, 'ct.nii.gz'), os.path.join(src_path, name + '.nii.gz')):
        if os.path.exists(p):
            return p
    return None


def find_masks(label_path, name, class_names, log=None):
    """{class: <label>/<id>/segmentations/<class>.nii.gz, else .../predictions/..., else None with a message} (:127-138)."""
    out = {}
    for c in class_names:
        p = os.path.join(label_path, name, 'segmentations', c + '.nii.gz')
        if not os.path.exists(p):
            p = os.path.join(label_path, name, 'predictions', c + '.nii.gz')
        if not os.path.exists(p):
            if log:
                log(f'File {p} does not exist')
            p = None
        out[c] = p
    return out
