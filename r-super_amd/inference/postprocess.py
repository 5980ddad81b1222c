"""Prediction post-processing of rsuper_train/predict_abdomenatlas.py on the MI355X path: prediction (:180-246), postprocess_npz (:637-690) and
keep_largest_component (:692-716) under the reference's names, on device tensors.

The reference copies the summed (classes, D, H, W) probabilities to the host, masks every lesion plane with its dilated organ in scipy and keeps
the largest component in SimpleITK.  Here the volumes stay on the device: the organ masking of all lesion planes of a case is one
`rsuper_organ_mask_*` launch, the component selection a union-find on the device (`rsuper_largest_component`).  Both are dispatcher ops
(`torch.ops.rsuper.organ_mask`, `torch.ops.rsuper.largest_component`, registered in hip/library.py).
"""
import ctypes
import math

import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library
from .detection import _detection_volumes_impl, _detection_binary_impl
from .inference3d import inference_sliding_window

Z_LEN = 800          # prediction(): cases deeper than this are inferred in independent depth chunks (:190-194)


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _ints(v):
    return (ctypes.c_int * max(1, len(v)))(*v)


def _organ_mask_impl(pred, lesion, organ_a, organ_b):
    """pred (C, D, H, W) uint8 or float32 -> (len(lesion), D, H, W): pred[lesion[k]] * box3_dilate(organ > 0.5), organ = pred[organ_a[k]]
    (+ pred[organ_b[k]] when organ_b[k] >= 0)."""
    assert pred.is_cuda and pred.dim() == 4 and pred.dtype in (torch.uint8, torch.float32), 'organ_mask: (C, D, H, W) uint8 / float32 on the device'
    assert len(lesion) == len(organ_a) == len(organ_b) and len(lesion) > 0
    pred = pred.contiguous()
    C, D, H, W = pred.shape
    out = torch.empty((len(lesion), D, H, W), device=pred.device, dtype=pred.dtype)
    fn = _l.lib().rsuper_organ_mask_u8 if pred.dtype == torch.uint8 else _l.lib().rsuper_organ_mask_f32
    _l.check(fn(pred.data_ptr(), C, D, H, W, len(lesion), _ints(lesion), _ints(organ_a), _ints(organ_b), out.data_ptr(), _stream(pred)),
             'organ_mask')
    return out


def largest_component_workspace(shape, device):
    D, H, W = shape
    return torch.empty((_l.lib().rsuper_largest_component_workspace_bytes(D, H, W),), device=device, dtype=torch.uint8)


def _largest_component_impl(mask, workspace=None):
    """mask (D, H, W) uint8 / bool / float32 -> uint8 0/1 volume of the largest 6-connected component of mask > 0 (all ones when empty)."""
    assert mask.is_cuda and mask.dim() == 3, 'largest_component: a (D, H, W) volume on the device'
    if mask.dtype == torch.bool:
        mask = mask.view(torch.uint8)
    assert mask.dtype in (torch.uint8, torch.float32), f'largest_component: uint8 / bool / float32 mask, got {mask.dtype}'
    mask = mask.contiguous()
    D, H, W = mask.shape
    ws = largest_component_workspace((D, H, W), mask.device) if workspace is None else workspace
    assert ws.is_cuda and ws.numel() * ws.element_size() >= _l.lib().rsuper_largest_component_workspace_bytes(D, H, W)
    out = torch.empty((D, H, W), device=mask.device, dtype=torch.uint8)
    _l.check(_l.lib().rsuper_largest_component(mask.data_ptr(), 1 if mask.dtype == torch.uint8 else 0, D, H, W, out.data_ptr(), ws.data_ptr(),
                                               _stream(mask)), 'largest_component')
    return out


def keep_largest_component(mask, workspace=None):
    """keep_largest_component (:692-716): uint8 volume, 1 on the largest face-connected component of `mask > 0`.  Ties go to the component
    whose first voxel comes first in C order (the label order of SimpleITK's ConnectedComponentImageFilter, and the reference keeps the first
    label of the largest size).  An empty mask gives all ones, as in the reference (its `Equal(cc, 0)` with label 0 left over)."""
    return torch.ops.rsuper.largest_component(mask, workspace)


def organ_name(lesion_class):
    """The organ of a lesion class in postprocess_npz (:658): first '_' field, 'pancreatic' -> 'pancreas'."""
    return lesion_class.split('_')[0].replace('pancreatic', 'pancreas')


def organ_planes(lesion_class, organs):
    """Organ planes masking `lesion_class` (:659-686): a list of one or two names of `organs` (the non-lesion classes), or None for the
    all-ones mask of bone / breast.  A missing organ raises KeyError, as the reference's dict lookup does."""
    name = organ_name(lesion_class)
    pairs = {'kidney': ['kidney_right', 'kidney_left'], 'adrenal': ['adrenal_gland_right', 'adrenal_gland_left'],
             'lung': ['lung_right', 'lung_left'], 'uterus': ['prostate'], 'gallbladder': ['gall_bladder']}
    if name in ('bone', 'breast'):
        if 'prostate' not in organs:          # np.ones_like(pred_dict['prostate'])
            raise KeyError('prostate')
        return None
    planes = pairs.get(name, [name])
    for p in planes:
        if p not in organs:
            raise KeyError(p)
    return planes


def postprocess_npz(pred, classes, args):
    """postprocess_npz (:637-690) on the device: pred (1, C, D, H, W) or (C, D, H, W), uint8 labels or float32 probabilities; returns
    {class name: (D, H, W) device tensor}, organs first, then lesions, in class order.  args.organ_mask_on_lesion multiplies every lesion plane
    by its dilated organ mask (one launch for all of them); args.connected_components (off by default, as in the reference's npz path)
    then keeps the largest component of each lesion plane -- the nii path's order (:503-504) -- which makes those planes uint8 0/1."""
    if pred.dim() == 5:
        pred = pred.squeeze(0)
    assert pred.dim() == 4 and pred.shape[0] == len(classes), f'postprocess_npz: {tuple(pred.shape)} for {len(classes)} classes'
    if not pred.is_cuda:
        raise _l.RSuperHipError('postprocess_npz: the prediction must be on the MI355X device (no CPU fallback)')
    out = {}
    organ_idx = {}
    for i, name in enumerate(classes):
        if 'lesion' not in name:
            out[name] = pred[i]
            organ_idx[name] = i
    lesions = [(i, name) for i, name in enumerate(classes) if 'lesion' in name]
    planes = {name: pred[i] for i, name in lesions}
    if getattr(args, 'organ_mask_on_lesion', False) and lesions:
        launch, ones = [], []
        for i, name in lesions:
            org = organ_planes(name, organ_idx)
            if org is None:
                ones.append((i, name))
            else:
                launch.append((i, name, organ_idx[org[0]], organ_idx[org[1]] if len(org) > 1 else -1))
        if launch:
            masked = torch.ops.rsuper.organ_mask(pred, [x[0] for x in launch], [x[2] for x in launch], [x[3] for x in launch])
            for k, (i, name, _, _) in enumerate(launch):
                planes[name] = masked[k]
        for i, name in ones:                  # organ of ones, dilated: still ones -> the lesion plane itself
            planes[name] = pred[i].clone()
    for i, name in lesions:
        p = planes[name]
        if getattr(args, 'connected_components', False):
            p = keep_largest_component(p)
        out[name] = p
    return out


def prediction(model_list, img, args, tgt_organ=None, to_cpu=False):
    """prediction (:180-246): img (D, H, W).  Sums the sliding-window probabilities of the models in model order (float32, from zeros: a sum,
    not a mean) and thresholds the sum at 0.5.  Cases deeper than 800 are cut into ceil(D / ceil(D / 800))-deep chunks inferred on their own
    (windows never cross a chunk boundary).  tgt_organ: the pancreas-only mask of inference_sliding_window, (D, H, W); it is cut with the image.
    Returns (label uint8 (classes, D, H, W), raw float32 (classes, D, H, W)) on the device, or on the host with to_cpu=True."""
    D, H, W = img.shape
    x = img.unsqueeze(0).unsqueeze(0)
    if D > Z_LEN:
        n = math.ceil(D / Z_LEN)
        cl = math.ceil(D / n)
        chunks = [(i * cl, min((i + 1) * cl, D)) for i in range(n)]
    else:
        chunks = [(0, D)]
    labels, raws = [], []
    with torch.no_grad():
        for z0, z1 in chunks:
            xc = x[:, :, z0:z1]
            org = None if tgt_organ is None else tgt_organ[..., z0:z1, :, :]
            total = None
            for model in model_list:
                pred = inference_sliding_window(model, xc, args, pancreas=org, to_cpu=False).squeeze(0)
                if total is None:
                    total = torch.zeros((args.classes, z1 - z0, H, W), device=pred.device, dtype=pred.dtype)
                total += pred
            labels.append((total > 0.5).to(torch.uint8))
            raws.append(total)
    label = labels[0] if len(labels) == 1 else torch.cat(labels, dim=1)
    raw = raws[0] if len(raws) == 1 else torch.cat(raws, dim=1)
    if to_cpu:
        return label.cpu(), raw.cpu()
    return label, raw


_library.install_postprocess_ops(_detection_volumes_impl, _detection_binary_impl, _organ_mask_impl, _largest_component_impl)
