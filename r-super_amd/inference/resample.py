"""Spacing resampling of predictions of rsuper_train/predict_abdomenatlas.py on the MI355X path: resample_image_with_gpu (:718-742) under the
reference's name, with unpad_img (:311-322) and the `> 0.5` of the postprocess_* variants fused in, and predict_case, the whole-case flow
preprocess -> prediction -> unpad_img -> resample_image_with_gpu -> postprocess_npz on device tensors.

The reference resamples a prediction one class plane at a time, in a Python loop of F.interpolate calls with a host round trip each.  Here a
whole (C, D, H, W) stack is one `rsuper_resample3d` launch (csrc/resample.hip) that reads the unpadded sub-box of every plane and writes float32
values, uint8 labels or `value > threshold`.  `torch.ops.rsuper.resample3d` is the dispatcher entry (CUDA key only; a CPU tensor raises
RSuperHipError).  The coordinate arithmetic is F.interpolate's on the reference's path: legacy 'nearest', and 'trilinear' with
align_corners=True, in float32.

NIfTI I/O and reorientation around predict_case are inference/nifti_device.py (predict_nifti_case, save_nifti_masks).  Out of scope: the
nii-path `postprocess` organ gate (sitk.BinaryDilate with ITK's radius-3 ball element) and multi-GPU case sharding.
"""
import numpy as np
import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library
from .postprocess import prediction, postprocess_npz
from .preprocess import preprocess_array

_DT = {torch.uint8: 0, torch.float32: 1}      # RSUPER_VOX_U8 / RSUPER_VOX_F32
_MODES = {'nearest': 0, 'trilinear': 1}
_LAUNCHES = 0


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def resample_launches():
    """Number of rsuper_resample3d launches this process has made (predict_case skips the launch on a same-grid, unpadded case)."""
    return _LAUNCHES


def _resample3d_impl(x, box, out_size, interp, threshold=None):
    """x (C, Dp, Hp, Wp) uint8 / bool / float32; box [z0, z1, y0, y1, x0, x1] inside it; out_size (Do, Ho, Wo) -> (C, Do, Ho, Wo): uint8 0 / 1 of
    `value > threshold` with a threshold, otherwise the input's dtype for 'nearest' and float32 for 'trilinear'."""
    global _LAUNCHES
    assert x.is_cuda and x.dim() == 4, 'resample3d: a (C, D, H, W) stack on the device'
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    assert x.dtype in _DT, f'resample3d: uint8 / bool / float32, got {x.dtype}'
    if interp not in _MODES:
        raise NotImplementedError(f'resample3d: interp {interp!r} (nearest / trilinear)')
    x = x.contiguous()
    C, Dp, Hp, Wp = x.shape
    z0, z1, y0, y1, x0, x1 = box
    Do, Ho, Wo = out_size
    odt = torch.uint8 if threshold is not None else (x.dtype if interp == 'nearest' else torch.float32)
    out = torch.empty((C, Do, Ho, Wo), device=x.device, dtype=odt)
    _l.check(_l.lib().rsuper_resample3d(x.data_ptr(), _DT[x.dtype], C, Dp, Hp, Wp, z0, y0, x0, z1 - z0, y1 - y0, x1 - x0, out.data_ptr(), _DT[odt],
                                        Do, Ho, Wo, _MODES[interp], 0 if threshold is None else 1, 0.0 if threshold is None else threshold,
                                        _stream(x)), 'resample3d')
    _LAUNCHES += 1
    return out


def _clip_box(box, shape):
    """original_idx of unpad_img -> the box its slices select from a (D, H, W) tensor (Python's slice clipping, as the reference's slicing does)."""
    out = []
    for a in range(3):
        lo, hi, _ = slice(int(box[2 * a]), int(box[2 * a + 1])).indices(int(shape[a]))
        if hi <= lo:
            raise ValueError(f'resample: box {list(box)} selects nothing of a {tuple(shape)} volume')
        out += [lo, hi]
    return out


def new_size_from_spacing(old_spacing, old_size, new_spacing):
    """round(old_size * old_spacing / new_spacing) as resample_image_with_gpu forms it (:721-730): old_size as a float32 array, numpy's
    round-half-to-even.  x, y, z order in; z, y, x order out."""
    new_spacing = np.array(new_spacing)[::-1]
    old_spacing = np.array(old_spacing)[::-1]
    old_size = np.array(old_size, dtype=np.float32)[::-1]
    new_size = old_size * (old_spacing / new_spacing)
    return new_size.round().astype(int).tolist()


def resample_image_with_gpu(tensor_img, old_spacing=(2., 2., 2.), old_size=(512, 512, 512), new_spacing=(1., 1., 1.), new_size=None,
                            interp='trilinear', *, box=None, threshold=None):
    """resample_image_with_gpu (:718-742) with the reference's signature and conventions: spacings and sizes are in x, y, z order, the tensor in
    z, y, x order; new_size=None means round(old_size * old_spacing / new_spacing).  As in the reference, old_size only enters that formula: the
    source grid is the tensor's own.

    Extensions: tensor_img may be a (C, D, H, W) stack as well as (D, H, W) -- one launch either way; box=original_idx (keyword only) resamples
    tensor_img[..., z_start:z_end, y_start:y_end, x_start:x_end], the fused unpad_img; threshold=t (keyword only) returns uint8 `value > t`.
    interp: 'trilinear' (align_corners=True, float32 out) or 'nearest' (F.interpolate's legacy 'nearest', the input's dtype out); anything else
    raises NotImplementedError.  uint8, bool and float32 inputs; a CPU tensor raises RSuperHipError."""
    if interp not in _MODES:
        raise NotImplementedError(f'resample_image_with_gpu: interp {interp!r} (trilinear / nearest)')
    if not torch.is_tensor(tensor_img) or not tensor_img.is_cuda:
        raise _l.RSuperHipError('resample_image_with_gpu needs a device tensor (no CPU fallback)')
    assert tensor_img.dim() in (3, 4), f'resample_image_with_gpu: (D, H, W) or (C, D, H, W), got {tuple(tensor_img.shape)}'
    if new_size is None:
        new_size = new_size_from_spacing(old_spacing, old_size, new_spacing)
    else:
        new_size = np.array(new_size)[::-1].tolist()
    x = tensor_img if tensor_img.dim() == 4 else tensor_img.unsqueeze(0)
    full = [0, x.shape[1], 0, x.shape[2], 0, x.shape[3]]
    out = torch.ops.rsuper.resample3d(x, full if box is None else _clip_box(box, x.shape[1:]), [int(v) for v in new_size], interp,
                                      None if threshold is None else float(threshold))
    return out if tensor_img.dim() == 4 else out.squeeze(0)


def predict_case(model_list, hu, args, classes, orig_spacing=None, orig_size=None, target_spacing=None):
    """One case from the HU array to the per-class dict, on the device: preprocess_array -> prediction(to_cpu=False) -> unpad + resample to the
    scan's own grid -> postprocess_npz.

    hu: (D, H, W) HU array at the target spacing (int16 / float32).  orig_spacing, orig_size (x, y, z order): the scan's own grid; with
    orig_size=None it is round(size * target_spacing / orig_spacing), and with neither spacing the prediction keeps hu's grid.  The labels go
    through one 'nearest' launch (uint8), the summed probabilities through one 'trilinear' launch (float32); on a same-grid case without padding
    both launches are skipped.  Returns ({class name: (D, H, W) device tensor} from postprocess_npz on the labels, raw (C, D, H, W) float32)."""
    img, idx = preprocess_array(hu, args)
    label, raw = prediction(model_list, img, args, to_cpu=False)
    box = _clip_box(idx, img.shape)
    size = [box[5] - box[4], box[3] - box[2], box[1] - box[0]]            # x, y, z of the unpadded prediction
    if orig_size is not None:
        new = [int(v) for v in orig_size]
    elif orig_spacing is not None and target_spacing is not None:
        new = new_size_from_spacing(target_spacing, size, orig_spacing)[::-1]
    else:
        new = size
    if new != size or tuple(label.shape[1:]) != tuple(size[::-1]):
        label = resample_image_with_gpu(label, new_size=new, interp='nearest', box=idx)
        raw = resample_image_with_gpu(raw, new_size=new, interp='trilinear', box=idx)
    return postprocess_npz(label, classes, args), raw


_library.install_resample_ops(_resample3d_impl)
