"""Whole-CT preprocessing of rsuper_train/predict_abdomenatlas.py on the MI355X path: `preprocess` from the clip onward (:347-354) and
pad_to_training_size / unpad_img (:249-322) under the reference's names, on device tensors.

The reference clips, takes torch.mean and torch.std of the whole volume, subtracts, divides and pads: five full-volume passes and a padded copy.
Here the z-score is two launches (csrc/resample.hip): `rsuper_ct_stats` writes per-block f64 partials of clip(x), `rsuper_ct_normalize` re-reduces
them in every block and writes (clip(x) - mean) / std straight into the zero-padded volume.  The input may stay int16, as a CT is stored.
`torch.ops.rsuper.ct_normalize` is the dispatcher entry (CUDA key only; a CPU tensor raises RSuperHipError).

NIfTI I/O, reorientation and the B-spline resample to the target spacing that precede the clip in `preprocess` are inference/nifti.py and
inference/nifti_device.py (load_nifti_device).  Out of scope: the nii-path `postprocess` organ gate (sitk.BinaryDilate with ITK's ball element)
and multi-GPU case sharding.
"""
import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library

CLIP = (-991.0, 500.0)         # preprocess :347
_DT = {torch.int16: 2, torch.float32: 1}      # RSUPER_VOX_I16 / RSUPER_VOX_F32


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def ct_stats_workspace(device):
    return torch.empty((_l.lib().rsuper_ct_stats_workspace_bytes(),), device=device, dtype=torch.uint8)


def _check_volume(hu, what):
    if not torch.is_tensor(hu) or not hu.is_cuda:
        raise _l.RSuperHipError(f'{what} needs a device tensor (no CPU fallback)')
    assert hu.dim() == 3 and hu.dtype in _DT, f'{what}: a (D, H, W) int16 or float32 volume, got {tuple(hu.shape)} {hu.dtype}'
    return hu.contiguous()


def _ct_normalize_impl(hu, lo, hi, out_shape, offset, workspace=None, pop=False):
    """hu (D, H, W) int16 / float32 -> ((Do, Ho, Wo) float32 with the z-score of clip(hu, lo, hi) at `offset` and zeros elsewhere, (mean, std) as a
    2-element float32 device tensor).  Two launches, no host synchronisation.  pop: the population std (rsuper_ct_normalize_pop: np.std, the
    dataset conversion's) instead of the unbiased one."""
    hu = _check_volume(hu, 'ct_normalize')
    D, H, W = hu.shape
    Do, Ho, Wo = out_shape
    L = _l.lib()
    ws = ct_stats_workspace(hu.device) if workspace is None else workspace
    assert ws.is_cuda and ws.is_contiguous()
    nbytes = ws.numel() * ws.element_size()
    out = torch.empty((Do, Ho, Wo), device=hu.device, dtype=torch.float32)
    ms = torch.empty((2,), device=hu.device, dtype=torch.float32)
    _l.check(L.rsuper_ct_stats(hu.data_ptr(), _DT[hu.dtype], D, H, W, lo, hi, ws.data_ptr(), nbytes, _stream(hu)), 'ct_stats')
    _l.check((L.rsuper_ct_normalize_pop if pop else L.rsuper_ct_normalize)(hu.data_ptr(), _DT[hu.dtype], D, H, W, lo, hi, ws.data_ptr(), nbytes,
                                                                           out.data_ptr(), Do, Ho, Wo, offset[0], offset[1], offset[2],
                                                                           ms.data_ptr(), _stream(hu)), 'ct_normalize_pop' if pop else 'ct_normalize')
    return out, ms


def normalize_ct(hu, clip=CLIP, pad=None, workspace=None):
    """(clip(hu) - mean) / std with the mean and unbiased std of the whole clipped volume (preprocess :347-352).  hu: (D, H, W) int16 or float32 on
    the device.  pad: None, or (out_shape, offset): the result sits at `offset` of a zero volume of `out_shape` (z, y, x).  Returns
    (float32 tensor, mean, std); mean and std are 0-dim device tensors (float32 roundings of the float64 statistics), so nothing waits for the
    device.  A constant volume gives NaN inside the box, as the reference's 0 / 0 does; the padding stays zero."""
    if not torch.is_tensor(hu) or not hu.is_cuda:
        raise _l.RSuperHipError('normalize_ct needs a device tensor (no CPU fallback)')
    out_shape, offset = (tuple(hu.shape), (0, 0, 0)) if pad is None else pad
    out, ms = torch.ops.rsuper.ct_normalize(hu, float(clip[0]), float(clip[1]), [int(v) for v in out_shape], [int(v) for v in offset], workspace)
    return out, ms[0], ms[1]


def _pad_geometry(shape, args):
    """pad_to_training_size's result as (output shape, offset of the input inside it, original_idx).  The reference's F.pad calls name the wrong
    pair for z and x (see pad_to_training_size): a short z widens x, a short x widens z, a short y widens y."""
    if args.dimension == '2d':
        raise NotImplementedError('2d prediction is outside the accelerated hot path (3-D UNet only)')
    if args.dimension != '3d':
        raise ValueError('Error in image dimension')
    z, y, x = (int(v) for v in shape)
    ts = args.training_size
    dz = (ts[0] + 2 - z) // 2 if z < ts[0] else 0
    dy = (ts[1] + 2 - y) // 2 if y < ts[1] else 0
    dx = (ts[2] + 2 - x) // 2 if x < ts[2] else 0
    out_shape = (z + 2 * dx, y + 2 * dy, x + 2 * dz)
    return out_shape, (dx, dy, dz), [dz, dz + z, dy, dy + y, dx, dx + x]


def pad_to_training_size(tensor_img, args):
    """pad_to_training_size (:249-306), 3-D branch: every axis shorter than args.training_size is padded with zeros by (size + 2 - n) // 2 on both
    sides.  Returns (padded float32 tensor, [z_start, z_end, y_start, y_end, x_start, x_end]).

    Axis quirk, reproduced bit for bit (parity is defined against the reference's outputs): the reference pads a 3-D tensor with
    F.pad(t, (diff, diff, 0, 0, 0, 0)) for z and F.pad(t, (0, 0, 0, 0, diff, diff)) for x, and F.pad counts pairs from the LAST axis.  A short z
    therefore widens x while z_start / z_end are recorded for z, and a short x widens z: a (10, 100, 120) volume with training size 96 becomes
    (10, 100, 208) with original_idx [44, 54, 0, 100, 0, 120].  y is padded where it is recorded.  There is no switch for this.

    Host index logic plus one padded-copy launch; preprocess_array fuses that copy into the z-score's second launch."""
    out_shape, offset, idx = _pad_geometry(tensor_img.shape, args)
    x = _check_volume(tensor_img, 'pad_to_training_size')
    if out_shape == tuple(x.shape):
        return tensor_img, idx             # F.pad is never called: the reference returns its argument
    D, H, W = x.shape
    out = torch.empty(out_shape, device=x.device, dtype=torch.float32)
    _l.check(_l.lib().rsuper_pad_box(x.data_ptr(), _DT[x.dtype], D, H, W, out.data_ptr(), out_shape[0], out_shape[1], out_shape[2],
                                     offset[0], offset[1], offset[2], _stream(x)), 'pad_box')
    return out, idx


def unpad_img(tensor_pred, original_idx, args):
    """unpad_img (:311-322), 3-D branch: the slice [z_start:z_end, y_start:y_end, x_start:x_end] of a (D, H, W) tensor, a view.  With the axis
    quirk of pad_to_training_size the recorded z range is cut from an axis that was padded by x's amount, with Python's slice clipping, exactly
    as the reference does."""
    if args.dimension == '2d':
        raise NotImplementedError('2d prediction is outside the accelerated hot path (3-D UNet only)')
    if args.dimension != '3d':
        raise ValueError('Error in image dimension')
    z_start, z_end, y_start, y_end, x_start, x_end = original_idx
    return tensor_pred[z_start:z_end, y_start:y_end, x_start:x_end]


def preprocess_array(hu, args, workspace=None):
    """`preprocess` (:325-356) from the clip onward: clip to [-991, 500], z-score with the whole-volume mean and unbiased std, pad to
    args.training_size.  hu: the (D, H, W) HU array, reoriented and resampled to the target spacing by the caller, int16 or float32, a numpy
    array or a tensor (moved to the current device).  Returns (tensor_img, original_idx) as the reference does; the statistics pass and the
    normalise + pad pass are the only two launches."""
    if not torch.is_tensor(hu):
        hu = torch.from_numpy(hu)
    if not hu.is_cuda:
        hu = hu.to('cuda')
    if hu.dtype not in _DT:
        hu = hu.float()
    out_shape, offset, idx = _pad_geometry(hu.shape, args)
    out, _, _ = normalize_ct(hu, CLIP, (out_shape, offset), workspace)
    return out, idx


_library.install_preprocess_ops(_ct_normalize_impl)
