"""The NIfTI front and back end of a case on the MI355X path: what `preprocess` does with SimpleITK before its clip (predict_abdomenatlas.py
:333-343 -- reorient to 'RAI', cubic B-spline in-plane and nearest along z to the target spacing) and the masks back on the scan's own grid, in
its own voxel order, as `.nii.gz`.

    load_nifti_device   file -> canonical (Z, Y, X) float32 HU at the target spacing.  The file's voxel buffer is uploaded as it is;
                        `rsuper_nifti_load_prefilter` reads it through the strides that realise the reorientation (a flip is a negative stride),
                        scales it and, when the spacing differs, turns every slice into cubic B-spline coefficients; `rsuper_bspline_resample`
                        evaluates them through the host's per-axis tables (inference/nifti.py).
    predict_nifti_case  load_nifti_device -> predict_case (back to the scan's canonical grid) -> postprocess_npz.
    save_nifti_masks    one `rsuper_reorient_store` launch puts every class plane in file order behind its 352 header bytes, the device DEFLATE
                        encoder compresses the planes, and only compressed bytes cross the bus.

`torch.ops.rsuper.nifti_load_prefilter / bspline_resample / reorient_store` are the dispatcher entries (CUDA key only; a CPU tensor raises
RSuperHipError).  Parity is with scipy (tests/nifti_ref.py); what is unverified against ITK is listed in INTEGRATION section 3h."""
import os
from dataclasses import dataclass

import numpy as np
import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library
from . import nifti as _n

# NIfTI-1 datatype -> (RSUPER_NII_* code, bytes per voxel); float64 is float32 by the time it leaves read_nifti
_NII = {2: (0, 1), 256: (1, 1), 4: (2, 2), 512: (3, 2), 8: (4, 4), 16: (5, 4), 64: (5, 4)}
_LAUNCHES = {'load': 0, 'prefilter': 0, 'resample': 0, 'store': 0}


def nifti_launches():
    """Calls of the three entry points this process has made: {'load', 'prefilter' (loads that ran the prefilter), 'resample', 'store'}."""
    return dict(_LAUNCHES)


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _need_device(t, what):
    if not torch.is_tensor(t) or not t.is_cuda:
        raise _l.RSuperHipError(f'{what} needs a device tensor (no CPU fallback)')


def _load_prefilter_impl(raw, dtype, size, strides, offset, slope, inter, prefilter):
    """raw: the file's voxel buffer as a flat uint8 device tensor; dtype: RSUPER_NII_*; size (Z, Y, X); strides (sz, sy, sx) in elements ->
    (Z, Y, X) float32 samples or B-spline coefficients."""
    _need_device(raw, 'nifti_load_prefilter')
    esz = (1, 1, 2, 2, 4, 4)[dtype]
    assert raw.dtype == torch.uint8 and raw.dim() == 1 and raw.is_contiguous() and raw.numel() % esz == 0
    Z, Y, X = (int(v) for v in size)
    out = torch.empty((Z, Y, X), device=raw.device, dtype=torch.float32)
    with torch.cuda.device(raw.device):
        _l.check(_l.lib().rsuper_nifti_load_prefilter(raw.data_ptr(), dtype, raw.numel() // esz, Z, Y, X, int(strides[0]), int(strides[1]),
                                                      int(strides[2]), int(offset), slope, inter, 1 if prefilter else 0, out.data_ptr(),
                                                      _stream(raw)), 'nifti_load_prefilter')
    _LAUNCHES['load'] += 1
    _LAUNCHES['prefilter'] += 1 if prefilter else 0
    return out


def _bspline_resample_impl(coef, ix, wx, iy, wy, iz, outside_value):
    """coef (Z, Y, X) float32; ix, iy (n, 4) int32 and wx, wy (n, 4) float32, iz (n,) int32 on the device -> (Zo, Yo, Xo) float32."""
    for t in (coef, ix, wx, iy, wy, iz):
        _need_device(t, 'bspline_resample')
    assert coef.dtype == torch.float32 and coef.dim() == 3, 'bspline_resample: (Z, Y, X) float32 coefficients'
    for i, w in ((ix, wx), (iy, wy)):
        assert i.dtype == torch.int32 and w.dtype == torch.float32 and i.dim() == 2 and i.shape[1] == 4 and i.shape == w.shape
    assert iz.dtype == torch.int32 and iz.dim() == 1
    coef, ix, wx, iy, wy, iz = (t.contiguous() for t in (coef, ix, wx, iy, wy, iz))
    Z, Y, X = coef.shape
    out = torch.empty((iz.shape[0], iy.shape[0], ix.shape[0]), device=coef.device, dtype=torch.float32)
    with torch.cuda.device(coef.device):
        _l.check(_l.lib().rsuper_bspline_resample(coef.data_ptr(), Z, Y, X, ix.data_ptr(), wx.data_ptr(), iy.data_ptr(), wy.data_ptr(), iz.data_ptr(),
                                                  out.data_ptr(), out.shape[0], out.shape[1], out.shape[2], outside_value, _stream(coef)),
                 'bspline_resample')
    _LAUNCHES['resample'] += 1
    return out


def _reorient_store_impl(stack, dst, dst_offset, plane_stride, shape_ijk, strides, offset):
    """stack (C, Z, Y, X) uint8 canonical -> dst (flat uint8): plane c in file order at dst_offset + c * plane_stride; strides (ci, cj, ck) and
    offset address the canonical plane by the file's (i, j, k)."""
    _need_device(stack, 'reorient_store')
    _need_device(dst, 'reorient_store')
    assert stack.dtype == torch.uint8 and stack.dim() == 4 and dst.dtype == torch.uint8 and dst.dim() == 1 and dst.is_contiguous()
    stack = stack.contiguous()
    C, Z, Y, X = stack.shape
    with torch.cuda.device(stack.device):
        _l.check(_l.lib().rsuper_reorient_store(stack.data_ptr(), C, Z, Y, X, dst.data_ptr(), dst.numel(), int(dst_offset), int(plane_stride),
                                                int(shape_ijk[0]), int(shape_ijk[1]), int(shape_ijk[2]), int(strides[0]), int(strides[1]),
                                                int(strides[2]), int(offset), _stream(stack)), 'reorient_store')
    _LAUNCHES['store'] += 1


_OPS = _library.install_nifti_ops(_load_prefilter_impl, _bspline_resample_impl, _reorient_store_impl)


@dataclass
class NiftiGeometry:
    """What the way back to the file needs.  shape_ijk, pixdim, qfac, affine: the input's; (perm, flip): nifti.orientation_plan of the affine;
    size, spacing: the canonical grid before resampling, in x, y, z order (predict_case's orig_size / orig_spacing)."""
    shape_ijk: tuple
    pixdim: tuple
    qfac: float
    affine: np.ndarray
    perm: tuple
    flip: tuple
    size: tuple
    spacing: tuple


def geometry_of(vol):
    aff = _n.affine(vol)
    perm, flip = _n.orientation_plan(aff)
    size, _, _, inv = _n.canonical_layout(vol.shape, perm, flip)
    return NiftiGeometry(tuple(vol.shape), tuple(vol.pixdim), vol.qfac, aff, perm, flip, size, tuple(vol.pixdim[a] for a in inv))


def same_spacing(spacing, target_spacing):
    """The reference's test (`preprocess` :337): torch.equal of the two float32 tensors."""
    return torch.equal(torch.tensor([float(v) for v in spacing]), torch.tensor([float(v) for v in target_spacing]))


def reorient_device(vol, geom=None, prefilter=False, device='cuda'):
    """The canonical (Z, Y, X) float32 volume of a NiftiVolume, scaled by scl_slope / scl_inter: the samples, or with prefilter their in-plane
    cubic B-spline coefficients.  One upload of the file's bytes and one call."""
    geom = geom or geometry_of(vol)
    code, esz = _NII[vol.datatype]
    size, stride, offset, _ = _n.canonical_layout(vol.shape, geom.perm, geom.flip)
    raw = torch.from_numpy(vol.data.reshape(-1).view(np.uint8)).to(device)
    slope, inter = vol.scl_slope, vol.scl_inter
    if not (np.isfinite(slope) and np.isfinite(inter)) or slope == 0:
        slope, inter = 1.0, 0.0
    return _OPS[0](raw, code, list(size[::-1]), list(stride[::-1]), offset, slope, inter, bool(prefilter))


def resample_tables(size, spacing, target_spacing, device):
    """The device tables of the reference's two resample passes for a canonical grid (x, y, z order): B-spline in x and y, nearest in z."""
    ix, wx = _n.resample_axis_table(size[0], spacing[0], target_spacing[0], 'bspline')
    iy, wy = _n.resample_axis_table(size[1], spacing[1], target_spacing[1], 'bspline')
    iz = _n.resample_axis_table(size[2], spacing[2], target_spacing[2], 'nearest')
    return tuple(torch.from_numpy(t).to(device) for t in (ix, wx, iy, wy, iz))


def load_nifti_device(path_or_volume, target_spacing=(1., 1., 1.), outside_value=0.0, device='cuda'):
    """A `.nii` / `.nii.gz` path or a NiftiVolume -> (hu, geom): the canonical (Z, Y, X) float32 HU tensor at target_spacing (x, y, z order) on
    the device and the NiftiGeometry of the input.  When the canonical spacing equals the target as float32 (the reference's test) neither the
    prefilter nor the resample runs.  Otherwise: prefilter in x and y, then B-spline in-plane and nearest along z through the host's tables;
    voxels whose source position is outside the scan are outside_value (ITK's default pixel, 0)."""
    vol = path_or_volume if isinstance(path_or_volume, _n.NiftiVolume) else _n.read_nifti(path_or_volume)
    geom = geometry_of(vol)
    if same_spacing(geom.spacing, target_spacing):
        return reorient_device(vol, geom, False, device), geom
    coef = reorient_device(vol, geom, True, device)
    ix, wx, iy, wy, iz = resample_tables(geom.size, geom.spacing, target_spacing, coef.device)
    return _OPS[1](coef, ix, wx, iy, wy, iz, float(outside_value)), geom


def predict_nifti_case(models, path, args, classes, target_spacing=(1., 1., 1.), return_raw=False):
    """One NIfTI case: load_nifti_device -> predict_case with the scan's canonical grid as orig_spacing / orig_size -> postprocess_npz (inside
    predict_case).  Returns ({class: (Z, Y, X) uint8 device tensor on the scan's canonical grid}, geom); with return_raw the (C, Z, Y, X) float32
    probabilities in between."""
    from .resample import predict_case
    hu, geom = load_nifti_device(path, target_spacing)
    pred, raw = predict_case(models, hu, args, classes, orig_spacing=geom.spacing, orig_size=geom.size, target_spacing=target_spacing)
    return (pred, raw, geom) if return_raw else (pred, geom)


def save_nifti_masks(case_dir, pred_dict, names, geom):
    """predictions/<class>.nii.gz for every name: uint8, the input's shape, pixdim, affine and voxel order.  One rsuper_reorient_store launch for the
    whole stack writes each class behind its 352 header bytes, one device DEFLATE call compresses the planes, and the host adds the gzip framing."""
    from .npz_writer import MAX_PITCH, gzip_planes_device
    stack = torch.stack([pred_dict[n].to(torch.uint8) for n in names])
    _need_device(stack, 'save_nifti_masks')
    if tuple(stack.shape[1:]) != tuple(geom.size[::-1]):
        raise ValueError(f'save_nifti_masks: masks of shape {tuple(stack.shape[1:])} are not on the scan\'s canonical grid {tuple(geom.size[::-1])}')
    C, nvox = stack.shape[0], stack[0].numel()
    header = _n.nifti1_header(geom.shape_ijk, geom.pixdim, geom.affine, 2)
    plane = len(header) + nvox
    buf = torch.empty((C, plane), device=stack.device, dtype=torch.uint8)
    buf[:, :len(header)] = torch.frombuffer(bytearray(header), dtype=torch.uint8).to(stack.device)
    # canonical element strides seen from the file's axes: voxel axis a runs along canonical axis perm[a]
    cstride = (1, geom.size[0], geom.size[0] * geom.size[1])
    strides = [(-cstride[geom.perm[a]] if geom.flip[a] else cstride[geom.perm[a]]) for a in range(3)]
    offset = sum((geom.shape_ijk[a] - 1) * cstride[geom.perm[a]] for a in range(3) if geom.flip[a])
    _OPS[2](stack, buf.view(-1), len(header), plane, list(geom.shape_ijk), strides, offset)
    ni = geom.shape_ijk[0]
    files = gzip_planes_device(buf.view(-1), plane, plane, C, pitch=ni if ni <= MAX_PITCH else 0, table='mask')
    os.makedirs(os.path.join(case_dir, 'predictions'), exist_ok=True)
    for n, data in zip(names, files):
        with open(os.path.join(case_dir, 'predictions', n + '.nii.gz'), 'wb') as f:
            f.write(data)
