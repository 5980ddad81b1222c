"""eval_AUC.detection (rsuper_train/eval_AUC.py:56-112) on an array instead of a NIfTI path, on the MI355X.

The reference resamples the lesion probability volume to 1 mm (ndimage.zoom, order 1, in float64) and, for each of 9 confidence thresholds,
binarises, erodes with a 3x3x3 box, dilates twice, ANDs with the binary volume and counts.  That chain is one integer pass here: with
L = the number of thresholds a voxel exceeds, the volume at threshold t is #(min(max5(min3(L)), L) > t) (min3 reads level 0 outside the
volume like binary_erosion's border; two box-3 dilations of a box domain are one box-5 maximum).  `rsuper_detection` resamples, levels,
filters and histograms every output tile in one launch; the counts are integer atomics, the maximum an atomicMax on an order-preserving
key, so the result does not depend on scheduling.

test_with_reports.detection (rsuper_train/test_with_reports.py:56-94) is `detection_binary`: the saved mask is binarised at `th` first, resampled
with ndimage.zoom(order=0), eroded once, dilated twice, ANDed with itself and counted -- the one-threshold case of the same tile pass with a
nearest sample (`rsuper_detection_binary`), reading uint8 / bool planes as bytes.
"""
import ctypes

import numpy as np
import torch

from ..hip import lib as _l

THRESHOLDS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)


def zoom_shape(shape, factors):
    """Output shape of ndimage.zoom: round(n * f) per axis, Python rounding (half to even: 5 * 0.5 -> 2, 7 * 0.5 -> 4)."""
    return tuple(int(round(float(n) * float(f))) for n, f in zip(shape, factors))


def _detection_volumes_impl(x, out_shape, thresholds, erode, workspace=None):
    """x (P, D, H, W) float32 on the device, resampled onto out_shape; thresholds sorted ascending.  Returns (volumes (P, T) int64,
    max_prob (P,) float64) on the device.  workspace: optional device buffer of rsuper_detection_workspace_bytes(P) bytes."""
    assert x.is_cuda and x.dtype == torch.float32 and x.dim() == 4, 'detection: (P, D, H, W) float32 on the device'
    x = x.contiguous()
    P, Di, Hi, Wi = x.shape
    Do, Ho, Wo = (int(v) for v in out_shape)
    T = len(thresholds)
    L = _l.lib()
    need = L.rsuper_detection_workspace_bytes(P)
    ws = torch.empty((need,), device=x.device, dtype=torch.uint8) if workspace is None else workspace
    assert ws.is_cuda and ws.numel() * ws.element_size() >= need
    vols = torch.empty((P, T), device=x.device, dtype=torch.int64)
    mx = torch.empty((P,), device=x.device, dtype=torch.float64)
    th = (ctypes.c_double * max(1, T))(*[float(t) for t in thresholds])
    _l.check(L.rsuper_detection(x.data_ptr(), P, Di, Hi, Wi, Do, Ho, Wo, ctypes.cast(th, ctypes.c_void_p), T, 1 if erode else 0,
                                vols.data_ptr(), mx.data_ptr(), ws.data_ptr(), torch._C._cuda_getCurrentRawStream(x.device.index)), 'detection')
    return vols, mx


def detection(array, spacing=(1, 1, 1), thresholds=THRESHOLDS, erode=True, workspace=None):
    """eval_AUC.detection (:56-112) on a lesion probability array: resample from `spacing` (per array axis) to 1 mm, then the volume (voxels)
    at each threshold after erosion + double dilation + AND (erode=True) or of the binary volume (erode=False), and the maximum resampled
    probability.  Returns ({threshold: volume}, max_prob) with Python ints and a float.

    array: (D, H, W), or (P, D, H, W) for several lesion planes of one case (same shape and spacing, one launch; returns a list of results).
    float32 numpy array or tensor (the NIfTI's stored dtype; float64 input is rounded to float32).  Thresholds compare in float64."""
    x = torch.as_tensor(np.ascontiguousarray(array)) if isinstance(array, np.ndarray) else array
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise _l.RSuperHipError('detection needs an MI355X device (no CPU fallback)')
        x = x.to('cuda')
    x = x.to(torch.float32)
    single = x.dim() == 3
    x4 = x.unsqueeze(0) if single else x
    assert x4.dim() == 4, f'detection: (D, H, W) or (P, D, H, W) array, got {tuple(x.shape)}'
    factors = [float(s) / 1.0 for s in spacing]                   # resample_image: original spacing / target spacing (1, 1, 1)
    out_shape = zoom_shape(x4.shape[1:], factors)
    if min(out_shape) < 1:
        raise ValueError(f'detection: zoom of {tuple(x4.shape[1:])} by {factors} gives an empty volume {out_shape}')
    ths = [float(t) for t in thresholds]
    order = sorted(range(len(ths)), key=ths.__getitem__)
    vols, mx = torch.ops.rsuper.detection_volumes(x4, list(out_shape), [ths[k] for k in order], bool(erode), workspace)
    vols, mx = vols.cpu().tolist(), mx.cpu().tolist()
    res = []
    for p in range(x4.shape[0]):
        v = {}
        for pos, k in enumerate(order):
            v[thresholds[k]] = int(vols[p][pos])
        res.append(({t: v[t] for t in thresholds}, float(mx[p])))
    return res[0] if single else res


def _detection_binary_impl(x, out_shape, th, erode, workspace=None):
    """x (P, D, H, W) uint8 or float32 on the device, binarised at th and resampled (order 0) onto out_shape.  Returns the (P,) int64 counts on
    the device.  workspace: optional device buffer of rsuper_detection_workspace_bytes(P) bytes."""
    assert x.is_cuda and x.dtype in (torch.uint8, torch.float32) and x.dim() == 4, 'detection_binary: (P, D, H, W) uint8 / float32 on the device'
    x = x.contiguous()
    P, Di, Hi, Wi = x.shape
    Do, Ho, Wo = (int(v) for v in out_shape)
    L = _l.lib()
    need = L.rsuper_detection_workspace_bytes(P)
    ws = torch.empty((need,), device=x.device, dtype=torch.uint8) if workspace is None else workspace
    assert ws.is_cuda and ws.numel() * ws.element_size() >= need
    counts = torch.empty((P,), device=x.device, dtype=torch.int64)
    _l.check(L.rsuper_detection_binary(x.data_ptr(), 1 if x.dtype == torch.uint8 else 0, P, Di, Hi, Wi, Do, Ho, Wo, float(th), 1 if erode else 0,
                                       counts.data_ptr(), ws.data_ptr(), torch._C._cuda_getCurrentRawStream(x.device.index)), 'detection_binary')
    return counts


def _binary_counts(array, spacing, th, erode, workspace=None):
    """The device part of detection_binary: ((P,) int64 counts on the device, single)."""
    x = torch.as_tensor(np.ascontiguousarray(array)) if isinstance(array, np.ndarray) else array
    if x.dtype == torch.bool:
        x = x.view(torch.uint8)
    if x.dtype not in (torch.uint8, torch.float32):
        raise TypeError(f'detection_binary: uint8 / bool / float32 array, got {x.dtype}')
    if not x.is_cuda:
        if not torch.cuda.is_available():
            raise _l.RSuperHipError('detection_binary needs an MI355X device (no CPU fallback)')
        x = x.to('cuda')
    single = x.dim() == 3
    x4 = x.unsqueeze(0) if single else x
    assert x4.dim() == 4, f'detection_binary: (D, H, W) or (P, D, H, W) array, got {tuple(x.shape)}'
    factors = [float(s) / 1.0 for s in spacing]
    out_shape = zoom_shape(x4.shape[1:], factors)
    if min(out_shape) < 1:
        raise ValueError(f'detection_binary: zoom of {tuple(x4.shape[1:])} by {factors} gives an empty volume {out_shape}')
    return torch.ops.rsuper.detection_binary(x4, list(out_shape), float(th), bool(erode), workspace), single


def detection_binary(array, spacing=(1, 1, 1), th=0.5, erode=True, workspace=None):
    """test_with_reports.detection (:56-94) on a saved lesion mask: `array > th` (in float64; a value equal to th is not set), resampled from
    `spacing` (per array axis) to 1 mm with ndimage.zoom's order 0, then the voxel count after erosion + double dilation + AND (erode=True) or of
    the resampled mask itself (erode=False).  Returns a Python int.

    array: (D, H, W), or (P, D, H, W) for several lesion planes of one case (same shape and spacing, one launch; returns a list).  uint8, bool
    or float32, numpy array or tensor; uint8 / bool planes are read as bytes."""
    counts, single = _binary_counts(array, spacing, th, erode, workspace)
    res = [int(v) for v in counts.cpu().tolist()]
    return res[0] if single else res
