"""rsuper_train/metric/metrics.py on the MI355X path: compute_surface_distances (:265-573) and the statistics on its result (:579-879) under the
reference's names, on device tensors.

The reference copies both masks to the host, runs two scipy distance transforms over the bounding box and sorts the surfels in Python.  Here the
masks stay on the device: `rsuper_surface_codes` writes the neighbour codes, the box of the border corners and the voxel counts of every plane of
a stack in one launch, `rsuper_edt3` is the exact distance transform of one code volume over that box, `rsuper_surfel_gather` compacts the
(distance, area) pairs, and torch.sort orders them by (distance, area).  `torch.ops.rsuper.surface_distances` and `torch.ops.rsuper.edt3` are the
dispatcher entries (hip/library.py).  Only the 3-D case exists here; the 2-D contour case raises.

The statistics are float64 torch reductions over the sorted arrays: sums and prefix sums whose order depends only on the length, so equal
inputs give bit-identical results on every call.
"""
import math

import numpy as np
import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library
from .lookup_tables import resolve_surface_area_table

KEYS = ('distances_gt_to_pred', 'distances_pred_to_gt', 'surfel_areas_gt', 'surfel_areas_pred')


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _mask_u8(name, m):
    if not isinstance(m, torch.Tensor) or not m.is_cuda:
        raise _l.RSuperHipError(f'{name}: the mask must be a tensor on the MI355X device (no CPU fallback)')
    if m.dtype == torch.bool:
        m = m.view(torch.uint8)
    if m.dtype != torch.uint8:
        raise _l.RSuperHipError(f'{name}: bool / uint8 mask expected, got {m.dtype}')
    return m.contiguous()


def _edt3_impl(codes, box, spacing, workspace=None):
    """codes (Dc, Hc, Wc) uint8 neighbour codes; box = (z0, y0, x0, nz, ny, nx) in corners; spacing (s0, s1, s2).  Returns the (nz, ny, nx) float64
    squared distance of every corner of the box to the nearest border corner (code neither 0 nor 255) inside it; +inf when there is none."""
    if not codes.is_cuda or codes.dim() != 3 or codes.dtype != torch.uint8:
        raise _l.RSuperHipError(f'edt3: a (Dc, Hc, Wc) uint8 code volume on the device, got {codes.dtype} {tuple(codes.shape)}')
    codes = codes.contiguous()
    z0, y0, x0, nz, ny, nx = (int(v) for v in box)
    s0, s1, s2 = (float(s) for s in spacing)
    need = _l.lib().rsuper_edt3_workspace_bytes(nz, ny, nx)
    if need == 0:
        raise _l.RSuperHipError(f'edt3: box {(nz, ny, nx)} is not supported (a side above 4096 corners or more than 2^31 corners)')
    ws = torch.empty((need,), device=codes.device, dtype=torch.uint8) if workspace is None else workspace
    if not ws.is_cuda or not ws.is_contiguous():
        raise _l.RSuperHipError('edt3: the workspace must be a contiguous device tensor')
    out = torch.empty((max(nz, 0), max(ny, 0), max(nx, 0)), device=codes.device, dtype=torch.float64)
    Dc, Hc, Wc = codes.shape
    _l.check(_l.lib().rsuper_edt3(codes.data_ptr(), Dc, Hc, Wc, z0, y0, x0, nz, ny, nx, s0, s1, s2, out.data_ptr(), ws.data_ptr(),
                                  ws.numel() * ws.element_size(), _stream(codes)), 'edt3')
    return out


def _gather(codes, box, sq, table, n):
    """The n (distance, area) pairs of the border corners of `codes` inside the box, sorted by (distance, area)."""
    Dc, Hc, Wc = codes.shape
    dist = torch.empty((n,), device=codes.device, dtype=torch.float64)
    area = torch.empty((n,), device=codes.device, dtype=torch.float64)
    count = torch.empty((1,), device=codes.device, dtype=torch.int64)
    _l.check(_l.lib().rsuper_surfel_gather(codes.data_ptr(), Dc, Hc, Wc, *box, 0 if sq is None else sq.data_ptr(), table.data_ptr(),
                                           dist.data_ptr(), area.data_ptr(), count.data_ptr(), n, _stream(codes)), 'surfel_gather')
    area, i = torch.sort(area, stable=True)              # two stable passes: by area, then by distance = by (distance, area)
    dist, j = torch.sort(dist[i], stable=True)
    return dist, area[j]


def _codes(gt, pred):
    """rsuper_surface_codes on two contiguous (P, D, H, W) uint8 stacks: the two (P, D+1, H+1, W+1) uint8 code volumes, the (P, 6) int32 box of the
    border corners (lo z, y, x, hi z, y, x) and the (P, 5) int64 counts |gt|, |pred|, |gt & pred|, surfels of gt, surfels of pred."""
    P, D, H, W = gt.shape
    cg = torch.empty((P, D + 1, H + 1, W + 1), device=gt.device, dtype=torch.uint8)
    cp = torch.empty_like(cg)
    bbox = torch.empty((P, 6), device=gt.device, dtype=torch.int32)
    counts = torch.empty((P, 5), device=gt.device, dtype=torch.int64)
    _l.check(_l.lib().rsuper_surface_codes(gt.data_ptr(), pred.data_ptr(), P, D, H, W, cg.data_ptr(), cp.data_ptr(), bbox.data_ptr(),
                                           counts.data_ptr(), _stream(gt)), 'surface_codes')
    return cg, cp, bbox, counts


def _surface_distances_impl(mask_gt, mask_pred, spacing, area_table):
    """mask_gt, mask_pred (P, D, H, W) uint8 on the device, spacing 3 floats, area_table (256,) float64 on the device.  Returns
    ([d_gt_to_pred, d_pred_to_gt, areas_gt, areas_pred] * P as one flat list, counts (P, 5) int64: |gt|, |pred|, |gt & pred|, surfels of gt,
    surfels of pred)."""
    if mask_gt.dim() != 4 or mask_gt.shape != mask_pred.shape or mask_gt.dtype != torch.uint8 or mask_pred.dtype != torch.uint8:
        raise _l.RSuperHipError(f'surface_distances: two (P, D, H, W) uint8 stacks, got {mask_gt.dtype} {tuple(mask_gt.shape)} and '
                                f'{mask_pred.dtype} {tuple(mask_pred.shape)}')
    if area_table.dtype != torch.float64 or area_table.numel() != 256 or not area_table.is_cuda:
        raise _l.RSuperHipError('surface_distances: the area table is 256 float64 values on the device')
    mask_gt, mask_pred, area_table = mask_gt.contiguous(), mask_pred.contiguous(), area_table.contiguous()
    spacing = [float(s) for s in spacing]
    if len(spacing) != 3:
        raise _l.RSuperHipError('surface_distances: 3-D masks with a 3-element spacing only (the 2-D contour case is out of scope)')
    P, dev = mask_gt.shape[0], mask_gt.device
    cg, cp, bbox, counts = _codes(mask_gt, mask_pred)
    hb, hc = bbox.cpu().tolist(), counts.cpu().tolist()   # the box sizes decide the allocations below: one synchronisation per stack
    boxes = [(b[0], b[1], b[2], b[3] - b[0] + 1, b[4] - b[1] + 1, b[5] - b[2] + 1) for b in hb]
    need = [_l.lib().rsuper_edt3_workspace_bytes(*bx[3:]) if c[3] + c[4] > 0 else 0 for bx, c in zip(boxes, hc)]
    for bx, c, nb in zip(boxes, hc, need):
        if c[3] + c[4] > 0 and nb == 0:
            raise _l.RSuperHipError(f'surface_distances: box {bx[3:]} is not supported (a side above 4096 corners)')
    ws = torch.empty((max(need + [1]),), device=dev, dtype=torch.uint8)
    empty = torch.empty((0,), device=dev, dtype=torch.float64)
    out = []
    for p in range(P):
        n_gt, n_pred = hc[p][3], hc[p][4]
        bx = boxes[p]
        sq_gt = _edt3_impl(cg[p], bx, spacing, ws) if n_gt > 0 and n_pred > 0 else None
        sq_pred = _edt3_impl(cp[p], bx, spacing, ws) if n_gt > 0 and n_pred > 0 else None
        d_gp, a_g = _gather(cg[p], bx, sq_pred, area_table, n_gt) if n_gt > 0 else (empty, empty)
        d_pg, a_p = _gather(cp[p], bx, sq_gt, area_table, n_pred) if n_pred > 0 else (empty, empty)
        out += [d_gp, d_pg, a_g, a_p]
    return out, counts


_SD_OP, _EDT_OP = _library.install_metric_ops(_surface_distances_impl, _edt3_impl)


def edt3(codes, box, spacing, workspace=None):
    """Exact squared Euclidean distance transform of a corner sub-box: see torch.ops.rsuper.edt3 / rsuper_edt3 in include/rsuper_hip.h."""
    return _EDT_OP(codes, [int(v) for v in box], [float(s) for s in spacing], workspace)


def surface_distances_stack(mask_gt, mask_pred, spacing_mm, area_table=None):
    """compute_surface_distances for every plane of two (P, D, H, W) stacks in batched launches.  Returns (list of P result dicts, counts (P, 5)
    int64 device tensor: |gt|, |pred|, |gt & pred|, surfels of gt, surfels of pred)."""
    gt, pred = _mask_u8('mask_gt', mask_gt), _mask_u8('mask_pred', mask_pred)
    if len(spacing_mm) != 3 or gt.dim() != 4 or pred.dim() != 4:
        raise _l.RSuperHipError('surface distances: 3-D masks with a 3-element spacing only (the 2-D contour case is out of scope)')
    table = torch.from_numpy(resolve_surface_area_table(spacing_mm, area_table)).to(gt.device)
    flat, counts = _SD_OP(gt, pred, [float(s) for s in spacing_mm], table)
    return [dict(zip(KEYS, flat[4 * p:4 * p + 4])) for p in range(gt.shape[0])], counts


def compute_surface_distances(mask_gt, mask_pred, spacing_mm, area_table=None):
    """compute_surface_distances (:265-573) for two 3-D bool / uint8 device masks.  Returns the reference's dict: `distances_gt_to_pred`,
    `distances_pred_to_gt`, `surfel_areas_gt`, `surfel_areas_pred`, float64 device tensors sorted by (distance, area).  An empty mask gives empty
    arrays on its side and +inf distances on the other; two empty masks give four empty arrays.  area_table: see metric/lookup_tables.py."""
    if getattr(mask_gt, 'ndim', 0) != 3 or getattr(mask_pred, 'ndim', 0) != 3 or len(spacing_mm) != 3:
        raise _l.RSuperHipError('compute_surface_distances: 3-D masks with a 3-element spacing only (the 2-D contour case is out of scope)')
    res, _ = surface_distances_stack(_mask_u8('mask_gt', mask_gt)[None], _mask_u8('mask_pred', mask_pred)[None], spacing_mm, area_table)
    return res[0]


def _avg(d, a):
    return (torch.sum(d * a) / torch.sum(a)).item()       # 0 / 0 = nan on an empty side, inf on a side whose other mask is empty


def compute_average_surface_distance(surface_distances):
    """(average distance gt -> pred, average distance pred -> gt), weighted by surfel area (:579-635)."""
    sd = surface_distances
    return _avg(sd['distances_gt_to_pred'], sd['surfel_areas_gt']), _avg(sd['distances_pred_to_gt'], sd['surfel_areas_pred'])


def _percentile(d, a, percent):
    if d.numel() == 0:
        return math.inf
    cum = torch.cumsum(a, 0) / torch.sum(a)
    idx = int(torch.searchsorted(cum, torch.tensor([percent / 100.0], device=d.device, dtype=torch.float64)).item())
    return d[min(idx, d.numel() - 1)].item()


def compute_robust_hausdorff(surface_distances, percent):
    """The reference's rule (:641-717): per direction the distance at the first index whose normalised cumulative area is >= percent / 100
    (searchsorted, left), clamped to the last index, +inf on an empty side; the maximum of the two."""
    sd = surface_distances
    return max(_percentile(sd['distances_gt_to_pred'], sd['surfel_areas_gt'], percent),
               _percentile(sd['distances_pred_to_gt'], sd['surfel_areas_pred'], percent))


def _overlap(d, a, tol):
    return torch.sum(a[d <= tol]), torch.sum(a)


def compute_surface_overlap_at_tolerance(surface_distances, tolerance_mm):
    """(overlap fraction of the gt surface, of the predicted surface) at the tolerance (:723-779)."""
    sd = surface_distances
    og, sg = _overlap(sd['distances_gt_to_pred'], sd['surfel_areas_gt'], tolerance_mm)
    op, sp = _overlap(sd['distances_pred_to_gt'], sd['surfel_areas_pred'], tolerance_mm)
    return (og / sg).item(), (op / sp).item()


def compute_surface_dice_at_tolerance(surface_distances, tolerance_mm):
    """Surface Dice / NSD at the tolerance (:785-839)."""
    sd = surface_distances
    og, sg = _overlap(sd['distances_gt_to_pred'], sd['surfel_areas_gt'], tolerance_mm)
    op, sp = _overlap(sd['distances_pred_to_gt'], sd['surfel_areas_pred'], tolerance_mm)
    return ((og + op) / (sg + sp)).item()


def mask_counts(mask_gt, mask_pred):
    """(P, 5) int64 device tensor of two (P, D, H, W) stacks: |gt|, |pred|, |gt & pred|, surfels of gt, surfels of pred (rsuper_surface_codes)."""
    gt, pred = _mask_u8('mask_gt', mask_gt), _mask_u8('mask_pred', mask_pred)
    if gt.dim() != 4 or gt.shape != pred.shape:
        raise _l.RSuperHipError(f'mask_counts: two (P, D, H, W) stacks, got {tuple(gt.shape)} and {tuple(pred.shape)}')
    return _codes(gt, pred)[3]


def compute_dice_coefficient(mask_gt, mask_pred):
    """2 |gt & pred| / (|gt| + |pred|) from the voxel counts of the code kernel; NaN when both masks are empty (:845-879)."""
    if getattr(mask_gt, 'ndim', 0) != 3 or getattr(mask_pred, 'ndim', 0) != 3:
        raise _l.RSuperHipError('compute_dice_coefficient: two 3-D masks')
    g, p, i = mask_counts(_mask_u8('mask_gt', mask_gt)[None], _mask_u8('mask_pred', mask_pred)[None])[0, :3].tolist()
    return float(np.nan) if g + p == 0 else 2 * i / (g + p)
