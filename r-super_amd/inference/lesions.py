"""Lesions of a mask, measured on the device: how many there are, where they sit and how large each is (csrc/lesion_table.hip,
`torch.ops.rsuper.lesion_table` / `torch.ops.rsuper.label_overlap`).  The reference has no counterpart: its data path only reads what a report says
about a tumour; this module goes the other way, from a predicted or annotated mask to a table of lesions, to lesion-level matching, and to report
rows that `training.dataset.augmented.estimate_tumor_volume` reads as they are.

A lesion is a connected component (6- or 26-connected) of one mask plane with at least `min_voxels` voxels.  The lesions of a plane are ordered by
voxel count, largest first, ties to the component whose first voxel comes first in C order; lesion k carries label k + 1.  Per lesion:

    root, voxels              the first voxel in C order (linear index) and the voxel count
    zmin .. xmax              the bounding box, inclusive
    sum_z, sum_y, sum_x       coordinate sums (centroid = sum / voxels)
    d3, (p3, q3)              the largest distance between two voxel centres in mm and the pair of linear indices that attains it
    a, (pa, qa)               the same among pairs that lie in one axis-0 slice: the longest in-slice diameter
    b                         the extent of the lesion, in the slice of (pa, qa), perpendicular to pa -> qa
    c                         (zmax - zmin) * spacing[0]
    flags                     bit 0: the 3-D search was skipped (more than max_candidates candidates), d3 is NaN and p3 = q3 = -1

All sizes are geometric measurements between voxel centres, not a radiologist's: `lesion_report_rows` adds one voxel per extent by default so that a
one-voxel lesion measures one voxel, not zero (see there)."""
import math

import numpy as np
import torch

from ..hip import lib as _l
from ..hip import ops as _ops  # noqa: F401  (imports hip/library.py in the order the op registration needs)
from ..hip import library as _library

MAX_PLANES = 64            # RSUPER_LESION_MAX_PLANES of the header: planes per launch group (more planes run as several groups)
MAX_ROWS = 254             # RSUPER_LESION_TABLE_MAX_ROWS
FIELDS_I = ('root', 'voxels', 'zmin', 'ymin', 'xmin', 'zmax', 'ymax', 'xmax', 'sum_z', 'sum_y', 'sum_x', 'p3', 'q3', 'pa', 'qa', 'flags')
FIELDS_F = ('d3', 'a', 'b', 'c')
TOTALS = ('kept', 'dropped', 'foreground', 'rows')
CSV_COLUMNS = ('BDMAP_ID', 'class', 'lesion') + FIELDS_I + FIELDS_F + ('location',)
REPORT_COLUMNS = ('Standardized Organ', 'Standardized Location', 'Tumor Size (mm)')


def _stream(t):
    return torch._C._cuda_getCurrentRawStream(t.device.index)


def _check_params(spacing, conn, min_voxels, max_lesions, max_candidates):
    """The bounds of the C ABI -> the spacing as three floats."""
    sp = tuple(float(s) for s in spacing)
    if len(sp) != 3 or not all(math.isfinite(s) and s > 0 for s in sp):
        raise ValueError(f'lesion_table: spacing must be three finite values > 0, got {spacing!r}')
    if conn not in (6, 26):
        raise ValueError(f'lesion_table: conn must be 6 or 26, got {conn!r}')
    if int(min_voxels) != min_voxels or min_voxels < 1:
        raise ValueError(f'lesion_table: min_voxels must be an integer >= 1, got {min_voxels!r}')
    if int(max_lesions) != max_lesions or not 1 <= max_lesions <= MAX_ROWS:
        raise ValueError(f'lesion_table: max_lesions must be an integer in 1..{MAX_ROWS}, got {max_lesions!r}')
    if int(max_candidates) != max_candidates or not 2 <= max_candidates < 2 ** 31:
        raise ValueError(f'lesion_table: max_candidates must be an integer in 2..2^31-1, got {max_candidates!r}')
    return sp


def _lesion_table_impl(masks, spacing, conn, min_voxels, max_lesions, max_candidates, return_labels):
    """The C ABI calls.  masks (P, D, H, W) uint8 on the device -> (rows_i (P, K, 16) int64, rows_f (P, K, 4) float64, totals (P, 4) int64,
    labels (P, D, H, W) uint8 or an empty tensor), all on the device."""
    if masks.dim() != 4 or masks.dtype != torch.uint8:
        raise ValueError(f'lesion_table: a uint8 (P, D, H, W) stack, got {masks.dtype} {tuple(masks.shape)}')
    P, D, H, W = masks.shape
    if min(P, D, H, W) < 1 or D * H * W > 2 ** 31:
        raise ValueError(f'lesion_table: planes of 1 .. 2^31 voxels, got {(D, H, W)}')
    sp = _check_params(spacing, conn, min_voxels, max_lesions, max_candidates)
    K = int(max_lesions)
    L = _l.lib()
    masks = masks.contiguous()
    dev = masks.device
    rows_i = torch.empty((P, K, 16), device=dev, dtype=torch.int64)
    rows_f = torch.empty((P, K, 4), device=dev, dtype=torch.float64)
    totals = torch.empty((P, 4), device=dev, dtype=torch.int64)
    labels = torch.empty((P, D, H, W) if return_labels else (0,), device=dev, dtype=torch.uint8)
    with torch.cuda.device(dev):
        st = _stream(masks)
        for p0 in range(0, P, MAX_PLANES):
            n = min(MAX_PLANES, P - p0)
            nbytes = L.rsuper_lesion_table_workspace_bytes(n, D, H, W, K)
            ws = torch.empty((nbytes // 8,), device=dev, dtype=torch.int64)
            _l.check(L.rsuper_lesion_table(masks[p0:p0 + n].data_ptr(), n, D, H, W, int(conn), int(min_voxels), K, int(max_candidates), sp[0], sp[1], sp[2],
                                           rows_i[p0:p0 + n].data_ptr(), rows_f[p0:p0 + n].data_ptr(), totals[p0:p0 + n].data_ptr(),
                                           labels[p0:p0 + n].data_ptr() if return_labels else None, ws.data_ptr(), nbytes, st), 'lesion_table')
    return rows_i, rows_f, totals, labels


def _label_overlap_impl(labels_a, labels_b, Ka, Kb):
    """labels_a, labels_b (P, ...) uint8 on the device with the same shape -> counts (P, Ka + 1, Kb + 1) int64 on the device."""
    if labels_a.dtype != torch.uint8 or labels_b.dtype != torch.uint8 or labels_a.shape != labels_b.shape or labels_a.dim() < 2:
        raise ValueError(f'label_overlap: two uint8 (P, ...) label stacks of one shape, got {labels_a.dtype} {tuple(labels_a.shape)} and '
                         f'{labels_b.dtype} {tuple(labels_b.shape)}')
    if not (0 <= Ka <= MAX_ROWS and 0 <= Kb <= MAX_ROWS):
        raise ValueError(f'label_overlap: Ka and Kb in 0..{MAX_ROWS}, got {Ka}, {Kb}')
    if labels_a.device != labels_b.device:
        raise ValueError('label_overlap: both label stacks on one device')
    P = labels_a.shape[0]
    V = labels_a[0].numel()
    if P < 1 or P > 65535 or V < 1:
        raise ValueError(f'label_overlap: 1..65535 planes of at least one voxel, got {tuple(labels_a.shape)}')
    a, b = labels_a.contiguous(), labels_b.contiguous()
    counts = torch.empty((P, Ka + 1, Kb + 1), device=a.device, dtype=torch.int64)
    with torch.cuda.device(a.device):
        _l.check(_l.lib().rsuper_label_overlap(a.data_ptr(), b.data_ptr(), P, V, int(Ka), int(Kb), counts.data_ptr(), _stream(a)), 'label_overlap')
    return counts


_TABLE_OP, _OVERLAP_OP = _library.install_lesion_ops(_lesion_table_impl, _label_overlap_impl)


class LesionTable:
    """The result of `lesion_table`: `rows_i` (P, K, 16) int64, `rows_f` (P, K, 4) float64, `totals` (P, 4) int64 and, when asked for, `labels`
    (P, D, H, W) uint8, on the device; `host()` copies the three small tensors once and keeps the copy.  `single` tells that the input was one
    (D, H, W) plane: the per-plane accessors then default to it."""

    def __init__(self, rows_i, rows_f, totals, labels, shape, spacing, conn, min_voxels, single=False):
        self.rows_i, self.rows_f, self.totals, self.labels = rows_i, rows_f, totals, labels
        self.shape, self.spacing, self.conn, self.min_voxels, self.single = tuple(shape), tuple(float(s) for s in spacing), conn, min_voxels, single
        self._host = None

    @classmethod
    def from_host(cls, rows_i, rows_f, totals, shape, spacing, conn=26, min_voxels=1):
        """A table from host arrays (what a test or a saved table holds); it has no labels."""
        t = cls(None, None, None, None, shape, spacing, conn, min_voxels, single=np.asarray(rows_i).ndim == 2)
        ri, rf, to = np.asarray(rows_i, np.int64), np.asarray(rows_f, np.float64), np.asarray(totals, np.int64)
        t._host = (ri.reshape((-1,) + ri.shape[-2:]), rf.reshape((-1,) + rf.shape[-2:]), to.reshape(-1, 4))
        return t

    def host(self):
        """(rows_i, rows_f, totals) as numpy arrays: one device-to-host copy, made on first use."""
        if self._host is None:
            P, K = self.rows_i.shape[:2]
            flat = torch.cat([self.rows_i.reshape(-1), self.rows_f.reshape(-1).view(torch.int64), self.totals.reshape(-1)]).cpu().numpy()
            self._host = (flat[:P * K * 16].reshape(P, K, 16).copy(), flat[P * K * 16:P * K * 20].view(np.float64).reshape(P, K, 4).copy(),
                          flat[P * K * 20:].reshape(P, 4).copy())
        return self._host

    @property
    def planes(self):
        return self.host()[0].shape[0]

    @property
    def max_lesions(self):
        return self.host()[0].shape[1]

    def plane(self, p):
        """Plane p as a table of its own (views of the same tensors)."""
        t = LesionTable(*(None if v is None else v[p:p + 1] for v in (self.rows_i, self.rows_f, self.totals, self.labels)), self.shape, self.spacing,
                        self.conn, self.min_voxels, single=True)
        t._host = tuple(h[p:p + 1] for h in self.host())
        return t

    def count(self, plane=0):
        """Rows written for the plane (at most max_lesions; totals[plane] holds how many components there were)."""
        return int(self.host()[2][plane, 3])

    def rows(self, plane=0):
        """The plane's lesions as dicts of FIELDS_I (int) and FIELDS_F (float), largest first."""
        ri, rf, _ = self.host()
        return [dict(list(zip(FIELDS_I, (int(v) for v in ri[plane, k]))) + list(zip(FIELDS_F, (float(v) for v in rf[plane, k]))))
                for k in range(self.count(plane))]


def _as_planes(masks, channels):
    """-> ((P, D, H, W) uint8 device tensor, single)."""
    if hasattr(masks, 'packed') and hasattr(masks, 'planes'):          # training.dataset.packed.PackedBits, one sample
        if channels is None:
            raise ValueError('lesion_table: a PackedBits label needs the list of channels to measure')
        if masks.packed.shape[0] != 1:
            raise ValueError('lesion_table: a PackedBits label of one sample')
        chs = [int(c) for c in channels]
        if not chs or min(chs) < 0 or max(chs) >= masks.C:
            raise ValueError(f'lesion_table: channels within 0..{masks.C - 1}, got {channels!r}')
        return masks.planes(chs)[0][chs], False                           # only these planes are inflated (csrc/label_bits.hip unpack_bits_sel)
    if not isinstance(masks, torch.Tensor) or not masks.is_cuda:
        raise _l.RSuperHipError('lesion_table: the masks must be on the MI355X device (no CPU fallback)')
    if channels is not None:
        raise ValueError('lesion_table: channels go with a PackedBits label only')
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8) if masks.is_contiguous() else masks.to(torch.uint8)
    if masks.dtype != torch.uint8 or masks.dim() not in (3, 4):
        raise ValueError(f'lesion_table: uint8 or bool masks (D, H, W) or (P, D, H, W), got {masks.dtype} {tuple(masks.shape)}')
    return (masks.unsqueeze(0), True) if masks.dim() == 3 else (masks, False)


def lesion_table(masks, spacing=(1, 1, 1), conn=26, min_voxels=1, max_lesions=64, max_candidates=65536, return_labels=False, channels=None):
    """The lesions of every plane of `masks`, measured on the device -> LesionTable.

    masks: a uint8 or bool device tensor (D, H, W) or (P, D, H, W), non-zero = foreground; or a one-sample PackedBits label with `channels`, the
    class indices to measure (only those planes are inflated).  spacing: mm per voxel along the three array axes.  Components of fewer than
    min_voxels voxels are dropped (and counted in totals); the max_lesions largest of a plane get rows.  return_labels: also the label volume, 0
    background, k + 1 lesion k, 255 a component without a row.  max_candidates bounds the 3-D diameter search of one lesion (a lesion with more
    candidate voxels gets d3 = NaN and flags bit 0; everything else about it stays exact): an organ-sized false positive cannot stall a run.
    A CPU tensor raises RSuperHipError: there is no host fallback."""
    stack, single = _as_planes(masks, channels)
    sp = _check_params(spacing, conn, min_voxels, max_lesions, max_candidates)
    ri, rf, to, lab = _TABLE_OP(stack, list(sp), int(conn), int(min_voxels), int(max_lesions), int(max_candidates), bool(return_labels))
    return LesionTable(ri, rf, to, lab if return_labels else None, stack.shape[1:], sp, conn, min_voxels, single)


def _need_labels(t, what):
    if t.labels is None:
        raise ValueError(f'{what}: the table has no label volume (lesion_table(..., return_labels=True))')


def match_lesions(pred_table, gt_table, min_overlap=1):
    """Lesion-level matching of two tables of the same planes (both made with return_labels=True).  Per plane a dict:

        overlap     (n_pred, n_gt) int64 array of shared voxels
        pred_to_gt  per predicted lesion the annotated lesion it overlaps most (ties: the lower index), -1 below min_overlap voxels
        gt_to_pred  the reverse
        tp, fn      annotated lesions that some predicted lesion overlaps by at least min_overlap voxels, and the others
        fp          predicted lesions that overlap no annotated lesion by at least min_overlap voxels
        dice        {(i, j): 2 |i & j| / (|i| + |j|)} for every predicted lesion i with pred_to_gt[i] = j

    A voxel of a component without a row (label 255) belongs to no lesion on its side.  One plane in, one dict out; P planes, a list."""
    _need_labels(pred_table, 'match_lesions')
    _need_labels(gt_table, 'match_lesions')
    if pred_table.labels.shape != gt_table.labels.shape:
        raise ValueError(f'match_lesions: label volumes of one shape, got {tuple(pred_table.labels.shape)} and {tuple(gt_table.labels.shape)}')
    if int(min_overlap) != min_overlap or min_overlap < 1:
        raise ValueError(f'match_lesions: min_overlap must be an integer >= 1, got {min_overlap!r}')
    counts = _OVERLAP_OP(pred_table.labels, gt_table.labels, pred_table.max_lesions, gt_table.max_lesions).cpu().numpy()
    out = []
    for p in range(pred_table.planes):
        na, nb = pred_table.count(p), gt_table.count(p)
        ov = counts[p, 1:na + 1, 1:nb + 1]
        va, vb = pred_table.host()[0][p, :na, 1], gt_table.host()[0][p, :nb, 1]
        p2g = [int(ov[i].argmax()) if nb and ov[i].max() >= min_overlap else -1 for i in range(na)]
        g2p = [int(ov[:, j].argmax()) if na and ov[:, j].max() >= min_overlap else -1 for j in range(nb)]
        tp = sum(1 for j in g2p if j >= 0)
        out.append({'overlap': ov.copy(), 'pred_to_gt': p2g, 'gt_to_pred': g2p, 'tp': tp, 'fn': nb - tp, 'fp': sum(1 for j in p2g if j < 0),
                    'dice': {(i, j): 2.0 * int(ov[i, j]) / (int(va[i]) + int(vb[j])) for i, j in enumerate(p2g) if j >= 0}})
    return out[0] if pred_table.single and gt_table.single else out


def locate_lesions(table, segment_planes, names):
    """Per lesion the name of the segment it shares most voxels with, 'u' (the reports' "unknown") when it touches none.  segment_planes: uint8 or
    bool device tensor (S, D, H, W), the planes of one organ's sub-segments, `names` their S names; ties go to the earlier segment.  The table needs
    its labels.  One plane in, a list of names out; P planes, a list of lists (every plane is located in the same segments)."""
    _need_labels(table, 'locate_lesions')
    if not isinstance(segment_planes, torch.Tensor) or not segment_planes.is_cuda:
        raise _l.RSuperHipError('locate_lesions: the segment planes must be on the MI355X device (no CPU fallback)')
    if segment_planes.dim() != 4 or tuple(segment_planes.shape[1:]) != tuple(table.labels.shape[1:]) or segment_planes.shape[0] != len(names):
        raise ValueError(f'locate_lesions: {len(names)} segment planes of shape {tuple(table.labels.shape[1:])}, got {tuple(segment_planes.shape)}')
    seg = (segment_planes != 0).to(torch.uint8)
    P, K = table.planes, table.max_lesions
    per = torch.stack([_OVERLAP_OP(table.labels, seg[s:s + 1].expand(P, -1, -1, -1).contiguous(), K, 1)[:, :, 1] for s in range(len(names))])
    per = per.cpu().numpy()                                                # (S, P, K + 1)
    out = []
    for p in range(P):
        col = per[:, p, 1:table.count(p) + 1]
        out.append([names[int(col[:, k].argmax())] if len(names) and col[:, k].max() > 0 else 'u' for k in range(col.shape[1])])
    return out[0] if table.single else out


def padded_diameters(row, spacing, pad='voxel'):
    """(a, b, c) of a lesion row in mm under the padding convention of lesion_report_rows."""
    if pad not in ('voxel', None):
        raise ValueError(f"pad must be 'voxel' or None, got {pad!r}")
    s0, s1, s2 = (float(s) for s in spacing)
    ip, zp = ((s1 + s2) / 2, s0) if pad == 'voxel' else (0.0, 0.0)
    return row['a'] + ip, row['b'] + ip, row['c'] + zp


def lesion_report_rows(table, organ, spacing=None, location=None, pad='voxel', plane=0):
    """The lesions of one plane as report rows: dicts with 'Standardized Organ' = organ, 'Standardized Location' and 'Tumor Size (mm)' =
    'a x b x c' to one decimal -- the columns training/dataset/reports.py and estimate_tumor_volume read, accepted by the latter as they are.

    location: None ('u' for every lesion, the reports' "unknown"), one name for all, or a list with one name per lesion (locate_lesions).
    spacing: the table's when None.

    Padding.  a, b and c are measured between voxel centres, so a one-voxel lesion measures 0 x 0 x 0 and a lesion that fills a 10 mm cube of 1 mm
    voxels 9 mm along each axis.  A radiologist's calipers span the outer edges.  pad='voxel' (the default) therefore adds one voxel to each
    extent: the mean in-plane spacing (s1 + s2) / 2 to a and b, whose directions are arbitrary in the slice, and s0 to c.  pad=None writes the
    centre-to-centre values."""
    sp = table.spacing if spacing is None else tuple(float(s) for s in spacing)
    rows = table.rows(plane)
    if location is None or isinstance(location, str):
        location = ['u' if location is None else location] * len(rows)
    if len(location) != len(rows):
        raise ValueError(f'lesion_report_rows: {len(location)} locations for {len(rows)} lesions')
    out = []
    for r, loc in zip(rows, location):
        a, b, c = padded_diameters(r, sp, pad)
        out.append({'Standardized Organ': organ, 'Standardized Location': loc, 'Tumor Size (mm)': f'{a:.1f} x {b:.1f} x {c:.1f}'})
    return out


def compare_with_report(table, report_rows, organ, pad='voxel', plane=0):
    """A table against what a report says about `organ` ('liver', 'kidney', 'pancreas': the organ words of estimate_tumor_volume), on the host.

    Reported lesions are the rows estimate_tumor_volume takes for the organ, with its diameters and ellipsoid volumes; predicted lesions are the
    plane's rows with their padded diameters (lesion_report_rows) and voxel volume voxels * s0 * s1 * s2.  Both lists are ordered by their largest
    diameter, largest first, and paired by rank.  Returns {'n_pred', 'n_report', 'pairs': [{'pred_diameter', 'report_diameter', 'diameter_error',
    'pred_volume', 'report_volume', 'volume_error'}, ...]} with absolute errors in mm and mm^3; unpaired lesions only show in the counts."""
    from ..training.dataset.augmented import estimate_tumor_volume
    vols, diam = estimate_tumor_volume(report_rows, [organ])
    reported = sorted(((max(float(v) for v in d), float(vol)) for vol, d in zip(vols, diam.tolist()) if max(d) > 0), reverse=True)
    voxel = table.spacing[0] * table.spacing[1] * table.spacing[2]
    pred = sorted(((max(padded_diameters(r, table.spacing, pad)), r['voxels'] * voxel) for r in table.rows(plane)), reverse=True)
    pairs = [{'pred_diameter': pd, 'report_diameter': rd, 'diameter_error': abs(pd - rd), 'pred_volume': pv, 'report_volume': rv,
              'volume_error': abs(pv - rv)} for (pd, pv), (rd, rv) in zip(pred, reported)]
    return {'n_pred': len(pred), 'n_report': len(reported), 'pairs': pairs}


def lesion_csv_rows(table, case_id, class_name, locations=None, plane=0):
    """The plane's lesions as CSV_COLUMNS dicts of strings (floats in repr form, which reads back to the same value)."""
    rows = table.rows(plane)
    if locations is None:
        locations = [''] * len(rows)
    out = []
    for k, (r, loc) in enumerate(zip(rows, locations)):
        d = {'BDMAP_ID': case_id, 'class': class_name, 'lesion': str(k + 1), 'location': loc}
        d.update({f: str(r[f]) for f in FIELDS_I})
        d.update({f: repr(r[f]) for f in FIELDS_F})
        out.append(d)
    return out


def csv_text(rows, header=True):
    """CSV_COLUMNS rows as text, '\\n' line ends."""
    import csv
    import io
    buf = io.StringIO()
    w = csv.DictWriter(buf, fieldnames=list(CSV_COLUMNS), lineterminator='\n')
    if header:
        w.writeheader()
    w.writerows(rows)
    return buf.getvalue()


def append_csv(path, rows):
    """Append the rows to `path`; the header goes in front of a new file (also of an empty table: the file then tells that the run measured)."""
    import os
    new = not os.path.exists(path)
    with open(path, 'a', newline='') as f:
        f.write(csv_text(rows, header=new))


def segment_classes(lesion_class, class_list):
    """The sub-segment planes of a lesion class's organ among `class_list`: the non-lesion classes named '<organ>_...' (liver_segment_1,
    pancreas_head, kidney_left, ...), organ as postprocess.organ_name gives it."""
    from .postprocess import organ_name
    organ = organ_name(lesion_class)
    return [c for c in class_list if 'lesion' not in c and c.startswith(organ + '_')]
