"""numpy-only restatement of the surface-distance metrics (metric/metrics.py of the reference): the yardstick of
tests/test_gpu_surface_metrics.py for cases drawn at test time.  No scipy: it runs wherever numpy does.

    neighbour_codes            correlate(mask, [[[128, 64], [32, 16]], [[8, 4], [2, 1]]], mode='constant') on the corner grid, by shifted adds
    nearest_distances          distance of every query corner to the nearest target corner, brute force in chunks (float64)
    surface_distances          the reference's dict, sorted by (distance, area); the area table is an argument
    average_surface_distance, robust_hausdorff, surface_overlap, surface_dice, dice      the statistics, with the reference's conventions
"""
import numpy as np

KERNEL = np.array([[[128, 64], [32, 16]], [[8, 4], [2, 1]]])


def neighbour_codes(mask):
    """(D, H, W) -> (D + 1, H + 1, W + 1) uint8: corner (i, j, k) sees voxels i-1..i, j-1..j, k-1..k, zero outside."""
    m = np.pad(np.asarray(mask) != 0, 1).astype(np.uint8)
    D, H, W = (s + 1 for s in np.asarray(mask).shape)
    code = np.zeros((D, H, W), np.uint8)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                code += np.uint8(KERNEL[a, b, c]) * m[a:a + D, b:b + H, c:c + W]
    return code


def borders(code):
    return (code != 0) & (code != 255)


def nearest_distances(queries, targets, spacing, chunk=1 << 22):
    """queries (n, 3), targets (m, 3) corner indices -> (n,) float64 distance to the nearest target: sqrt(min sum((spacing * delta) ** 2))."""
    s = np.asarray(spacing, np.float64)
    q, t = np.asarray(queries, np.float64), np.asarray(targets, np.float64)     # index differences are exact; the spacing scales them
    if len(t) == 0:
        return np.full(len(q), np.inf)
    out = np.empty(len(q))
    rows = max(1, chunk // len(t))
    for i in range(0, len(q), rows):
        d = (q[i:i + rows, None, :] - t[None, :, :]) * s
        out[i:i + rows] = np.sqrt((d * d).sum(-1).min(1))
    return out


def surface_distances(mask_gt, mask_pred, spacing, table):
    cg, cp = neighbour_codes(mask_gt), neighbour_codes(mask_pred)
    bg, bp = np.argwhere(borders(cg)), np.argwhere(borders(cp))
    table = np.asarray(table, np.float64)

    def side(b, other, code):
        d, a = nearest_distances(b, other, spacing), table[code[tuple(b.T)]] if len(b) else np.zeros(0)
        o = np.lexsort((a, d))
        return d[o], a[o]

    dg, ag = side(bg, bp, cg)
    dp, ap = side(bp, bg, cp)
    return {'distances_gt_to_pred': dg, 'distances_pred_to_gt': dp, 'surfel_areas_gt': ag, 'surfel_areas_pred': ap}


def average_surface_distance(sd):
    with np.errstate(invalid='ignore', divide='ignore'):
        return (np.sum(sd['distances_gt_to_pred'] * sd['surfel_areas_gt']) / np.sum(sd['surfel_areas_gt']),
                np.sum(sd['distances_pred_to_gt'] * sd['surfel_areas_pred']) / np.sum(sd['surfel_areas_pred']))


def _percentile(d, a, percent):
    if len(d) == 0:
        return np.inf
    cum = np.cumsum(a) / np.sum(a)
    return d[min(int(np.searchsorted(cum, percent / 100.0)), len(d) - 1)]


def robust_hausdorff(sd, percent):
    return max(_percentile(sd['distances_gt_to_pred'], sd['surfel_areas_gt'], percent),
               _percentile(sd['distances_pred_to_gt'], sd['surfel_areas_pred'], percent))


def surface_overlap(sd, tol):
    with np.errstate(invalid='ignore', divide='ignore'):
        return (np.sum(sd['surfel_areas_gt'][sd['distances_gt_to_pred'] <= tol]) / np.sum(sd['surfel_areas_gt']),
                np.sum(sd['surfel_areas_pred'][sd['distances_pred_to_gt'] <= tol]) / np.sum(sd['surfel_areas_pred']))


def surface_dice(sd, tol):
    with np.errstate(invalid='ignore', divide='ignore'):
        og = np.sum(sd['surfel_areas_gt'][sd['distances_gt_to_pred'] <= tol])
        op = np.sum(sd['surfel_areas_pred'][sd['distances_pred_to_gt'] <= tol])
        return (og + op) / (np.sum(sd['surfel_areas_gt']) + np.sum(sd['surfel_areas_pred']))


def dice(mask_gt, mask_pred):
    g, p = np.asarray(mask_gt) != 0, np.asarray(mask_pred) != 0
    s = int(g.sum()) + int(p.sum())
    return np.nan if s == 0 else 2 * int((g & p).sum()) / s


def label_dice(pred, target, C, block_size=None):
    """calculate_dice / calculate_dice_split of metric/utils.py on integer label vectors, float32 as in the reference."""
    pred, target = np.asarray(pred).reshape(-1), np.asarray(target).reshape(-1)
    blocks = [(0, len(pred))] if block_size is None else [(s, min(s + block_size, len(pred))) for s in range(0, len(pred), block_size)]
    ti, ts = np.zeros(C, np.float32), np.zeros(C, np.float32)
    for s, e in blocks:
        p, t = pred[s:e], target[s:e]
        inter = np.bincount(t[p == t], minlength=C).astype(np.float32)
        summ = (np.bincount(p, minlength=C) + np.bincount(t, minlength=C)).astype(np.float32) + np.float32(1e-5)
        ti += inter
        ts += summ
    if block_size is None:
        return 2 * ti / ts, ti, ts
    return 2 * ti / (ts + np.float32(1e-5)), ti, ts
