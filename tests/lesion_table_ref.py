"""scipy / numpy restatement of the lesion table (csrc/lesion_table.hip, rsuper_amd.inference.lesions): scipy.ndimage.label for the components and
brute force over ALL voxels of a component for the diameters -- no pruning, so nothing here depends on the kernel's candidate rule.  Squared distances
are the float64 expression (q0 * dz**2 + q1 * dy**2) + q2 * dx**2 with q_i = s_i * s_i, every product and sum rounded on its own as numpy does; the
canonical pair is the lexicographically smallest (p, q), p <= q, among the pairs that attain the maximum."""
import numpy as np
from scipy import ndimage

STRUCT = {6: ndimage.generate_binary_structure(3, 1), 26: np.ones((3, 3, 3), bool)}
ROWS = 4096        # rows of the pairwise matrix held at once


def sq_dist(a, b, q):
    """(len(a), len(b)) float64 squared distances between integer coordinates a (n, 3) and b (m, 3)."""
    d = a[:, None, :].astype(np.float64) - b[None, :, :].astype(np.float64)
    return (q[0] * d[..., 0] ** 2 + q[1] * d[..., 1] ** 2) + q[2] * d[..., 2] ** 2


def far_pair(coords, lin, q):
    """(max squared distance, p, q) over all pairs of a voxel set given in C order (lin ascending)."""
    best, bp, bq = -1.0, -1, -1
    for r0 in range(0, len(lin), ROWS):
        sq = sq_dist(coords[r0:r0 + ROWS], coords, q)
        m = sq.max()
        if m > best:                                   # rows ascend, so an equal maximum further down has a larger p
            i, j = np.argwhere(sq == m)[0]             # row-major: the smallest p, then the smallest q; symmetry puts q >= p
            best, bp, bq = float(m), int(lin[r0 + i]), int(lin[j])
    assert bp <= bq
    return best, bp, bq


def measure(coords, lin, spacing, shape):
    """One component (coords (n, 3) in C order, lin its linear indices) -> (16 ints, 4 floats)."""
    s = np.asarray(spacing, np.float64)
    q = s * s
    z, y, x = coords[:, 0], coords[:, 1], coords[:, 2]
    k3, p3, q3 = far_pair(coords, lin, q)
    ka, pa, qa = -1.0, -1, -1
    for zz in np.unique(z):                            # ascending: a tie between slices stays with the lower one
        sel = z == zz
        k, p, qq = far_pair(coords[sel], lin[sel], q)
        if k > ka:
            ka, pa, qa = k, p, qq
    a = np.sqrt(np.float64(ka))
    b = 0.0
    if ka > 0:
        za, ya, xa = np.unravel_index(pa, shape)
        _, yb, xb = np.unravel_index(qa, shape)
        sel = z == za
        ey, ex = (yb - ya) * s[1], (xb - xa) * s[2]
        t = ey * (x[sel] * s[2]) - ex * (y[sel] * s[1])
        b = float((t.max() - t.min()) / a)
    ints = [int(lin[0]), len(lin), int(z.min()), int(y.min()), int(x.min()), int(z.max()), int(y.max()), int(x.max()), int(z.sum()), int(y.sum()),
            int(x.sum()), p3, q3, pa, qa, 0]
    return ints, [float(np.sqrt(np.float64(k3))), float(a), b, float((z.max() - z.min()) * s[0])]


def table(mask, spacing=(1.0, 1.0, 1.0), conn=26, min_voxels=1, max_lesions=64):
    """One (D, H, W) plane -> {'totals' (4,), 'rows_i' (max_lesions, 16) int64, 'rows_f' (max_lesions, 4) float64, 'labels' uint8}."""
    mask = np.asarray(mask) != 0
    lab, n = ndimage.label(mask, structure=STRUCT[conn])
    flat = lab.ravel()
    order = np.argsort(flat, kind='stable')
    order = order[np.searchsorted(flat[order], 1):]    # foreground voxels grouped by component, C order inside each
    bounds = np.searchsorted(flat[order], np.arange(1, n + 2))
    comps = [order[bounds[i]:bounds[i + 1]] for i in range(n)]
    kept = sorted((c for c in comps if len(c) >= min_voxels), key=lambda c: (-len(c), c[0]))
    rows_i, rows_f = np.zeros((max_lesions, 16), np.int64), np.zeros((max_lesions, 4), np.float64)
    labels = np.where(mask, 255, 0).astype(np.uint8).ravel()
    for k, lin in enumerate(kept[:max_lesions]):
        coords = np.stack(np.unravel_index(lin, mask.shape), 1)
        rows_i[k], rows_f[k] = measure(coords, lin, spacing, mask.shape)
        labels[lin] = k + 1
    totals = np.array([len(kept), n - len(kept), int(mask.sum()), min(len(kept), max_lesions)], np.int64)
    return {'totals': totals, 'rows_i': rows_i, 'rows_f': rows_f, 'labels': labels.reshape(mask.shape)}


def tables(masks, **kw):
    """(P, D, H, W) -> the stacked arrays of `table` per plane."""
    ts = [table(m, **kw) for m in masks]
    return {k: np.stack([t[k] for t in ts]) for k in ts[0]}


def overlap(a, b, Ka, Kb):
    """Joint histogram of two label volumes; values above Ka / Kb count nowhere, [0, 0] stays 0."""
    a, b = np.asarray(a).ravel().astype(np.int64), np.asarray(b).ravel().astype(np.int64)
    ok = (a <= Ka) & (b <= Kb) & ((a | b) != 0)
    out = np.zeros((Ka + 1, Kb + 1), np.int64)
    np.add.at(out, (a[ok], b[ok]), 1)
    return out


# ------------------------------------------------------------------------------------------------ inputs shared by the CPU and the GPU tests
def blobs(shape, seed=0, quantile=0.85, sigma=1.5):
    """Smoothed-noise blobs: gaussian_filter(standard_normal, sigma) above its quantile."""
    g = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), sigma)
    return (g > np.quantile(g, quantile)).astype(np.uint8)


def salt(shape, seed, p=0.05):
    return (np.random.default_rng(seed).random(shape) < p).astype(np.uint8)


def ball(shape, centre, r):
    g = np.indices(shape)
    return (sum((g[i] - centre[i]) ** 2 for i in range(3)) <= r * r).astype(np.uint8)


def diagonal(shape, n):
    """n voxels (i, i, i): one component at 26-connectivity, n at 6."""
    m = np.zeros(shape, np.uint8)
    i = np.arange(n)
    m[i, i, i] = 1
    return m
