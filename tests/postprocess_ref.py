"""numpy-only restatement of the prediction post-processing (predict_abdomenatlas.py postprocess_npz / keep_largest_component) and of
eval_AUC.detection: the yardstick of tests/test_gpu_postprocess.py.  No scipy: it runs wherever numpy does.

    zoom(x, factors)           ndimage.zoom(order=1): align-corners trilinear in float64, output side round(n * f), 0 beyond the last sample
    levels / detection         the per-threshold erode / dilate / AND chain as one level pass: min(max5(min3(L)), L) > t
    label_min_root             6-connected labelling, every voxel labelled with the smallest linear index of its component
    largest_component          keep_largest_component, ties to the first component in C order, all ones when empty
    organ_mask                 the lesion * dilated-organ rule of postprocess_npz
"""
import numpy as np

THRESHOLDS = (0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8, 0.9)


def zoom_shape(shape, factors):
    return tuple(int(round(float(n) * float(f))) for n, f in zip(shape, factors))


def _axis(n_in, n_out):
    """Per output index: lower / upper input index, upper weight (input coordinate o * (n_in - 1) / (n_out - 1), 0 when n_out == 1) and
    whether the coordinate lies inside [0, n_in - 1] -- ndimage's 'constant' mode gives 0 beyond it, which happens to the last output index
    whenever (n_out - 1) * s rounds above n_in - 1."""
    s = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    c = np.arange(n_out, dtype=np.float64) * s
    inside = c <= n_in - 1
    i0 = np.minimum(np.floor(c).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, c - i0, inside


def zoom(x, factors):
    """ndimage.zoom(x, factors, order=1) for a 3-D array: value * wz * wy * wx summed over the 8 corners in float64."""
    x = np.asarray(x, dtype=np.float64)
    out = zoom_shape(x.shape, factors)
    (z0, z1, fz, iz), (y0, y1, fy, iy), (x0, x1, fx, ix) = (_axis(n, m) for n, m in zip(x.shape, out))
    zi, yi, xi = (z0, z1), (y0, y1), (x0, x1)
    wz, wy, wx = (1.0 - fz, fz), (1.0 - fy, fy), (1.0 - fx, fx)
    t = np.zeros(out, np.float64)
    for a in range(2):
        for b in range(2):
            for c in range(2):
                v = x[zi[a][:, None, None], yi[b][None, :, None], xi[c][None, None, :]]
                t += v * wz[a][:, None, None] * wy[b][None, :, None] * wx[c][None, None, :]
    return np.where(iz[:, None, None] & iy[None, :, None] & ix[None, None, :], t, 0.0)


def levels(v, thresholds):
    """Number of thresholds each value exceeds (`value > t` in float64)."""
    L = np.zeros(v.shape, np.int32)
    for t in thresholds:
        L += (v > float(t))
    return L


def _box(a, k, fill, op):
    """k x k x k box min / max by shifted views, `fill` outside the volume (separable)."""
    r = k // 2
    for ax in range(3):
        pad = [(0, 0)] * 3
        pad[ax] = (r, r)
        p = np.pad(a, pad, constant_values=fill)
        n = a.shape[ax]
        out = None
        for s in range(k):
            sl = [slice(None)] * 3
            sl[ax] = slice(s, s + n)
            v = p[tuple(sl)]
            out = v.copy() if out is None else op(out, v)
        a = out
    return a


def final_levels(L):
    """min(max5(min3(L)), L): min3 with level 0 outside the volume (binary_erosion's border), max5 over the volume."""
    e = _box(L, 3, 0, np.minimum)
    m = _box(e, 5, 0, np.maximum)        # e >= 0: a 0 fill adds nothing to the maximum
    return np.minimum(m, L)


def detection(array, spacing=(1, 1, 1), thresholds=THRESHOLDS, erode=True):
    """eval_AUC.detection on an array: ({threshold: volume}, max_prob)."""
    v = zoom(array, [float(s) for s in spacing])
    L = levels(v, thresholds)
    F = final_levels(L) if erode else L
    ths = [float(t) for t in thresholds]
    order = sorted(ths)
    vols = {t: int((F > order.index(float(t))).sum()) for t in thresholds}
    return vols, float(v.max())


def label_min_root(mask):
    """6-connected labelling of mask > 0 by vectorised union-find: every face edge between two foreground voxels hooks the larger of its two
    roots below the smaller (np.minimum.at), then full path compression; repeated until no edge joins two roots.  Parents only ever point
    to smaller indices, so a root is the smallest linear index of its component.  Foreground voxels get that index, background -1."""
    m = np.asarray(mask) > 0
    shape = m.shape
    flat = m.ravel()
    idx = np.flatnonzero(flat)                               # foreground voxels; their rank order is the linear order
    lab = np.full(flat.size, -1, np.int64)
    if idx.size == 0:
        return lab.reshape(shape)
    rank = np.full(flat.size, -1, np.int64)
    rank[idx] = np.arange(idx.size)
    lin = np.arange(flat.size).reshape(shape)
    ea, eb = [], []
    for ax in range(3):
        lo = [slice(None)] * 3
        hi = [slice(None)] * 3
        lo[ax], hi[ax] = slice(0, -1), slice(1, None)
        both = m[tuple(lo)] & m[tuple(hi)]
        ea.append(rank[lin[tuple(hi)][both]])
        eb.append(rank[lin[tuple(lo)][both]])
    ea, eb = np.concatenate(ea), np.concatenate(eb)
    parent = np.arange(idx.size)
    while ea.size:
        ra, rb = parent[ea], parent[eb]
        cross = ra != rb
        ea, eb, ra, rb = ea[cross], eb[cross], ra[cross], rb[cross]
        if not ea.size:
            break
        np.minimum.at(parent, np.maximum(ra, rb), np.minimum(ra, rb))
        while True:                                          # full compression: every parent is a root again
            pp = parent[parent]
            if np.array_equal(pp, parent):
                break
            parent = pp
    lab[idx] = idx[parent]
    return lab.reshape(shape)


def largest_component(mask):
    """keep_largest_component: uint8 0/1 of the largest 6-connected component of mask > 0; ties -> smallest root; empty -> all ones."""
    lab = label_min_root(mask)
    fg = lab >= 0
    if not fg.any():
        return np.ones(lab.shape, np.uint8)
    sizes = np.bincount(lab[fg].ravel())
    root = int(np.argmax(sizes))                             # first maximum = smallest root
    return (lab == root).astype(np.uint8)


def organ_name(lesion_class):
    return lesion_class.split('_')[0].replace('pancreatic', 'pancreas')


def organ_of(lesion_class, organs):
    """Organ planes of a lesion class: list of names, or None for the all-ones bone / breast mask; KeyError when the organ is absent."""
    name = organ_name(lesion_class)
    table = {'kidney': ['kidney_right', 'kidney_left'], 'adrenal': ['adrenal_gland_right', 'adrenal_gland_left'],
             'lung': ['lung_right', 'lung_left'], 'uterus': ['prostate'], 'gallbladder': ['gall_bladder']}
    if name in ('bone', 'breast'):
        organs['prostate']                                   # noqa: B018  (KeyError as the reference's ones_like(pred_dict['prostate']))
        return None
    planes = table.get(name, [name])
    for p in planes:
        organs[p]                                            # noqa: B018
    return planes


def dilate3(b):
    return _box(b.astype(np.uint8), 3, 0, np.maximum)


def postprocess(pred, classes, organ_mask_on_lesion=True, connected_components=False):
    """postprocess_npz on a (C, D, H, W) uint8 / float32 array: {name: plane}."""
    organs = {n: pred[i] for i, n in enumerate(classes) if 'lesion' not in n}
    out = dict(organs)
    for i, n in enumerate(classes):
        if 'lesion' not in n:
            continue
        p = pred[i]
        if organ_mask_on_lesion:
            planes = organ_of(n, organs)
            if planes is None:
                o = np.ones_like(organs['prostate'], dtype=np.uint8)
            elif len(planes) == 2:
                o = organs[planes[0]] + organs[planes[1]]         # uint8 wraps, float32 adds in float32
            else:
                o = organs[planes[0]]
            o = dilate3(o > 0.5).astype(p.dtype)
            p = o * p
        if connected_components:
            p = largest_component(p)
        out[n] = p
    return out
