"""numpy + scipy restatement of the report-guided pseudo-label refinement, for the CPU tests and tools/bench_pseudo_labels.py (product code never imports
it), and the synthetic volumes of tests/golden/pseudo_labels.npz that are cheap to rebuild from a formula.

candidates() states the loop the way the device kernels run it: every comparison in float32, the threshold one float32 product, 26-connected
components, the first C-order voxel of the maximum as the seed.  It also returns the number of labelling passes."""
import itertools

import numpy as np

BOX26 = np.ones((3, 3, 3), dtype=bool)
# the 13 neighbour directions that follow a voxel in C order (their negatives precede it)
DIRECTIONS = [d for d in itertools.product((-1, 0, 1), repeat=3) if d > (0, 0, 0)]
SMOOTH_SHAPES = [(13, 21, 37), (24, 40, 72), (33, 9, 65)]
# (n_lesions, peak_cut, min_voxels, min_peak) of every smooth_* call
SMOOTH_PARAMS = [(1, 0.40, 11, 0.01), (4, 0.40, 11, 0.01), (60, 0.40, 11, 0.01), (6, 0.8, 3, 0.01), (3, 0.1, 1, 0.3)]
REJECT_CALLS = [(1, 11), (2, 11), (3, 11), (2, 10)]        # (n_lesions, min_voxels) on the `reject` volume
BRIDGE_PEAK = np.float32(0.6369617)                          # float32(float32(0.4) * p) = 0.25478467 < 0.4 * p = 0.25478467941...


def candidates(prob, n_lesions, peak_cut=0.40, min_voxels=11, min_peak=0.01):
    """-> (mask uint8, kept, iterations)."""
    from scipy import ndimage
    prob = np.asarray(prob)
    assert prob.dtype == np.float32 and prob.ndim == 3
    cut, floor = np.float32(peak_cut), np.float32(min_peak)
    left = prob.copy()
    mask = np.zeros(prob.shape, np.uint8)
    kept = passes = 0
    while kept < n_lesions:
        seed = int(np.argmax(left))                          # first maximum in C order
        peak = left.reshape(-1)[seed]
        if peak < floor:
            break
        thr = np.float32(cut * peak)                         # float32 * float32: one rounding
        lab, _ = ndimage.label(left >= thr, structure=BOX26)
        passes += 1
        comp = lab == lab.reshape(-1)[seed]
        if int(np.count_nonzero(comp)) >= min_voxels:
            mask[comp] = 1
            kept += 1
        left[comp] = 0
    return mask, kept, passes


def direction_volume(d):
    """(16, 16, 64): twelve voxels at (8, 8, 32) + t * d, t = -6 .. 5, values 0.9 - 0.01 * (t + 6): the staircase crosses z = 8, y = 8 and x = 32."""
    v = np.zeros((16, 16, 64), np.float32)
    for t in range(-6, 6):
        v[8 + t * d[0], 8 + t * d[1], 32 + t * d[2]] = np.float32(0.9 - 0.01 * (t + 6))
    return v


def ties_volume():
    v = np.zeros((9, 9, 34), np.float32)
    v[0:2, 0:3, 0:2] = 0.8
    v[6:9, 6:9, 30:34] = 0.8
    return v


def reject_volume():
    v = np.zeros((9, 10, 36), np.float32)
    v[1, 1, 1:11] = 0.9
    v[4, 8, 20:31] = 0.7
    v[7:9, 2:6, 30:35] = 0.5
    return v


def bridge_volume():
    """Two runs of three voxels at BRIDGE_PEAK joined by one voxel equal to the float32 threshold (below the float64 product)."""
    p = BRIDGE_PEAK
    thr = np.float32(np.float32(0.4) * p)
    assert float(thr) < 0.4 * float(p)
    v = np.zeros((4, 4, 8), np.float32)
    v[1, 1, 0:3] = p
    v[1, 1, 3] = thr
    v[1, 1, 4:7] = p
    return v


def minpeak_volume(below):
    """A 12-voxel block at exactly float32(0.01), or at the next float32 below it."""
    p = np.float32(0.01)
    if below:
        p = np.nextafter(p, np.float32(0))
    v = np.zeros((4, 5, 6), np.float32)
    v[0:2, 0:3, 0:2] = p
    return v


def plateau_volume():
    """(9, 9, 70): one line x = 2 .. 65 with two flat-topped peaks; the first component takes x = 2 .. 33, the second the rest."""
    v = np.zeros((9, 9, 70), np.float32)
    x = np.arange(2, 34)
    v[4, 4, 2:34] = np.minimum(0.9, 0.95 - 0.01 * np.abs(x - 10)).astype(np.float32)
    x = np.arange(34, 66)
    v[4, 4, 34:66] = np.minimum(0.3, 0.31 - 0.002 * np.abs(x - 50)).astype(np.float32)
    return v


def snake_support():
    """(17, 18, 70) bool: one serpentine path of 5759 voxels.  Even z: the rows y = 0, 2, .., 16 in full, joined at alternating ends through the odd rows,
    and a tail voxel in row 17; odd z: one voxel above that tail.  Rows two apart do not touch, so the path is the only way through."""
    s = np.zeros((17, 18, 70), bool)
    for z in range(0, 17, 2):
        s[z, 0:17:2, :] = True
        for y in range(1, 17, 2):
            s[z, y, 69 if (y // 2) % 2 == 0 else 0] = True
        s[z, 17, 0] = True
        if z + 1 < 17:
            s[z + 1, 17, 0] = True
    return s


def snake_volume():
    s = snake_support()
    idx = np.arange(s.size, dtype=np.float64).reshape(s.shape)
    return np.where(s, 0.6 + 0.3 * idx / s.size, 0.0).astype(np.float32)


def smooth_volume(shape, seed):
    """Lightly smoothed noise stretched to [0, 0.97] and cubed: a few large blobs and many crumbs below min_voxels, so a high lesion count takes a
    few hundred passes and the smallest volume runs dry before 60 are kept."""
    from scipy import ndimage
    g = ndimage.gaussian_filter(np.random.default_rng(seed).standard_normal(shape), 0.8, mode='wrap')
    g = (g - g.min()) / (g.max() - g.min())
    return (0.97 * g ** 3).astype(np.float32)


def speckle_volume(seed=9):
    return (np.random.default_rng(seed).random((16, 24, 40)) ** 8).astype(np.float32)


def merge_numpy(organs, organ_names, lesion_masks, label_names):
    """to_npz's stacking in numpy: sorted labels, organ planes by name, lesion planes from the masks or zeros."""
    planes = []
    for label in sorted(label_names):
        if label in organ_names:
            planes.append(organs[list(organ_names).index(label)])
        else:
            assert 'lesion' in label
            planes.append(lesion_masks[label] if label in lesion_masks else np.zeros_like(organs[0]))
    return np.stack(planes).astype(np.uint8)
