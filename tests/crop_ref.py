"""numpy restatement of what csrc/crop.hip computes: the per-chunk and total voxel counts of a bit-packed label, the k-th set voxel of a column in
row-major order, and the box crop of a zero-padded volume.  tests/test_crop_cpu.py pins it to tests/golden/crop.npz (the unmodified reference);
tests/test_gpu_crop.py compares the kernels with it bit for bit."""
import numpy as np

CHUNK = 16384


def column_masks(packed, C):
    """packed (P, D, H, W) u8 -> bool (C + 1, D, H, W): the C class masks of np.unpackbits and, last, the background (every byte zero)."""
    bits = np.unpackbits(packed, axis=0)[:C].astype(bool)
    return np.concatenate([bits, (packed == 0).all(0)[None]], 0)


def totals(packed, C):
    """(C + 1,) int64: voxels of every class, then of the background."""
    return column_masks(packed, C).reshape(C + 1, -1).sum(1).astype(np.int64)


def chunk_table(packed, C, chunk=CHUNK):
    """(chunks, C + 1) int32: the counts per run of `chunk` consecutive voxels in row-major order."""
    m = column_masks(packed, C).reshape(C + 1, -1)
    n = -(-m.shape[1] // chunk)
    m = np.pad(m, ((0, 0), (0, n * chunk - m.shape[1])))
    return m.reshape(C + 1, n, chunk).sum(2).T.astype(np.int32)


def kth_voxel(packed, C, column, k):
    """(z, y, x) of the k-th voxel of `column` in row-major order: np.argwhere(mask)[k] = torch.nonzero(mask)[k]."""
    return [int(v) for v in np.argwhere(column_masks(packed, C)[column])[k]]


def padded(a, pad):
    """pad_volume_pair on the last three axes: zeros up to max(size, pad), (padded - size) // 2 of them on the low side."""
    if pad is None:
        return a
    width = [(0, 0)] * (a.ndim - 3)
    for s, p in zip(a.shape[-3:], pad):
        t = max(0, int(p) - s)
        width.append((t // 2, t - t // 2))
    return np.pad(a, width)


def box(a, size, origin, pad=None):
    z, y, x = origin
    return padded(a, pad)[..., z:z + size[0], y:y + size[1], x:x + size[2]]


def shifted_origin(center, crop, offset, size):
    """crop_around_coordinate_3d 'small_rnd_shift' (:525-542)."""
    return [int(np.clip(c - s // 2 + o, 0, n - s)) for c, s, o, n in zip(center, crop, offset, size)]
