"""numpy restatement of the whole-CT preprocessing and the class-stack resampler (csrc/resample.hip, inference/preprocess.py,
inference/resample.py): the yardstick for shapes that have no fixture.  tests/test_resample_cpu.py pins it to the reference's own outputs in
tests/golden/resample.npz.

    nearest    scale = (float)n_in / (float)n_out;  src = min((int)floorf((float)dst * scale), n_in - 1)
    trilinear  scale = n_out > 1 ? (float)(n_in - 1) / (float)(n_out - 1) : 0;  s = scale * (float)dst;  i0 = min((int)s, n_in - 1);
               i1 = i0 + (i0 < n_in - 1);  l1 = s - (float)i0;  l0 = 1 - l1

with the index and weight arithmetic in float32; the interpolation itself runs in `dtype` (float64: the exact_* evaluation with the float32
weights; float32: the kernel's own order, lerps in x, y, z as l0 * a + l1 * b).
"""
import numpy as np

CLIP = (-991.0, 500.0)


def axis_nearest(n_in, n_out):
    scale = np.float32(n_in) / np.float32(n_out)
    dst = np.arange(n_out, dtype=np.float32)
    return np.minimum(np.floor(dst * scale).astype(np.int64), n_in - 1)


def axis_linear(n_in, n_out):
    scale = np.float32(n_in - 1) / np.float32(n_out - 1) if n_out > 1 else np.float32(0)
    s = scale * np.arange(n_out, dtype=np.float32)
    i0 = np.minimum(s.astype(np.int64), n_in - 1)
    i1 = i0 + (i0 < n_in - 1)
    l1 = s - i0.astype(np.float32)
    l0 = np.float32(1) - l1
    assert l0.dtype == np.float32 and l1.dtype == np.float32
    return i0, i1, l0, l1


def resample(x, out_size, mode, dtype=np.float64):
    """x (C, D, H, W) -> (C, Do, Ho, Wo).  nearest keeps x's dtype; trilinear returns `dtype`."""
    x = np.asarray(x)
    assert x.ndim == 4
    D, H, W = x.shape[1:]
    Do, Ho, Wo = out_size
    if mode == 'nearest':
        return x[:, axis_nearest(D, Do)][:, :, axis_nearest(H, Ho)][:, :, :, axis_nearest(W, Wo)]
    assert mode == 'trilinear'
    v = x.astype(dtype)
    z0, z1, lz0, lz1 = axis_linear(D, Do)
    y0, y1, ly0, ly1 = axis_linear(H, Ho)
    x0, x1, lx0, lx1 = axis_linear(W, Wo)
    a = lx0.astype(dtype) * v[..., x0] + lx1.astype(dtype) * v[..., x1]                                           # x
    b = ly0.astype(dtype)[:, None] * a[:, :, y0] + ly1.astype(dtype)[:, None] * a[:, :, y1]                        # y
    return lz0.astype(dtype)[:, None, None] * b[:, z0] + lz1.astype(dtype)[:, None, None] * b[:, z1]              # z


def new_size(old_spacing, old_size, new_spacing):
    """z, y, x output size of resample_image_with_gpu for new_size=None; the arguments are in x, y, z order."""
    new_spacing = np.array(new_spacing)[::-1]
    old_spacing = np.array(old_spacing)[::-1]
    old_size = np.array(old_size, dtype=np.float32)[::-1]
    return (old_size * (old_spacing / new_spacing)).round().astype(int).tolist()


def pad_geometry(shape, training_size):
    """(output shape, offset of the input inside it, original_idx) of pad_to_training_size: F.pad counts its pairs from the last axis, so a short
    z widens x and a short x widens z while the recorded ranges keep their own names."""
    z, y, x = shape
    d = [(t + 2 - n) // 2 if n < t else 0 for n, t in zip(shape, training_size)]
    return (z + 2 * d[2], y + 2 * d[1], x + 2 * d[0]), (d[2], d[1], d[0]), [d[0], d[0] + z, d[1], d[1] + y, d[2], d[2] + x]


def pad(x, training_size):
    shape, off, idx = pad_geometry(x.shape, training_size)
    out = np.zeros(shape, x.dtype)
    out[off[0]:off[0] + x.shape[0], off[1]:off[1] + x.shape[1], off[2]:off[2] + x.shape[2]] = x
    return out, idx


def zscore(x, clip=CLIP):
    """float64 evaluation: (exact z-score, mean, unbiased std) of clip(x)."""
    c = np.clip(np.asarray(x, np.float64), clip[0], clip[1])
    n = c.size
    mean = c.sum() / n
    with np.errstate(invalid='ignore', divide='ignore'):
        std = np.sqrt(((c * c).sum() - n * mean * mean) / (n - 1))
        return (c - mean) / std, mean, std


def zscore_bound(x, mean, std, clip=CLIP):
    """4 * 2^-24 * (max|clip(x)| + |mean|) / std: one subtraction, one division, mean and std each rounded once to float32."""
    c = np.clip(np.asarray(x, np.float64), clip[0], clip[1])
    return 4.0 * 2.0 ** -24 * (np.abs(c).max() + abs(mean)) / std


def trilinear_bound(x):
    """12 * 2^-24 * max|x|: three nested lerps of at most 4 roundings each on values bounded by max|x|."""
    return 12.0 * 2.0 ** -24 * float(np.abs(np.asarray(x, np.float64)).max())


# ---- deterministic inputs shared by the fixture generator and the tests
def rng(seed):
    return np.random.Generator(np.random.PCG64(seed))


def ct_volume(shape, mean, sigma, seed, dtype):
    """HU-like volume with values beyond both clip limits: N(mean, sigma^2), the first voxels forced to -2000 and 3000.  int16: rounded HU;
    float32: the same draw with its fraction kept."""
    g = rng(seed)
    x = g.standard_normal(shape) * sigma + mean
    f = x.reshape(-1)
    f[0], f[-1] = -2000.0, 3000.0
    if f.size > 4:
        f[1], f[2] = 2999.25, -1999.5
    x = np.clip(x, -32000, 32000)
    return np.rint(x).astype(np.int16) if dtype == np.int16 else x.astype(np.float32)


def stack(shape, planes, seed, dtype, levels=16):
    """Class stack (planes, D, H, W).  uint8: labels 0 / 1 with a few 2 and 3; float32: probability levels (k + 0.3371) / levels (few distinct values:
    small in the compressed fixture; no average with simple rational weights -- the 1/2, 3/5, 9/12 of small size ratios -- lands on the 0.5 threshold)."""
    g = rng(seed)
    if dtype == np.uint8:
        u = g.random((planes,) + tuple(shape))
        return ((u < 0.45).astype(np.uint8) + (u < 0.05) + (u < 0.02)).astype(np.uint8)
    return ((g.integers(0, levels, (planes,) + tuple(shape)) + 0.3371) / levels).astype(np.float32)


THRESHOLD = {'u8': 0.4637, 'f32': 0.5}    # u8 labels under simple rational weights (1/2, 3/5, 9/12) give simple fractions: 0.5 or 0.45 would sit ON the threshold


def sample_index(n, limit=2048, count=768):
    """Flat indices of the voxels a fixture records of an n-voxel output: all of them up to `limit`, otherwise `count` spread over the whole range."""
    if n <= limit:
        return np.arange(n)
    return (np.arange(count) * (n - 1)) // (count - 1)
