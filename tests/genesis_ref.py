"""Numpy restatement of the device's Models Genesis pair (csrc/genesis.hip, baselines/model_genesis/utils.py) for one sample -- a helper of
tests/test_genesis_cpu.py, tests/test_gpu_genesis.py and tools/bench_genesis.py, not a test.

`apply` runs the six stages on a (D, H, W) float32 volume given a plan: min-max normalisation in float32, the flips, the block shuffle (every block
reads the flipped image, later blocks overwrite earlier ones), np.interp in float64 rounded to float32 once, the painting with an explicit noise field
or the Philox one of `paint_noise`, and the map back in float32.  Without explicit permutations `device_perms` restates the device's draw: the stable
argsort of one Philox key per box voxel.  Philox comes from tests/intensity_ref.py."""
import numpy as np

from intensity_ref import MASK, philox4x32_10

STREAM_PAINT, STREAM_PERM = 1, 2


def _key(seed):
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    return [seed & 0xFFFFFFFF, seed >> 32]


def paint_noise(seed, n):
    """The painted value of voxels 0 .. n-1 (float32): counter (i >> 2 low, i >> 2 high, 1, 0), voxel i takes word i & 3, u = ((r >> 8) + 0.5) * 2^-24
    rounded once to float32."""
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox4x32_10([q & MASK, q >> np.uint64(32), STREAM_PAINT, 0], _key(seed))
    u = np.stack([((v >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for v in r], axis=1)
    return u.reshape(-1)[:n].astype(np.float32)


def device_perms(seed, sizes):
    """perm_k for blocks of sizes[k] voxels: the stable argsort of key(i) = philox(counter (i, k, 2, 0), seed)[0], i = 0 .. sizes[k] - 1 -> a list."""
    sizes = np.asarray(sizes, dtype=np.int64)
    start = np.concatenate([[0], np.cumsum(sizes)])
    k = np.repeat(np.arange(len(sizes), dtype=np.int64), sizes)
    i = np.arange(start[-1], dtype=np.int64) - start[k]
    key = philox4x32_10([i, k, STREAM_PERM, 0], _key(seed))[0]
    order = np.lexsort((i, key, k))                      # by block, then key, ties by position
    flat = i[order]
    return [flat[start[j]:start[j + 1]] for j in range(len(sizes))]


def apply(img, flip=(False, False, False), blocks=None, perms=None, curve=None, paint=None, boxes=(), noise=None, seed=0):
    """img: (D, H, W) float32 -> (x, y) float32.  blocks: (nb, 6) ints (z0, y0, x0, nz, ny, nx) or None; perms: one array of source positions per block
    or None (device_perms(seed)); curve: (xp, fp) float64 or None; paint: None / 'in' / 'out' with boxes; noise: explicit (D, H, W) field, else
    paint_noise(seed)."""
    img = np.asarray(img, dtype=np.float32)
    minv, maxv = img.min(), img.max()
    span = np.maximum(maxv - minv, np.float32(1e-7))
    v = (img - minv) / span
    assert v.dtype == np.float32
    for axis in range(3):
        if flip[axis]:
            v = np.flip(v, axis=axis)
    v = np.ascontiguousarray(v)
    x, y = v.copy(), v.copy()
    if blocks is not None:
        blocks = np.asarray(blocks, dtype=np.int64).reshape(-1, 6)
        if perms is None:
            perms = device_perms(seed, blocks[:, 3] * blocks[:, 4] * blocks[:, 5])
        for (z0, y0, x0, nz, ny, nx), p in zip(blocks, perms):
            box = v[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx].reshape(-1)
            x[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = box[np.asarray(p)].reshape(nz, ny, nx)
    if curve is not None:
        x = np.interp(x, curve[0], curve[1]).astype(np.float32)
    if paint is not None:
        n = np.asarray(noise, dtype=np.float32) if noise is not None else paint_noise(seed, x.size).reshape(x.shape)
        inside = np.zeros(x.shape, bool)
        for z0, y0, x0, nz, ny, nx in boxes:
            inside[z0:z0 + nz, y0:y0 + ny, x0:x0 + nx] = True
        x = np.where(inside if paint == 'in' else ~inside, n, x)
    x, y = x * span + minv, y * span + minv
    assert x.dtype == np.float32 and y.dtype == np.float32
    return x, y


def apply_plan(img, plan, b, noise=None):
    """`apply` with sample b of a GenesisPlan (baselines/model_genesis/utils.py)."""
    return apply(img, plan.flip[b], plan.blocks[b], plan.perms[b], plan.curve[b], plan.paint[b], plan.boxes[b], noise, plan.seed[b])
