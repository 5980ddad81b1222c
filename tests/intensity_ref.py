"""Float64 numpy restatement of the device intensity augmentation (csrc/augment_intensity.hip, training/augmentation.py) for one sample -- a helper of
tests/test_intensity_cpu.py and tests/test_gpu_intensity.py, not a test.

`apply` runs the chain multiply -> additive -> gamma -> contrast -> blur -> noise on a (D, H, W) volume with every operation in float64 (parameters are
the float32 values of the plan, exact in float64): unbiased std, zero-padded separable blur W -> H -> D with the plan's taps, and either an explicit
noise field or the Philox4x32-10 + Box-Muller field of `noise_field` (integers exact, transcendentals in float64; `dtype=np.float32` evaluates
Box-Muller in float32 instead -- the arithmetic a float32 implementation has)."""
import numpy as np

M0, M1, W0, W1 = 0xD2511F53, 0xCD9E8D57, 0x9E3779B9, 0xBB67AE85
MASK = np.uint64(0xFFFFFFFF)


def philox4x32_10(ctr, key):
    """ctr: four uint32 arrays (or ints), key: two -> four uint32 arrays.  Random123's philox4x32 with 10 rounds."""
    c = [np.atleast_1d(np.asarray(v, dtype=np.uint64)) & MASK for v in ctr]
    c = list(np.broadcast_arrays(*c))
    k = [np.uint64(int(v) & 0xFFFFFFFF) for v in key]
    for _ in range(10):
        p0, p1 = np.uint64(M0) * c[0], np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ k[0], p1 & MASK, (p0 >> np.uint64(32)) ^ c[3] ^ k[1], p0 & MASK]
        k = [(k[0] + np.uint64(W0)) & MASK, (k[1] + np.uint64(W1)) & MASK]
    return [v.astype(np.uint32) for v in c]


def noise_field(seed, n, dtype=np.float64):
    """The N(0, 1) value of voxels 0 .. n-1 of a sample with the 64-bit `seed`: key (seed low, seed high), counter (i >> 2 low, i >> 2 high, 0, 0);
    u = ((r >> 8) + 0.5) * 2^-24; normals 0, 1 = sqrt(-2 ln u(r0)) * (cos, sin)(2 pi u(r1)), normals 2, 3 from (r2, r3); voxel i takes normal i & 3."""
    seed = int(seed) & 0xFFFFFFFFFFFFFFFF
    q = np.arange((n + 3) // 4, dtype=np.uint64)
    r = philox4x32_10([q & MASK, q >> np.uint64(32), 0, 0], [seed & 0xFFFFFFFF, seed >> 32])
    u = [((v >> np.uint32(8)).astype(np.float64) + 0.5) * 2.0 ** -24 for v in r]
    out = np.empty((len(q), 4), dtype)
    for p in range(2):
        u1, u2 = u[2 * p].astype(dtype), u[2 * p + 1].astype(dtype)
        R = np.sqrt(dtype(-2.0) * np.log(u1))
        ang = dtype(2.0 * np.pi) * u2
        out[:, 2 * p], out[:, 2 * p + 1] = R * np.cos(ang), R * np.sin(ang)
    return out.reshape(-1)[:n]


def blur(v, taps):
    """Zero-padded correlation with the 1-D taps along W, then H, then D (float64)."""
    taps = np.asarray(taps, dtype=np.float64)
    r = len(taps) // 2
    for axis in (2, 1, 0):
        pad = [(0, 0)] * 3
        pad[axis] = (r, r)
        p = np.pad(v, pad)
        n = v.shape[axis]
        acc = np.zeros_like(v)
        for j in range(len(taps)):
            sl = [slice(None)] * 3
            sl[axis] = slice(j, j + n)
            acc += taps[j] * p[tuple(sl)]
        v = acc
    return v


def apply(x, multiply=None, additive=None, gamma=None, contrast=None, taps=None, noise_std=None, noise=None, seed=0, noise_dtype=np.float64):
    """x: (D, H, W) float32.  A parameter that is None did not fire.  noise: explicit (D, H, W) field, else noise_field(seed)."""
    with np.errstate(all='ignore'):
        v = np.asarray(x, dtype=np.float64)
        if multiply is not None:
            v = v * np.float64(multiply)
        if additive is not None:
            v = v + np.float64(additive)
        if gamma is not None:
            lo, hi, mean, std = v.min(), v.max(), v.mean(), v.std(ddof=1)
            y = np.power((v - lo) / (hi - lo), np.float64(gamma)) * (hi - lo) + lo
            v = (y - y.mean()) / y.std(ddof=1) * std + mean
        if contrast is not None:
            lo, hi, mean = v.min(), v.max(), v.mean()
            v = np.clip((v - mean) * np.float64(contrast) + mean, lo, hi)
        if taps is not None:
            v = blur(v, taps)
        if noise_std is not None:
            n = np.asarray(noise, dtype=np.float64) if noise is not None else noise_field(seed, v.size, noise_dtype).astype(np.float64).reshape(v.shape)
            v = v + n * np.float64(noise_std)
        return v


def apply_plan(x, plan, b, noise=None):
    """`apply` with sample b of an IntensityPlan (training/augmentation.py)."""
    on = lambda k: plan.flags[b] >> k & 1
    return apply(x, plan.multiply[b] if on(0) else None, plan.additive[b] if on(1) else None, plan.gamma[b] if on(2) else None,
                 plan.contrast[b] if on(3) else None, plan.taps[b] if on(4) else None, plan.noise_std[b] if on(5) else None, noise, plan.seed[b])
