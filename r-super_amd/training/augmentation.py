"""Online intensity augmentations of the pre-cropped training volumes -- the six transforms `load_augmented_data`
(rsuper_train/training/dataset/dim3/dataset_abdomenatlas_UFO.py:1047-1060) applies, each behind `np.random.random() < 0.3`.

Every function takes the (1, C, D, H, W) float32 volume the loader holds at that point and consumes the torch / numpy global
generators in the same order and with the same shapes as rsuper_train/training/augmentation.py, so a run seeded like the
reference draws the same parameters: with the same seeds the outputs agree to float32 rounding (tests/golden/loader.npz).

Differences in *how* (not what): the blur is applied as three 1-D passes (k taps each instead of k^3; zero padding makes the
separable form exact up to rounding -- see gaussian_blur), and gamma / contrast avoid the reference's (C, N) broadcast
temporaries for the single-channel volumes this path feeds them.

The second half of the file is the spatial augmentation -- random_scale_rotate_translate_3d and crop_3d with the reference's signatures, and
their fusion for batches of bit-packed volumes (affine_center_crop, spatial_augment_batch) -- on the HIP kernel of csrc/augment.hip.
"""
import math

import numpy as np
import torch
import torch.nn.functional as F


def _expect_volume(img):
    if img.dim() != 5 or img.shape[0] != 1:
        raise ValueError('expected a (1, C, D, H, W) volume, got %s' % (tuple(img.shape),))


def brightness_multiply(img, multiply_range=(0.7, 1.3)):
    """img * U(lo, hi), one factor per volume (augmentation.py:85-102, per_channel=False)."""
    _expect_volume(img)
    lo, hi = multiply_range
    assert hi > lo, 'Invalid range'
    factor = torch.rand(size=(1, 1, 1, 1, 1)) * (hi - lo) + lo
    return img * factor


def brightness_additive(img, std, mean=0.0):
    """img + N(mean, std), one offset per volume (augmentation.py:68-82, per_channel=False)."""
    _expect_volume(img)
    return img + torch.normal(mean, std, size=(1, 1, 1, 1, 1))


def gamma(img, gamma_range=(0.5, 2.0)):
    """Gamma curve on the volume normalised to [0, 1], then restored to its original mean / (unbiased) std
    (augmentation.py:105-137, per_channel=False, retain_stats=True).  The reference draws torch.rand(C, 1) exponents and
    lets them broadcast against the flattened (1, N) volume; for C == 1 -- the only case the loader produces -- that is a
    single exponent, which is what is implemented; C > 1 is rejected rather than silently reshaped."""
    _expect_volume(img)
    C = img.shape[1]
    if C != 1:
        raise ValueError('gamma: only single-channel volumes are on this path')
    flat = img.reshape(1, -1)
    lo, hi = flat.min(), flat.max()
    span = hi - lo
    mean, std = flat.mean(), flat.std()
    g = torch.rand(C, 1) * (gamma_range[1] - gamma_range[0]) + gamma_range[0]
    out = torch.pow((flat - lo) / span, g) * span + lo
    out = out - out.mean()
    out = out / out.std() * std + mean
    return out.reshape(img.shape)


def contrast(img, contrast_range=(0.65, 1.5)):
    """(img - mean) * U(lo, hi) + mean, clamped to the original [min, max] (augmentation.py:139-168, preserve_range=True)."""
    _expect_volume(img)
    C = img.shape[1]
    if C != 1:
        raise ValueError('contrast: only single-channel volumes are on this path')
    flat = img.reshape(1, -1)
    lo, hi = flat.min(), flat.max()
    mean = flat.mean()
    factor = torch.rand(C, 1) * (contrast_range[1] - contrast_range[0]) + contrast_range[0]
    out = torch.clamp((flat - mean) * factor + mean, min=lo, max=hi)
    return out.reshape(img.shape)


def gaussian_kernel_1d(kernel_size, sigma):
    """Normalised 1-D Gaussian taps on the integer grid -(k//2) .. k//2.  The reference builds the k^3 kernel
    exp(-(x^2+y^2+z^2)/(2 sigma^2)) / sum (augmentation.py:35-47); that is the outer product of three of these."""
    x = torch.arange(-(kernel_size // 2), kernel_size // 2 + 1, dtype=torch.float32)
    k = torch.exp(-(x * x) / (2.0 * sigma * sigma))
    return k / k.sum()


def gaussian_blur(img, sigma_range=(0.5, 1.0)):
    """Zero-padded Gaussian blur, sigma ~ U(lo, hi), kernel size 2*ceil(3 sigma)+1 (augmentation.py:49-65).
    Applied separably: because the padding is zeros, convolving along W, H and D in turn equals the reference's single
    k^3 conv3d exactly in real arithmetic (float32 differences ~1e-7 relative)."""
    _expect_volume(img)
    if img.shape[1] != 1:
        raise ValueError('gaussian_blur: only single-channel volumes are on this path')
    sigma = torch.rand(1) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
    ks = 2 * math.ceil(3 * sigma) + 1
    k = gaussian_kernel_1d(ks, sigma)
    p = ks // 2
    out = F.conv3d(img, k.view(1, 1, 1, 1, ks), padding=(0, 0, p))
    out = F.conv3d(out, k.view(1, 1, 1, ks, 1), padding=(0, p, 0))
    out = F.conv3d(out, k.view(1, 1, ks, 1, 1), padding=(p, 0, 0))
    return out


def gaussian_noise(img, std, mean=0.0):
    """img + N(0, 1) * std + mean, one draw per voxel (augmentation.py:16-18)."""
    return img + torch.randn(img.shape) * std + mean


# ---------------------------------------------------------------------------------------------------------------------------
# Spatial augmentation on the device (csrc/augment.hip): random_scale_rotate_translate_3d (augmentation.py:228-319) and crop_3d
# (:446-469), and their fusion for the loader's `random_crop` branch (dataset_abdomenatlas_UFO.py:567-578).  The affine resampling
# is one HIP launch that reads the f32 image and up to three byte volumes (bit-packed class planes or plain u8 planes) with the
# same coordinates and writes only the output crop.  No CPU kernel: a CPU tensor raises RSuperHipError.
# ---------------------------------------------------------------------------------------------------------------------------
def _triple(v):
    return [v] * 3 if isinstance(v, (float, int)) else list(v)


def draw_affine_3d(scale=0.3, rotate=45, translate=0.1, shear=0.05):
    """The (3, 4) float32 theta of random_scale_rotate_translate_3d (:236-288).  Consumes np.random in the reference's order --
    three scales U(1 - s, 1 / (1 - s)), six shears, three translations, three integer angles randint(-r, max(r, 1)) -- and
    composes Rx . Ry . Rz . S as float32 torch.mm products in the same order: with the same seed theta is bit-identical.
    Arguments as the reference takes them: scalars or per-axis lists."""
    scale, translate, rotate, shear = _triple(scale), _triple(translate), _triple(rotate), _triple(shear)
    u = np.random.uniform
    scale_x, scale_y, scale_z = (u(low=1 - s, high=1 / (1 - s)) for s in scale)
    shear_xy, shear_xz = u(-shear[0], shear[0]), u(-shear[0], shear[0])
    shear_yx, shear_yz = u(-shear[1], shear[1]), u(-shear[1], shear[1])
    shear_zx, shear_zy = u(-shear[2], shear[2]), u(-shear[2], shear[2])
    translate_x, translate_y, translate_z = (u(-t, t) for t in translate)
    theta_scale = torch.tensor([[scale_x, shear_xy, shear_xz, translate_x],
                                [shear_yx, scale_y, shear_yz, translate_y],
                                [shear_zx, shear_zy, scale_z, translate_z],
                                [0, 0, 0, 1]]).float()
    ax, ay, az = ((float(np.random.randint(-r, max(r, 1))) / 180.) * math.pi for r in rotate)
    rx = torch.tensor([[1, 0, 0, 0], [0, math.cos(ax), -math.sin(ax), 0], [0, math.sin(ax), math.cos(ax), 0], [0, 0, 0, 1]]).float()
    ry = torch.tensor([[math.cos(ay), 0, -math.sin(ay), 0], [0, 1, 0, 0], [math.sin(ay), 0, math.cos(ay), 0], [0, 0, 0, 1]]).float()
    rz = torch.tensor([[math.cos(az), -math.sin(az), 0, 0], [math.sin(az), math.cos(az), 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]]).float()
    theta = torch.mm(torch.mm(rx, ry), rz)
    return torch.mm(theta, theta_scale)[0:3, :]


IDENTITY_THETA = ((1., 0., 0., 0.), (0., 1., 0., 0.), (0., 0., 1., 0.))


def _affine_crop(img, volumes, theta, out_size, offsets):
    """The C ABI call.  img (B, Ci, D, H, W) f32, volumes: list of (B, P, D, H, W) u8, theta (B, 3, 4) f32 (any device: it is
    12 floats per sample), offsets: B * 3 ints (z, y, x per sample) -> (image crop, list of volume crops)."""
    import ctypes
    from ..hip import lib as _l
    if not img.is_cuda or any(not v.is_cuda for v in volumes):
        raise _l.RSuperHipError('affine_crop needs device tensors (no CPU fallback)')
    if img.dim() != 5 or img.dtype != torch.float32:
        raise ValueError('affine_crop: image must be float32 (B, Ci, D, H, W), got %s %s' % (img.dtype, tuple(img.shape)))
    B, Ci, D, H, W = img.shape
    d, h, w = (int(s) for s in out_size)
    for v in volumes:
        if v.dtype != torch.uint8 or v.dim() != 5 or v.shape[0] != B or tuple(v.shape[2:]) != (D, H, W):
            raise ValueError('affine_crop: byte volumes must be uint8 (B, P, D, H, W) on the image grid')
    if tuple(theta.shape) != (B, 3, 4):
        raise ValueError('affine_crop: theta must be (B, 3, 4)')
    offsets = [int(o) for o in offsets]
    if len(offsets) != 3 * B:
        raise ValueError('affine_crop: one (z, y, x) offset per sample')
    img = img.contiguous()
    volumes = [v.contiguous() for v in volumes]
    theta = theta.to(device=img.device, dtype=torch.float32).contiguous()
    out = torch.empty((B, Ci, d, h, w), device=img.device, dtype=torch.float32)
    outs = [torch.empty((B, v.shape[1], d, h, w), device=img.device, dtype=torch.uint8) for v in volumes]
    n = len(volumes)
    src = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in volumes])
    dst = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in outs])
    planes = (ctypes.c_int * max(n, 1))(*[v.shape[1] for v in volumes])
    offs = (ctypes.c_int * (3 * B))(*offsets)
    with torch.cuda.device(img.device):
        _l.check(_l.lib().rsuper_affine_crop(theta.data_ptr(), img.data_ptr(), out.data_ptr(), B, Ci, D, H, W, n, src, dst, planes, d, h, w, offs,
                                             torch.cuda.current_stream().cuda_stream), 'affine_crop')
    return out, outs


def _affine_crop_op(img, volumes, theta, out_size, offsets):
    """torch.ops.rsuper.affine_crop, registered on first use (hip/library.py); no derivative."""
    from ..hip import lib as _l
    from ..hip import ops as _ops          # noqa: F401  (hip/ops.py pulls in hip/library.py; this order avoids the import cycle)
    from ..hip import library as _library
    if not img.is_cuda:                                    # the dispatcher's "no CPU kernel" error, as the project's own exception
        raise _l.RSuperHipError('affine_crop needs device tensors (no CPU fallback)')
    return _library.install_augment_ops(_affine_crop)(img, list(volumes), theta, list(out_size), list(offsets))


def crop_3d(img, lab, crop_size, mode):
    """crop_3d (:446-469): 'random' draws np.random.randint(0, max(diff, 1)) for z, y, x in this order, 'center' takes diff // 2."""
    assert mode in ['random', 'center'], "Invalid Mode, should be 'random' or 'center'"
    if isinstance(crop_size, int):
        crop_size = [crop_size] * 3
    z, y, x = crop_offsets(img.shape[2:], crop_size, mode)
    cd, ch, cw = crop_size
    return img[:, :, z:z + cd, y:y + ch, x:x + cw].contiguous(), lab[:, :, z:z + cd, y:y + ch, x:x + cw].contiguous()


def crop_offsets(size, crop_size, mode):
    """The (z, y, x) corner crop_3d cuts at (:453-464)."""
    diff = [int(s) - int(c) for s, c in zip(size, crop_size)]
    if mode == 'random':
        return [int(np.random.randint(0, max(df, 1))) for df in diff]
    return [df // 2 for df in diff]


def _as_bytes(t, what):
    """int64 / u8 / bool volume -> the u8 planes the kernel gathers (the reference resamples .float() planes with 'nearest': values pass through)."""
    if t.dtype in (torch.uint8, torch.bool):
        return t.to(torch.uint8)
    if t.dtype == torch.int64:
        if t.numel() and (int(t.min()) < 0 or int(t.max()) > 255):
            raise ValueError('%s: label values must fit a byte' % what)
        return t.to(torch.uint8)
    raise ValueError('%s: expected an int64, uint8 or bool volume, got %s' % (what, t.dtype))


def random_scale_rotate_translate_3d(img, lab, scale=0.3, rotate=45, translate=0.1, shear=0.05, foreground=None):
    """random_scale_rotate_translate_3d (:228-319) on device tensors: img (1, C, D, H, W) f32 trilinear, lab (1, C, D, H, W) int64 / u8 / bool
    nearest -> int64 as the reference's `.long()`, foreground (D, H, W) / (1, D, H, W) / (1, 1, D, H, W) nearest -> bool in its own rank.
    The kernel runs with the crop set to the full volume."""
    assert len(img.size()) == 5
    theta = draw_affine_3d(scale, rotate, translate, shear)
    B = img.shape[0]
    vols = [_as_bytes(lab, 'lab')]
    if foreground is not None:
        if foreground.ndim not in (3, 4, 5):
            raise ValueError('Invalid dimension of foreground mask')
        fg = _as_bytes(foreground, 'foreground')
        vols.append(fg.reshape((1,) * (5 - fg.ndim) + tuple(fg.shape)))
    out, outs = _affine_crop_op(img.float(), vols, theta.unsqueeze(0).expand(B, 3, 4), img.shape[2:], [0, 0, 0] * B)
    if foreground is None:
        return out, outs[0].long()
    return out, outs[0].long(), outs[1].reshape(foreground.shape).bool()


def _packed_of(v):
    return v.packed if hasattr(v, 'packed') else v


def _like(v, t):
    return type(v)(t, v.C) if hasattr(v, 'packed') else t


def affine_center_crop(img, volumes, theta, out_size):
    """The fused production path: img (B, Ci, D, H, W) f32, volumes: tuple of packed u8 (B, P, D, H, W) tensors or PackedBits, theta (B, 3, 4) ->
    (image crop, tuple of crops of the same kinds).  Equals transforming the whole volume and then crop_3d(..., 'center') -- offsets
    ((D - d) // 2, (H - h) // 2, (W - w) // 2) -- but only the crop is computed."""
    off = crop_offsets(img.shape[2:], out_size, 'center')
    out, outs = _affine_crop_op(img, [_packed_of(v) for v in volumes], theta, out_size, off * img.shape[0])
    return out, tuple(_like(v, t) for v, t in zip(volumes, outs))


def plan_spatial_augment(batch, size, training_size, scale, rotate, translate, p=0.4):
    """The random draws of `random_crop` (dataset_abdomenatlas_UFO.py:573-577) for `batch` samples of extent `size`, in the reference's order per
    sample: np.random.random() < p -> the affine draws, centre crop; otherwise the three randint offsets of a random plain crop (identity theta).
    Returns theta (batch, 3, 4) f32, the flat offset list and the branch taken per sample (True = affine)."""
    thetas, offs, branch = [], [], []
    for _ in range(batch):
        if np.random.random() < p:
            thetas.append(draw_affine_3d(scale, rotate, translate))
            offs += crop_offsets(size, training_size, 'center')
            branch.append(True)
        else:
            thetas.append(torch.tensor(IDENTITY_THETA))
            offs += crop_offsets(size, training_size, 'random')
            branch.append(False)
    return torch.stack(thetas), offs, branch


def spatial_augment_batch(img, volumes, training_size, scale, rotate, translate, p=0.4):
    """`random_crop`'s branch for a batch of large crops (d + 20, h + 40, w + 40) already on the device: per sample, with probability p the random
    affine + centre crop, otherwise a random plain crop to training_size -- the same kernel with an identity theta (an exact copy) and that
    sample's offset, so the whole batch is one launch.  volumes as in affine_center_crop."""
    if isinstance(training_size, int):
        training_size = [training_size] * 3
    theta, offs, _ = plan_spatial_augment(img.shape[0], img.shape[2:], training_size, scale, rotate, translate, p)
    out, outs = _affine_crop_op(img, [_packed_of(v) for v in volumes], theta, training_size, offs)
    return out, tuple(_like(v, t) for v, t in zip(volumes, outs))


# ---------------------------------------------------------------------------------------------------------------------------
# Intensity augmentation on the device (csrc/augment_intensity.hip): the six functions at the top of this file, gated per sample as
# dataset/augmented.py online_intensity_augmentation gates them, for a batch of (B, 1, D, H, W) volumes already on the training stream.
# A plan holds what fired and with which parameter per sample; one C ABI call applies it (at most 3 launches per 8 samples).
# No CPU kernel: a CPU tensor raises RSuperHipError.
# ---------------------------------------------------------------------------------------------------------------------------
INTENSITY_TRANSFORMS = ('multiply', 'additive', 'gamma', 'contrast', 'blur', 'noise')      # bit k of a sample's flags = transform k fired


class IntensityPlan:
    """Per sample: flags (bit k = INTENSITY_TRANSFORMS[k] fired), the four scalars and the noise std as exact float32 values (0 where not fired),
    sigma / radius / taps of the blur (taps: the 2 * radius + 1 float32 values of gaussian_kernel_1d) and the 64-bit noise seed."""

    def __init__(self, batch):
        self.batch = batch
        self.flags = [0] * batch
        self.multiply, self.additive, self.gamma, self.contrast, self.noise_std = ([0.0] * batch for _ in range(5))
        self.sigma, self.radius, self.taps = [None] * batch, [0] * batch, [[] for _ in range(batch)]
        self.seed = [0] * batch

    def fired(self, b):
        return [n for k, n in enumerate(INTENSITY_TRANSFORMS) if self.flags[b] >> k & 1]


def _f32(v):
    """The float32 value of a Python number / one-element tensor, as an (exact) Python float."""
    return float(torch.as_tensor(v, dtype=torch.float32).reshape(-1)[0])


def _per_sample(v, batch, what):
    if v is None:
        return [None] * batch
    v = list(v)
    if len(v) != batch:
        raise ValueError('%s: one value (or None) per sample, got %d for a batch of %d' % (what, len(v), batch))
    return v


def make_intensity_plan(batch, multiply=None, additive=None, gamma=None, contrast=None, sigma=None, noise_std=None, seed=None):
    """A plan from explicit per-sample values: every argument is None or a sequence of `batch` entries, an entry None = that transform did not fire
    for that sample.  sigma becomes the radius ceil(3 sigma) and the taps of gaussian_kernel_1d exactly as gaussian_blur computes them (float32
    sigma, kernel size 2 * ceil(3 sigma) + 1).  seed: the 64-bit key of the in-kernel noise field per sample (default 0; unused with an explicit
    noise tensor)."""
    plan = IntensityPlan(batch)
    cols = [_per_sample(v, batch, n) for v, n in ((multiply, 'multiply'), (additive, 'additive'), (gamma, 'gamma'), (contrast, 'contrast'),
                                                  (sigma, 'sigma'), (noise_std, 'noise_std'))]
    seeds = _per_sample(seed, batch, 'seed')
    for b in range(batch):
        for k, dst in ((0, plan.multiply), (1, plan.additive), (2, plan.gamma), (3, plan.contrast), (5, plan.noise_std)):
            if cols[k][b] is not None:
                plan.flags[b] |= 1 << k
                dst[b] = _f32(cols[k][b])
        if cols[4][b] is not None:
            s = torch.as_tensor(cols[4][b], dtype=torch.float32).reshape(1)
            ks = 2 * math.ceil(3 * s) + 1
            plan.flags[b] |= 1 << 4
            plan.sigma[b], plan.radius[b], plan.taps[b] = float(s), ks // 2, [float(t) for t in gaussian_kernel_1d(ks, s)]
        if seeds[b] is not None:
            plan.seed[b] = int(seeds[b]) & 0xFFFFFFFFFFFFFFFF
    return plan


def plan_intensity_augment(batch, p=0.3, multiply_range=(0.7, 1.3), additive_std=0.1, gamma_range=(0.7, 1.5), contrast_range=(0.7, 1.3),
                           sigma_range=(0.5, 1.5), noise_std_max=0.2):
    """The random draws of online_intensity_augmentation plus the six functions for `batch` samples, from numpy's and torch's global generators in
    the reference's order and shapes per sample: the gate np.random.random() < p, then the transform's own torch.rand / torch.normal
    ((1, 1, 1, 1, 1) for multiply and additive, (1, 1) for gamma and contrast, (1,) for sigma); for the noise the gate, then np.random.random() *
    noise_std_max.  With the same seeds the gates and the five parameters are the reference's, bit for bit.  The one difference is the noise
    field: the reference draws torch.randn(img.shape) there; the plan draws one 64-bit seed (two torch.randint words) for the in-kernel Philox
    field instead, so from the first sample whose noise fires torch's generator stands elsewhere than the reference's (numpy's does not)."""
    cols = {k: [None] * batch for k in ('multiply', 'additive', 'gamma', 'contrast', 'sigma', 'noise_std', 'seed')}
    for b in range(batch):
        if np.random.random() < p:
            lo, hi = multiply_range
            cols['multiply'][b] = torch.rand(size=(1, 1, 1, 1, 1)) * (hi - lo) + lo
        if np.random.random() < p:
            cols['additive'][b] = torch.normal(0.0, additive_std, size=(1, 1, 1, 1, 1))
        if np.random.random() < p:
            cols['gamma'][b] = torch.rand(1, 1) * (gamma_range[1] - gamma_range[0]) + gamma_range[0]
        if np.random.random() < p:
            cols['contrast'][b] = torch.rand(1, 1) * (contrast_range[1] - contrast_range[0]) + contrast_range[0]
        if np.random.random() < p:
            cols['sigma'][b] = torch.rand(1) * (sigma_range[1] - sigma_range[0]) + sigma_range[0]
        if np.random.random() < p:
            cols['noise_std'][b] = np.random.random() * noise_std_max
            w = torch.randint(0, 1 << 32, (2,), dtype=torch.int64)
            cols['seed'][b] = int(w[0]) | (int(w[1]) << 32)
    return make_intensity_plan(batch, **cols)


def _intensity_augment(img, flags, scalars, radius, taps, seeds, noise=None, workspace=None):
    """The C ABI call.  img (B, 1, D, H, W) f32 on the device; flags / radius / seeds: B ints, scalars: B * 5 floats (multiply, additive, gamma,
    contrast, noise std), taps: B * (2 * BLUR_MAX_RADIUS + 1) floats; noise: optional N(0, 1) tensor of img's shape that replaces the generator;
    workspace: optional uint8 device tensor of rsuper_intensity_augment_workspace_bytes bytes (allocated here when gamma / contrast fire) -> new tensor."""
    import ctypes
    from ..hip import lib as _l
    if not img.is_cuda or (noise is not None and not noise.is_cuda):
        raise _l.RSuperHipError('intensity_augment needs device tensors (no CPU fallback)')
    if img.dim() != 5 or img.shape[1] != 1 or img.dtype != torch.float32:
        raise ValueError('intensity_augment: image must be float32 (B, 1, D, H, W), got %s %s' % (img.dtype, tuple(img.shape)))
    B, _, D, H, W = img.shape
    nt = 2 * _l.BLUR_MAX_RADIUS + 1
    if len(flags) != B or len(radius) != B or len(seeds) != B or len(scalars) != 5 * B or len(taps) != nt * B:
        raise ValueError('intensity_augment: per-sample records do not match the batch of %d' % B)
    if noise is not None and (noise.dtype != torch.float32 or tuple(noise.shape) != tuple(img.shape)):
        raise ValueError('intensity_augment: the noise tensor must be float32 of the image shape')
    img = img.contiguous()
    noise = None if noise is None else noise.contiguous()
    L = _l.lib()
    if workspace is None and any(f & 12 for f in flags):
        workspace = torch.empty((L.rsuper_intensity_augment_workspace_bytes(B, D, H, W),), device=img.device, dtype=torch.uint8)
    out = torch.empty_like(img)
    with torch.cuda.device(img.device):
        _l.check(L.rsuper_intensity_augment(
            img.data_ptr(), out.data_ptr(), B, D, H, W, (ctypes.c_int * B)(*[int(f) for f in flags]), (ctypes.c_float * (5 * B))(*scalars),
            (ctypes.c_int * B)(*[int(r) for r in radius]), (ctypes.c_float * (nt * B))(*taps),
            (ctypes.c_ulonglong * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in seeds]), None if noise is None else noise.data_ptr(),
            None if workspace is None else workspace.data_ptr(), 0 if workspace is None else workspace.numel() * workspace.element_size(),
            torch.cuda.current_stream().cuda_stream), 'intensity_augment')
    return out


def intensity_launches(plan):
    """Kernel launches intensity_augment_batch makes for this plan (0: nothing fired, the input is returned)."""
    import ctypes
    from ..hip import lib as _l
    if not any(plan.flags):
        return 0
    return _l.lib().rsuper_intensity_augment_launches(plan.batch, (ctypes.c_int * plan.batch)(*plan.flags))


def intensity_augment_batch(img, plan=None, noise=None, **ranges):
    """The six intensity transforms on a batch of volumes (B, 1, D, H, W) f32 on the device, each sample with its own draws: `plan` (default:
    plan_intensity_augment(B, **ranges), drawn here) says what fires; noise: optional explicit N(0, 1) tensor instead of the in-kernel field.
    One dispatcher call, torch.ops.rsuper.intensity_augment; returns a new tensor -- or img itself when nothing fired in any sample."""
    from ..hip import lib as _l
    from ..hip import ops as _ops          # noqa: F401  (hip/ops.py pulls in hip/library.py; this order avoids the import cycle)
    from ..hip import library as _library
    if not img.is_cuda:                                    # the dispatcher's "no CPU kernel" error, as the project's own exception
        raise _l.RSuperHipError('intensity_augment needs device tensors (no CPU fallback)')
    if img.dim() != 5 or img.shape[1] != 1 or img.dtype != torch.float32:
        raise ValueError('intensity_augment: image must be float32 (B, 1, D, H, W), got %s %s' % (img.dtype, tuple(img.shape)))
    if plan is None:
        plan = plan_intensity_augment(img.shape[0], **ranges)
    elif ranges:
        raise ValueError('intensity_augment_batch: ranges are for drawing a plan; one was given')
    if plan.batch != img.shape[0]:
        raise ValueError('intensity_augment_batch: the plan is for %d samples, the batch has %d' % (plan.batch, img.shape[0]))
    if not any(plan.flags):
        return img
    nt = 2 * _l.BLUR_MAX_RADIUS + 1
    scalars, taps = [], []
    for b in range(plan.batch):
        scalars += [plan.multiply[b], plan.additive[b], plan.gamma[b], plan.contrast[b], plan.noise_std[b]]
        taps += (list(plan.taps[b]) + [0.0] * nt)[:nt]    # a radius above the limit is refused by the call itself, never clamped
    seeds = [s - (1 << 64) if s >= (1 << 63) else s for s in plan.seed]        # the schema's ints are signed 64-bit
    return _library.install_intensity_ops(_intensity_augment)(img, list(plan.flags), scalars, list(plan.radius), taps, seeds, noise, None)


# ---------------------------------------------------------------------------------------------------------------------------
# Crop-on-tumour on the device (csrc/crop.hip): random_crop_on_tumor (augmentation.py:600), negative_crop (:662), organ_crop (:675),
# tumor_crop (:716), crop_around_coordinate_3d (:498) and pad_volume_pair (:1023) for a whole CT whose label is a PackedBits (or a plain
# u8 / int64 (1, C, D, H, W) label).  The label is never inflated: rsuper_class_counts popcounts the packed bytes into a chunk table and
# (C + 1) totals, the draws are made on the host from the totals (plan_crop_on_tumor, the one device-to-host read of a sample),
# rsuper_select_voxel finds "the k-th set voxel in row-major order" = torch.nonzero(mask)[k] on the device, and rsuper_crop_box cuts the
# image and the byte planes around it.  The chosen voxel and the crop's corner stay on the device.  Every function takes `pad=(pd, ph, pw)`
# in addition to the reference's arguments: the source then counts as pad_volume_pair(img, lab, pd, ph, pw) would have padded it, without
# the padded copy being made.  No CPU kernel: a CPU tensor raises RSuperHipError.
# ---------------------------------------------------------------------------------------------------------------------------
CROP_CHUNK = 16384         # RSUPER_CROP_CHUNK of the header: voxels per row of the chunk table
VOX_F32, VOX_I16 = 1, 2    # RSUPER_VOX_* of the header


def padded_size(size, pad):
    """(padded extents, padding on the low side) of pad_volume_pair (:1049-1066): max(size, desired), (padded - size) // 2."""
    size = [int(s) for s in size]
    if pad is None:
        return size, [0, 0, 0]
    full = [max(s, int(p)) for s, p in zip(size, pad)]
    return full, [(f - s) // 2 for f, s in zip(full, size)]


class CropPlan:
    """What the draws of one crop decided.  branch: 'tumor' / 'background' / 'organ' (the function entered); fallback: it fell back to crop_3d's random
    corner `origin`; otherwise the crop is centred on voxel number `rank` (row-major) of `column` (a class, or C = the background column) whose total
    is `count`, shifted by `offsets`; crop_organ: what the reference returns with return_crop_organ (a class index or 'random')."""

    def __init__(self, branch):
        self.branch, self.fallback, self.column, self.rank, self.count = branch, False, None, None, None
        self.offsets, self.origin, self.crop_organ = None, None, 'random'

    def __repr__(self):
        return 'CropPlan(%s)' % ', '.join('%s=%r' % kv for kv in sorted(vars(self).items()))


def _draw_center(plan, column, count, crop):
    """center = voxels[torch.randint(0, len(voxels), (1,))][0], then the three shifts of 'small_rnd_shift' (:530-537)."""
    plan.column, plan.count = int(column), int(count)
    plan.rank = int(torch.randint(0, int(count), (1,)))
    plan.offsets = [int(np.random.randint(-int(c * 0.5), int(c * 0.5) + 1)) for c in crop]
    return plan


def _fall_back(plan, size, crop):
    plan.fallback, plan.origin, plan.crop_organ = True, crop_offsets(size, crop, 'random'), 'random'
    return plan


def plan_tumor_crop(totals, lesion_classes, size, crop):
    """tumor_crop's draws (:716-738) from the (C + 1) totals: no lesion voxel -> crop_3d's three draws; otherwise torch.randint over the lesion classes
    that are present, torch.randint over the chosen class's voxels, the three shifts."""
    plan = CropPlan('tumor')
    lesion_classes = [int(c) for c in lesion_classes]
    possibilities = [i for i, c in enumerate(lesion_classes) if totals[c] > 0]
    if not possibilities:
        return _fall_back(plan, size, crop)
    chosen = possibilities[torch.randint(0, len(possibilities), (1,)).item()]
    plan.crop_organ = lesion_classes[chosen]
    return _draw_center(plan, lesion_classes[chosen], totals[lesion_classes[chosen]], crop)


def plan_organ_crop(totals, lesion_classes, size, crop, foreground_classes=None):
    """organ_crop's draws (:675-710): the non-lesion classes (of foreground_classes when given) that are present, one by torch.randint, then a voxel."""
    plan = CropPlan('organ')
    C = len(totals) - 1
    clss = [c for c in range(C) if c not in lesion_classes and (foreground_classes is None or c in foreground_classes) and totals[c] > 0]
    if not clss:
        return _fall_back(plan, size, crop)
    plan.crop_organ = clss[torch.randint(0, len(clss), (1,)).item()]
    return _draw_center(plan, plan.crop_organ, totals[plan.crop_organ], crop)


def plan_negative_crop(totals, size, crop):
    """negative_crop's draws (:662-672): a voxel of the background column (label.sum(0) == 0), or crop_3d's when there is none."""
    plan = CropPlan('background')
    C = len(totals) - 1
    if totals[C] == 0:
        return _fall_back(plan, size, crop)
    return _draw_center(plan, C, totals[C], crop)


def plan_crop_on_tumor(totals, lesion_classes, size, crop, tumor_case, tumor_prob=None, foreground_prob=None, background_prob=None,
                       foreground_classes=None):
    """The draws of random_crop_on_tumor (:618-652) in the reference's order: np.random.random() picks the branch, then that branch's draws.
    totals: the (C + 1) voxel counts of the (padded) volume -- classes 0 .. C - 1, then the background; size: its (padded) extents; crop: (d, h, w)."""
    totals = [int(t) for t in totals]
    rnd = np.random.random()
    if (tumor_prob is None) or (foreground_prob is None) or (background_prob is None):
        tumor_prob, foreground_prob, background_prob = (0.9, 0.05, 0.05) if tumor_case else (0, 0.9, 0.1)
    if rnd < tumor_prob:
        return plan_tumor_crop(totals, lesion_classes, size, crop)
    if rnd < (tumor_prob + background_prob):
        return plan_negative_crop(totals, size, crop)
    return plan_organ_crop(totals, lesion_classes, size, crop, foreground_classes)


def _crop_ops():
    from ..hip import ops as _ops          # noqa: F401  (hip/ops.py pulls in hip/library.py; this order avoids the import cycle)
    from ..hip import library as _library
    return _library.install_crop_ops(_class_counts, _select_voxel, _crop_box)


def _need_device(what, *ts):
    from ..hip import lib as _l
    if any(t is not None and not t.is_cuda for t in ts):
        raise _l.RSuperHipError('%s needs device tensors (no CPU fallback)' % what)


def _class_counts(packed, C, plain, workspace=None):
    """The C ABI call.  packed (B, P, D, H, W) u8 -> (totals (B, C + 1) int64, the chunk table as the uint8 workspace it lives in)."""
    from ..hip import lib as _l
    _need_device('class_counts', packed)
    if packed.dim() != 5 or packed.dtype != torch.uint8:
        raise ValueError('class_counts: the label must be uint8 (B, P, D, H, W), got %s %s' % (packed.dtype, tuple(packed.shape)))
    if not packed.is_contiguous():
        raise ValueError('class_counts: the label must be contiguous')
    B, P, D, H, W = packed.shape
    L = _l.lib()
    need = L.rsuper_class_counts_workspace_bytes(B, int(C), D, H, W)
    if workspace is None:
        workspace = torch.empty((need,), device=packed.device, dtype=torch.uint8)
    totals = torch.empty((B, int(C) + 1), device=packed.device, dtype=torch.int64)
    with torch.cuda.device(packed.device):
        _l.check(L.rsuper_class_counts(packed.data_ptr(), B, P, int(C), int(bool(plain)), D, H, W, workspace.data_ptr(),
                                       workspace.numel() * workspace.element_size(), totals.data_ptr(), torch.cuda.current_stream().cuda_stream),
                 'class_counts')
    return totals, workspace


def _select_voxel(packed, C, plain, table, b, column, k, count, add):
    """The C ABI call -> (3,) int32 device tensor (z, y, x) + add.  k outside [0, count) is refused before anything is launched."""
    from ..hip import lib as _l
    _need_device('select_voxel', packed, table)
    B, P, D, H, W = packed.shape
    out = torch.empty((3,), device=packed.device, dtype=torch.int32)
    with torch.cuda.device(packed.device):
        _l.check(_l.lib().rsuper_select_voxel(packed.data_ptr(), B, P, int(C), int(bool(plain)), D, H, W, table.data_ptr(),
                                              table.numel() * table.element_size(), int(b), int(column), int(k), int(count),
                                              int(add[0]), int(add[1]), int(add[2]), out.data_ptr(), torch.cuda.current_stream().cuda_stream),
                 'select_voxel')
    return out


def _crop_box(img, volumes, size, pad, center, origin):
    """The C ABI call.  img (B, Ci, D, H, W) f32 / int16 or None, volumes: list of (B, P, D, H, W) u8, size (d, h, w), pad (pd, ph, pw) (0 = none),
    center: None or (B, 3) int32 device tensor, origin: B * 3 ints (the corner, or with a center the shift) -> (f32 image crop, volume crops,
    (B, 3) int32 device tensor of the corners used)."""
    import ctypes
    from ..hip import lib as _l
    _need_device('crop_box', img, center, *volumes)
    ref = img if img is not None else volumes[0]
    if ref.dim() != 5:
        raise ValueError('crop_box: expected (B, C, D, H, W) tensors')
    B, _, D, H, W = ref.shape
    if img is not None and img.dtype not in (torch.float32, torch.int16):
        raise ValueError('crop_box: the image must be float32 or int16, got %s' % img.dtype)
    for v in volumes:
        if v.dtype != torch.uint8 or v.dim() != 5 or v.shape[0] != B or tuple(v.shape[2:]) != (D, H, W):
            raise ValueError('crop_box: byte volumes must be uint8 (B, P, D, H, W) on the image grid')
    d, h, w = (int(s) for s in size)
    pad = [int(p) for p in pad]
    origin = [int(o) for o in origin]
    if len(origin) != 3 * B or len(pad) != 3:
        raise ValueError('crop_box: one (z, y, x) triple per sample and one pad triple')
    if center is not None and (center.dtype != torch.int32 or center.numel() != 3 * B):
        raise ValueError('crop_box: the centre must be a (B, 3) int32 tensor')
    img = None if img is None else img.contiguous()
    volumes = [v.contiguous() for v in volumes]
    center = None if center is None else center.contiguous()
    Ci = 0 if img is None else img.shape[1]
    out = torch.empty((B, Ci, d, h, w), device=ref.device, dtype=torch.float32)
    outs = [torch.empty((B, v.shape[1], d, h, w), device=ref.device, dtype=torch.uint8) for v in volumes]
    used = torch.empty((B, 3), device=ref.device, dtype=torch.int32)
    n = len(volumes)
    src = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in volumes])
    dst = (ctypes.c_void_p * max(n, 1))(*[v.data_ptr() for v in outs])
    planes = (ctypes.c_int * max(n, 1))(*[v.shape[1] for v in volumes])
    with torch.cuda.device(ref.device):
        _l.check(_l.lib().rsuper_crop_box(None if img is None else img.data_ptr(), VOX_I16 if (img is not None and img.dtype == torch.int16) else VOX_F32,
                                          out.data_ptr() if Ci else None, B, Ci, D, H, W, n, src, dst, planes, d, h, w, pad[0], pad[1], pad[2],
                                          None if center is None else center.data_ptr(), (ctypes.c_int * (3 * B))(*origin), used.data_ptr(),
                                          torch.cuda.current_stream().cuda_stream), 'crop_box')
    return out, outs, used


class LabelCounts:
    """The chunk table and the (B, C + 1) totals of one label, as rsuper_class_counts left them on the device.  `host(b)` is the one device-to-host read."""

    def __init__(self, planes, C, plain, totals, table):
        self.planes, self.C, self.plain, self.totals, self.table = planes, int(C), bool(plain), totals, table
        self._host = None

    def host(self, b=0):
        if self._host is None:
            self._host = self.totals.cpu().tolist()
        return list(self._host[b])


def _label_planes(lab, what):
    """PackedBits -> (its packed bytes, C, False); a plain int64 / u8 / bool (B, C, D, H, W) label -> (u8 planes, C, True)."""
    if hasattr(lab, 'packed'):
        return lab.packed, lab.C, False
    _need_device(what, lab)
    if lab.dim() != 5:
        raise ValueError('%s: the label must be (B, C, D, H, W)' % what)
    return _as_bytes(lab, what).contiguous(), lab.shape[1], True


def _label_like(lab, t):
    if hasattr(lab, 'packed'):
        return type(lab)(t, lab.C)
    return t.to(lab.dtype)


def class_counts(lab):
    """Voxel counts of every class and of the background of a PackedBits or plain label on the device -> LabelCounts (torch.ops.rsuper.class_counts)."""
    planes, C, plain = _label_planes(lab, 'class_counts')
    totals, table = _crop_ops()[0](planes, C, plain, None)
    return LabelCounts(planes, C, plain, totals, table)


def select_voxel(counts, column, k, count=None, b=0, add=(0, 0, 0)):
    """(z, y, x) + add of the k-th voxel (row-major) of `column` (a class, or counts.C = the background) of sample b, as a (3,) int32 device tensor:
    torch.nonzero(mask)[k] without the mask (torch.ops.rsuper.select_voxel).  count: the column's total when the caller has already read it (default:
    read here).  k outside [0, count) raises RSuperHipError."""
    if count is None:
        count = counts.host(b)[column]
    return _crop_ops()[1](counts.planes, counts.C, counts.plain, counts.table, int(b), int(column), int(k), int(count), [int(v) for v in add])


def crop_box(img, volumes, size, pad=None, origin=None, center=None, offset=None):
    """Box crops of size (d, h, w) of img (B, Ci, D, H, W) f32 / int16 (or None) and of the byte volumes (packed u8 tensors or PackedBits), the source
    zero-padded to `pad` as pad_volume_pair pads, in padded coordinates (torch.ops.rsuper.crop_box).  Either origin = B * 3 ints (the corners), or
    center = (B, 3) int32 device tensor and offset = B * 3 ints: corner = clip(center - size // 2 + offset, 0, padded size - size).
    -> (f32 image crop or None, tuple of crops of the kinds given, (B, 3) int32 device tensor of the corners used)."""
    if (origin is None) == (center is None):
        raise ValueError('crop_box: give either origin or center (+ offset)')
    ref = img if img is not None else _packed_of(volumes[0])
    B = ref.shape[0]
    shift = list(origin) if center is None else list(offset if offset is not None else [0, 0, 0] * B)
    out, outs, used = _crop_ops()[2](img, [_packed_of(v) for v in volumes], [int(s) for s in size], [0, 0, 0] if pad is None else [int(p) for p in pad],
                                     None if center is None else center.reshape(B, 3), [int(s) for s in shift])
    return (out if img is not None else None), tuple(_like(v, t) for v, t in zip(volumes, outs)), used


def pad_volume_pair(input_tensor, label_tensor, desired_d, desired_h, desired_w):
    """pad_volume_pair (:1023-1075) on the device: zeros on both sides, pad // 2 on the low side; tensors that need no padding are returned as they
    are.  One crop_box launch whose crop is the whole padded volume (the image comes back as float32).  The crop functions below do not need it: they
    take pad= and never make this copy."""
    size = tuple(input_tensor.shape[-3:])
    if size != tuple(label_tensor.shape[-3:]):
        raise ValueError('The input and label tensors must have the same spatial dimensions.')
    full, _ = padded_size(size, (desired_d, desired_h, desired_w))
    if list(size) == full:
        return input_tensor, label_tensor
    planes, _, _ = _label_planes(label_tensor, 'pad_volume_pair')
    img, (lab,), _ = crop_box(input_tensor, (planes,), full, pad=full, origin=[0, 0, 0] * input_tensor.shape[0])
    return img, _label_like(label_tensor, lab)


def crop_planned(tensor_img, tensor_lab, plan_fn, crop, pad=None, counts=None, foreground=None):
    """The chain behind every crop function: class_counts -> one read of the totals -> plan_fn(totals, padded size) draws a CropPlan ->
    select_voxel -> crop_box.  With pad= the totals are those of the padded volume (its padding is background).  A background voxel of a padded
    volume is ranked in the padded volume's row-major order, which no table of the real volume gives: for that branch alone the padded label (not
    the image) is written once and counted again.  -> (image crop, label crop of tensor_lab's kind [, foreground crop], plan, corner (1, 3) int32)."""
    _need_device('crop_on_tumor', tensor_img)
    if tensor_img.dim() != 5 or tensor_img.shape[0] != 1:
        raise ValueError('expected a (1, C, D, H, W) volume, got %s' % (tuple(tensor_img.shape),))
    planes, C, plain = _label_planes(tensor_lab, 'crop_on_tumor')
    assert planes.shape[0] == 1
    size = tuple(tensor_img.shape[2:])
    if tuple(planes.shape[2:]) != size:
        raise ValueError('The input and label tensors must have the same spatial dimensions.')
    crop = [int(c) for c in crop]
    full, lo = padded_size(size, pad)
    if any(c > f for c, f in zip(crop, full)):
        raise ValueError('crop %s is larger than the (padded) volume %s' % (crop, full))
    if counts is None:
        counts = class_counts(tensor_lab)
    totals = counts.host(0)
    extra = full[0] * full[1] * full[2] - size[0] * size[1] * size[2]
    totals[C] += extra
    plan = plan_fn(totals, full)
    vols = [planes]
    if foreground is not None:
        fg = _as_bytes(foreground, 'foreground')
        vols.append(fg.reshape((1,) * (5 - fg.ndim) + tuple(fg.shape)))
    if plan.fallback:
        out, outs, used = crop_box(tensor_img, vols, crop, pad=full, origin=plan.origin)
    else:
        if plan.column == C and extra:
            padded = crop_box(None, (planes,), full, pad=full, origin=[0, 0, 0])[1][0]
            pc = _crop_ops()[0](padded, C, plain, None)
            center = _crop_ops()[1](padded, C, plain, pc[1], 0, C, plan.rank, plan.count, [0, 0, 0])
        else:
            center = select_voxel(counts, plan.column, plan.rank, plan.count, add=lo)
        out, outs, used = crop_box(tensor_img, vols, crop, pad=full, center=center, offset=plan.offsets)
    res = (out, _label_like(tensor_lab, outs[0]))
    if foreground is not None:
        res += (outs[1].to(foreground.dtype),)
    return res + (plan, used)


def _organ_name(plan, class_names):
    co = plan.crop_organ
    return class_names[co] if (co is not None and co != 'random' and class_names is not None) else co


def random_crop_on_tumor(tensor_img, tensor_lab, lesion_classes, d, h, w, tumor_case, tumor_prob=None, foreground_prob=None, background_prob=None,
                         return_crop_organ=False, class_names=None, foreground_classes=None, pad=None, counts=None):
    """random_crop_on_tumor (:600-660) on a device image (1, Ci, D, H, W) f32 / int16 and a PackedBits or plain (1, C, D, H, W) label."""
    r = crop_planned(tensor_img, tensor_lab, lambda t, s: plan_crop_on_tumor(t, lesion_classes, s, [d, h, w], tumor_case, tumor_prob, foreground_prob,
                                                                            background_prob, foreground_classes), [d, h, w], pad, counts)
    return (r[0], r[1], _organ_name(r[2], class_names)) if return_crop_organ else r[:2]


def negative_crop(tensor_img, tensor_lab, lesion_classes, d, h, w, pad=None, counts=None):
    """negative_crop (:662-673): around a random background voxel, or crop_3d's random crop when every voxel carries a label."""
    return crop_planned(tensor_img, tensor_lab, lambda t, s: plan_negative_crop(t, s, [d, h, w]), [d, h, w], pad, counts)[:2]


def organ_crop(tensor_img, tensor_lab, lesion_classes, d, h, w, return_crop_organ=False, foreground_classes=None, pad=None, counts=None):
    """organ_crop (:675-714): around a random voxel of a random non-lesion class that is present."""
    r = crop_planned(tensor_img, tensor_lab, lambda t, s: plan_organ_crop(t, lesion_classes, s, [d, h, w], foreground_classes), [d, h, w], pad, counts)
    return (r[0], r[1], r[2].crop_organ) if return_crop_organ else r[:2]


def tumor_crop(tensor_img, tensor_lab, lesion_classes, d, h, w, return_crop_organ=False, pad=None, counts=None):
    """tumor_crop (:716-742): around a random voxel of a random lesion class that is present."""
    r = crop_planned(tensor_img, tensor_lab, lambda t, s: plan_tumor_crop(t, lesion_classes, s, [d, h, w]), [d, h, w], pad, counts)
    return (r[0], r[1], r[2].crop_organ) if return_crop_organ else r[:2]


def crop_around_coordinate_3d(tensor_img, tensor_lab, crop_size, coordinate, mode, foreground=None, pad=None):
    """crop_around_coordinate_3d (:498-559).  coordinate: three ints, or for 'small_rnd_shift' a (3,) int32 device tensor (select_voxel's output), which
    is then never read by the host.  'random' and 'center' compute their corner on the host, so a device coordinate is read once for them."""
    assert mode in ['random', 'center', 'small_rnd_shift'], "Invalid Mode, should be 'random' or 'center'"
    if isinstance(crop_size, int):
        crop_size = [crop_size] * 3
    crop_size = [int(c) for c in crop_size]
    _need_device('crop_around_coordinate_3d', tensor_img)
    planes, _, _ = _label_planes(tensor_lab, 'crop_around_coordinate_3d')
    full, _ = padded_size(tensor_img.shape[2:], pad)
    if any(c > f for c, f in zip(crop_size, full)):
        raise ValueError('crop %s is larger than the (padded) volume %s' % (crop_size, full))
    vols = [planes]
    if foreground is not None:
        fg = _as_bytes(foreground, 'foreground')
        vols.append(fg.reshape((1,) * (5 - fg.ndim) + tuple(fg.shape)))
    on_device = isinstance(coordinate, torch.Tensor) and coordinate.is_cuda
    if mode == 'small_rnd_shift':
        offs = [int(np.random.randint(-int(c * 0.5), int(c * 0.5) + 1)) for c in crop_size]
        if on_device:
            out, outs, _ = crop_box(tensor_img, vols, crop_size, pad=full, center=coordinate.to(torch.int32), offset=offs)
        else:
            org = [int(np.clip(int(z) - c // 2 + o, 0, f - c)) for z, c, o, f in zip(coordinate, crop_size, offs, full)]
            out, outs, _ = crop_box(tensor_img, vols, crop_size, pad=full, origin=org)
    else:
        zyx = [int(v) for v in (coordinate.tolist() if isinstance(coordinate, torch.Tensor) else coordinate)]
        if mode == 'random':
            org = [int(np.random.randint(max(0, z - c), min(f - c, z + c))) for z, c, f in zip(zyx, crop_size, full)]
        else:
            org = [min(max(0, z - math.ceil(c / 2)), f - c) for z, c, f in zip(zyx, crop_size, full)]
        out, outs, _ = crop_box(tensor_img, vols, crop_size, pad=full, origin=org)
    res = (out, _label_like(tensor_lab, outs[0]))
    return res + (outs[1].to(foreground.dtype),) if foreground is not None else res


# ---------------------------------------------------------------------------------------------------------------------------
# The report-annotated crop on the device (csrc/crop_report.hip): crop_foreground_3d (augmentation.py:790) and denoise_mask (:746) for a whole
# CT whose label is a PackedBits.  The foreground of a report crop is a union of segment classes: rsuper_union_bbox gives its voxel count and
# bounding box in one pass over the packed planes the set touches (the reference sums inflated planes and calls torch.nonzero), and only
# when that box is larger than the crop does the opening run -- on the bits of the box alone (rsuper_union_bits, rsuper_bits_open), followed
# by rsuper_largest_component on the box's u8 mask.  Restricting the opening to the mask's own bounding box is exact: an erosion reads zero
# outside either way, and a dilation step can only set a voxel outside the box from a voxel inside it, which the final `& m` clears again
# while nothing outside ever feeds back in (the L1 path between two voxels of a box stays in the box).  No CPU kernel.
# ---------------------------------------------------------------------------------------------------------------------------
OPEN_MAX_RADIUS = 4        # RSUPER_OPEN_MAX_RADIUS of the header
ZERO_MASK, NO_FIT = 'zero mask', 'mask does not fit crop size'      # crop_foreground_3d's two strings (:849, :908)


def class_set(classes):
    """Class indices (or one 64-bit set) -> the 64-bit set the union kernels take: bit c = class c."""
    if isinstance(classes, int):
        return classes
    s = 0
    for c in classes:
        if not 0 <= int(c) < 64:
            raise ValueError('class_set: class %r outside [0, 64)' % (c,))
        s |= 1 << int(c)
    return s


def _signed64(v):
    v = int(v) & 0xFFFFFFFFFFFFFFFF
    return v - (1 << 64) if v >> 63 else v


def _count_box(B, device):
    """One int64 buffer that holds count [B] int64 and bbox [B][6] int32, so that both come to the host in one read."""
    buf = torch.empty((4 * B,), device=device, dtype=torch.int64)
    return buf, buf[:B], buf[B:].view(torch.int32).view(B, 6)


def _read_count_box(buf, B=1):
    """-> [(count, [min z, y, x, max z, y, x])] per sample: the one device-to-host read."""
    h = buf.cpu()
    box = h[B:].view(torch.int32).view(B, 6).tolist()
    return [(int(h[b]), box[b]) for b in range(B)]


def _union_bbox(packed, C, plain, sets):
    """The C ABI call.  packed (B, P, D, H, W) u8, sets: B ints -> the (4 B,) int64 buffer of _count_box."""
    import ctypes
    from ..hip import lib as _l
    _need_device('union_bbox', packed)
    if packed.dim() != 5 or packed.dtype != torch.uint8 or not packed.is_contiguous():
        raise ValueError('union_bbox: the label must be contiguous uint8 (B, P, D, H, W), got %s %s' % (packed.dtype, tuple(packed.shape)))
    B, P, D, H, W = packed.shape
    if len(sets) != B:
        raise ValueError('union_bbox: one class set per sample')
    L = _l.lib()
    ws = torch.empty((max(L.rsuper_union_bbox_workspace_bytes(B, D, H, W), 1),), device=packed.device, dtype=torch.uint8)
    buf, count, bbox = _count_box(B, packed.device)
    with torch.cuda.device(packed.device):
        _l.check(L.rsuper_union_bbox(packed.data_ptr(), B, P, int(C), int(bool(plain)), D, H, W,
                                     (ctypes.c_ulonglong * B)(*[int(s) & 0xFFFFFFFFFFFFFFFF for s in sets]), ws.data_ptr(), ws.numel(),
                                     count.data_ptr(), bbox.data_ptr(), torch.cuda.current_stream().cuda_stream), 'union_bbox')
    return buf


def _union_bits(packed, C, plain, b, cset, box):
    """The C ABI call.  box: (z0, y0, x0, nz, ny, nx) -> (nz, ny, ceil(nx / 64)) int64 device tensor of the bit words."""
    from ..hip import lib as _l
    _need_device('union_bits', packed)
    if packed.dim() != 5 or packed.dtype != torch.uint8 or not packed.is_contiguous():
        raise ValueError('union_bits: the label must be contiguous uint8 (B, P, D, H, W)')
    B, P, D, H, W = packed.shape
    z0, y0, x0, nz, ny, nx = (int(v) for v in box)
    if min(nz, ny, nx) < 1:
        raise ValueError('union_bits: an empty box %s' % (tuple(box),))
    bits = torch.empty((nz, ny, (nx + 63) // 64), device=packed.device, dtype=torch.int64)
    with torch.cuda.device(packed.device):
        _l.check(_l.lib().rsuper_union_bits(packed.data_ptr(), B, P, int(C), int(bool(plain)), D, H, W, int(b), int(cset) & 0xFFFFFFFFFFFFFFFF,
                                            z0, y0, x0, nz, ny, nx, bits.data_ptr(), torch.cuda.current_stream().cuda_stream), 'union_bits')
    return bits


def _bits_open(bits, nx, r, add):
    """The C ABI call.  bits (nz, ny, ceil(nx / 64)) int64 -> (opened bits, (nz, ny, nx) u8 mask, the (4,) int64 count + bbox buffer)."""
    from ..hip import lib as _l
    _need_device('bits_open', bits)
    nx = int(nx)
    if bits.dim() != 3 or bits.dtype != torch.int64 or not bits.is_contiguous() or nx < 1 or bits.shape[2] != (nx + 63) // 64:
        raise ValueError('bits_open: bits must be a contiguous int64 (nz, ny, ceil(nx / 64)) tensor')
    nz, ny = int(bits.shape[0]), int(bits.shape[1])
    L = _l.lib()
    ws = torch.empty((max(L.rsuper_bits_open_workspace_bytes(nz, ny, nx), 8) // 8,), device=bits.device, dtype=torch.int64)
    out = torch.empty_like(bits)
    mask = torch.empty((nz, ny, nx), device=bits.device, dtype=torch.uint8)
    buf, count, bbox = _count_box(1, bits.device)
    with torch.cuda.device(bits.device):
        _l.check(L.rsuper_bits_open(bits.data_ptr(), nz, ny, nx, int(r), int(add[0]), int(add[1]), int(add[2]), ws.data_ptr(), ws.numel() * 8,
                                    out.data_ptr(), mask.data_ptr(), count.data_ptr(), bbox.data_ptr(), torch.cuda.current_stream().cuda_stream),
                 'bits_open')
    return out, mask, buf


def _label_remap(packed, C_in, C_out, nvol, masks, ones):
    """The C ABI call.  packed (B, P_in, d, h, w) u8; masks: B * nvol * C_out ints, ones: B * nvol ints -> nvol (B, ceil(C_out / 8), d, h, w) u8."""
    import ctypes
    from ..hip import lib as _l
    _need_device('label_remap', packed)
    if packed.dim() != 5 or packed.dtype != torch.uint8 or not packed.is_contiguous():
        raise ValueError('label_remap: the label must be contiguous uint8 (B, P, d, h, w)')
    B, P = int(packed.shape[0]), int(packed.shape[1])
    nvol, C_in, C_out = int(nvol), int(C_in), int(C_out)
    if len(masks) != B * nvol * C_out or len(ones) != B * nvol or not 1 <= nvol <= 3:
        raise ValueError('label_remap: masks must hold B * nvol * C_out sets and ones B * nvol, nvol <= 3')
    v = packed[0, 0].numel()
    P_out = (C_out + 7) // 8
    outs = [torch.empty((B, P_out) + tuple(packed.shape[2:]), device=packed.device, dtype=torch.uint8) for _ in range(nvol)]
    u = 0xFFFFFFFFFFFFFFFF
    with torch.cuda.device(packed.device):
        _l.check(_l.lib().rsuper_label_remap(packed.data_ptr(), B, P, C_in, v, nvol, (ctypes.c_void_p * nvol)(*[o.data_ptr() for o in outs]), P_out, C_out,
                                             (ctypes.c_ulonglong * len(masks))(*[int(m) & u for m in masks]),
                                             (ctypes.c_ulonglong * len(ones))(*[int(o) & u for o in ones]),
                                             torch.cuda.current_stream().cuda_stream), 'label_remap')
    return outs


def _report_ops():
    from ..hip import ops as _ops          # noqa: F401
    from ..hip import library as _library
    return _library.install_report_crop_ops(_union_bbox, _union_bits, _bits_open, _label_remap)


def _mask_planes(mask, what):
    """A device mask (D, H, W) / (1, D, H, W) -> the plain one-class label (1, 1, D, H, W) u8 of the union kernels."""
    _need_device(what, mask)
    if mask.dim() == 4 and mask.shape[0] == 1:
        mask = mask[0]
    if mask.dim() != 3:
        raise ValueError('Foreground must be [D,H,W] or [1,D,H,W], got %s' % (tuple(mask.shape),))
    return _as_bytes(mask, what).contiguous()[None, None]


def union_bbox(lab, class_sets):
    """Voxel count and bounding box of the union of the classes of `class_sets` (one per sample: a 64-bit set or class indices) of a PackedBits or
    plain (B, C, D, H, W) label -> the device buffer `_read_count_box` turns into [(count, [min z, y, x, max z, y, x])] with one read
    (torch.ops.rsuper.union_bbox).  No voxel: min = (D, H, W), max = (-1, -1, -1)."""
    planes, C, plain = _label_planes(lab, 'union_bbox')
    return _report_ops()[0](planes, C, plain, [_signed64(class_set(s)) for s in class_sets])


def union_bits(lab, cset, box, b=0):
    """The union of the classes of `cset` of sample b inside box = (z0, y0, x0, nz, ny, nx) as (nz, ny, ceil(nx / 64)) int64 bit words: bit i of word
    k is voxel x0 + 64 k + i (torch.ops.rsuper.union_bits)."""
    planes, C, plain = _label_planes(lab, 'union_bits')
    return _report_ops()[1](planes, C, plain, int(b), _signed64(class_set(cset)), [int(v) for v in box])


def bits_open(bits, nx, iterations, add=(0, 0, 0)):
    """binary_dilation(binary_erosion(m, iterations), iterations) & m of a bit volume, zero outside (torch.ops.rsuper.bits_open) -> (bits, (nz, ny,
    nx) u8 mask, count + bbox buffer in box coordinates + add)."""
    if not 1 <= int(iterations) <= OPEN_MAX_RADIUS:
        raise ValueError('bits_open: 1 <= iterations <= %d, got %r' % (OPEN_MAX_RADIUS, iterations))
    return _report_ops()[2](bits, int(nx), int(iterations), [int(v) for v in add])


def label_remap(lab, C_out, masks, ones):
    """lab: PackedBits (B, C_in, d, h, w); masks [B][nvol][C_out] and ones [B][nvol] as nested lists of 64-bit sets -> nvol PackedBits of C_out classes:
    class j of volume k = (the voxel's classes & masks[b][k][j]) != 0 or bit j of ones[b][k] (torch.ops.rsuper.label_remap)."""
    nvol = len(ones[0])
    flat_m = [_signed64(m) for sample in masks for vol in sample for m in vol]
    flat_o = [_signed64(o) for sample in ones for o in sample]
    outs = _report_ops()[3](lab.packed, lab.C, int(C_out), nvol, flat_m, flat_o)
    return tuple(type(lab)(o, int(C_out)) for o in outs)


def _open_box(planes, C, plain, cset, box, lo_corner, iterations, connected_component=True):
    """The opening of the union inside its bounding box `box` = [min z, y, x, max z, y, x] (real coordinates), then the largest component.
    -> (count, bbox in coordinates + lo_corner, (nz, ny, nx) u8 mask of the box), count == 0: nothing is left.  Two device-to-host reads at the most:
    the opening's count (the largest-component kernel answers all ones for an empty mask, so it must not run on one) and the component's box."""
    from ..inference.postprocess import keep_largest_component
    z0, y0, x0 = box[:3]
    nz, ny, nx = (box[3 + i] - box[i] + 1 for i in range(3))
    add = [z0 + lo_corner[0], y0 + lo_corner[1], x0 + lo_corner[2]]
    bits = _report_ops()[1](planes, C, plain, 0, _signed64(cset), [z0, y0, x0, nz, ny, nx])
    _, mask, buf = _report_ops()[2](bits, nx, int(iterations), add)
    (count, bbox), = _read_count_box(buf)
    if count == 0 or not connected_component:
        return count, bbox, mask
    mask = keep_largest_component(mask)
    (count, bbox), = _read_count_box(_report_ops()[0](mask[None, None], 1, True, [1]))
    return count, [v + add[i % 3] for i, v in enumerate(bbox)], mask


def denoise_mask(mask_3d, iterations=2, connected_component=True):
    """denoise_mask (:746-787) on a device mask (D, H, W): `iterations` erosions and dilations with scipy's cross, AND with the mask, then the largest
    face-connected component (ties: the first in C order, as np.argmax over ndimage.label's counts).  -> bool (D, H, W) on the device."""
    planes = _mask_planes(mask_3d, 'denoise_mask')
    (count, box), = _read_count_box(_report_ops()[0](planes, 1, True, [1]))
    out = torch.zeros(tuple(planes.shape[2:]), device=planes.device, dtype=torch.bool)
    if count == 0:
        return out
    count, _, sub = _open_box(planes, 1, True, 1, box, [0, 0, 0], iterations, connected_component)
    if count:
        out[box[0]:box[3] + 1, box[1]:box[4] + 1, box[2]:box[5] + 1] = sub.bool()
    return out


def bbox_with_margin(bbox, size, margin=1):
    """[min z, y, x, max z, y, x] widened by the margin and clamped to the volume, with the reference's swaps (:857-872)."""
    margin = (margin,) * 3 if isinstance(margin, int) else tuple(margin)
    lo = [max(int(bbox[i]) - margin[i], 0) for i in range(3)]
    hi = [min(int(bbox[3 + i]) + margin[i], int(size[i]) - 1) for i in range(3)]
    for i in range(3):
        if lo[i] > hi[i]:
            lo[i], hi[i] = hi[i], lo[i]
    return lo + hi


def bbox_fits(box, crop_size):
    return all(box[3 + i] - box[i] + 1 <= int(crop_size[i]) for i in range(3))


def plan_crop_foreground(bbox, size, crop_size, margin=1, rand=True):
    """The host part of crop_foreground_3d after the bounding box is known (:857-966): margin, clamp and swaps, the size test, valid_shifts_1D, and the
    random.randint draws in z, y, x order (rand=False: the middle of the range).  bbox: [min z, y, x, max z, y, x] of the foreground in the
    coordinates of `size`.  -> the crop's corner [z, y, x], or 'mask does not fit crop size'."""
    import random
    box = bbox_with_margin(bbox, size, margin)
    if not bbox_fits(box, crop_size):
        return NO_FIT
    rng = []
    for i in range(3):
        low = max(box[3 + i] - (int(crop_size[i]) - 1), 0)
        high = min(box[i], int(size[i]) - int(crop_size[i]))
        rng.append((int(low), int(high)))
    if any(low > high for low, high in rng):
        return NO_FIT
    return [random.randint(low, high) if rand else (low + high) // 2 for low, high in rng]


def crop_foreground_3d(tensor_ct, tensor_lab, foreground, crop_size, margin=1, refine_iterations=3, rand=True, pad=None, count_box=None):
    """crop_foreground_3d (:790-1019) on a device volume (1, 1, D, H, W) f32 / int16 and a PackedBits or plain (1, C, D, H, W) label.  foreground: a
    device mask (D, H, W) / (1, D, H, W), or the classes of tensor_lab whose union it is (a 64-bit set or class indices; PackedBits label).  All
    coordinates are those of the volume padded to `pad` as pad_volume_pair pads (no padded copy is made).  -> (image crop, label crop of
    tensor_lab's kind, bool (d, h, w) crop of the foreground, or of the refined mask when the opening ran), or 'zero mask' /
    'mask does not fit crop size'.  One device-to-host read, three when the opening runs; count_box: the (count, box) of the foreground when the
    caller has already read it."""
    _need_device('crop_foreground_3d', tensor_ct)
    if tensor_ct.dim() != 5 or tensor_ct.shape[0] != 1 or tensor_ct.shape[1] != 1:
        raise ValueError('CT must be [1,1,D,H,W], got %s' % (tuple(tensor_ct.shape),))
    planes, C, plain = _label_planes(tensor_lab, 'crop_foreground_3d')
    size = tuple(tensor_ct.shape[2:])
    if tuple(planes.shape[2:]) != size:
        raise ValueError('The input and label tensors must have the same spatial dimensions.')
    crop = [int(c) for c in ([crop_size] * 3 if isinstance(crop_size, int) else crop_size)]
    full, lo = padded_size(size, pad)
    if any(c > f for c, f in zip(crop, full)):
        raise ValueError('crop %s is larger than the (padded) volume %s' % (crop, full))
    if isinstance(foreground, torch.Tensor):
        fplanes, fC, fplain, cset = _mask_planes(foreground, 'crop_foreground_3d'), 1, True, 1
        if tuple(fplanes.shape[2:]) != size:
            raise ValueError('The foreground must be on the image grid')
    else:
        fplanes, fC, fplain, cset = planes, C, plain, class_set(foreground)
    count, box = count_box if count_box is not None else _read_count_box(_report_ops()[0](fplanes, fC, fplain, [_signed64(cset)]))[0]
    if count == 0:
        return ZERO_MASK
    padded_box = [v + lo[i % 3] for i, v in enumerate(box)]
    refined = None
    if not bbox_fits(bbox_with_margin(padded_box, full, margin), crop):
        count, padded_box, refined = _open_box(fplanes, fC, fplain, cset, box, lo, refine_iterations)
        if count == 0:
            return ZERO_MASK
    corner = plan_crop_foreground(padded_box, full, crop, margin, rand)
    if isinstance(corner, str):
        return corner
    vols = [planes] if refined is not None or fplain is False or fplanes is planes else [planes, fplanes[:, 0:1]]
    img, outs, _ = crop_box(tensor_ct, vols, crop, pad=full, origin=corner)
    if refined is not None:
        fg = torch.zeros(crop, device=planes.device, dtype=torch.bool)
        o = [box[i] + lo[i] - corner[i] for i in range(3)]                   # the box's origin in the crop
        a = [max(0, -o[i]) for i in range(3)]
        e = [min(refined.shape[i], crop[i] - o[i]) for i in range(3)]
        fg[o[0] + a[0]:o[0] + e[0], o[1] + a[1]:o[1] + e[1], o[2] + a[2]:o[2] + e[2]] = refined[a[0]:e[0], a[1]:e[1], a[2]:e[2]].bool()
    elif len(vols) == 2:
        fg = outs[1][0, 0] != 0
    elif plain:
        fg = (outs[0][0] != 0)[[c for c in range(C) if cset >> c & 1]].any(0)
    else:
        fg = _report_ops()[3](outs[0].contiguous(), C, 1, 1, [_signed64(cset)], [0])[0][0, 0] != 0
    return img, _label_like(tensor_lab, outs[0]), fg
