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
