"""MI355X tests of the device intensity augmentation (training/augmentation.py intensity_augment_batch, kernel csrc/augment_intensity.hip; every launch
goes through the C ABI rsuper_intensity_augment) against the reference's own outputs in tests/golden/loader.npz where it has them and against the CPU
functions of training/augmentation.py (which tests/test_loader_cpu.py pins to the reference at 2e-5) elsewhere.

The rule of every comparison (check): E64 = the float64 restatement of the chain (tests/intensity_ref.py), R = the reference's / the CPU functions'
float32 output, e_ref = max |R - E64|; required: max |kernel - E64| <= max(2 * e_ref, ulp32(max |E64|)).  The factor 2 admits another equally valid
float32 operation order, the floor is the rounding any float32 result carries.
"""
import contextlib
import ctypes
import os
import sys
from unittest import mock

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import intensity_ref as IR  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'loader.npz'))
NOISE_STD = 0.137                                        # the std of the gaussian_noise fixtures (tests/golden/gen_golden_loader.py)


def A():
    from rsuper_amd.training import augmentation
    return augmentation


def run(x, plan, noise=None):
    """x (B, 1, D, H, W) CPU tensor -> the device result as a CPU tensor."""
    out = A().intensity_augment_batch(x.to(DEV), plan, None if noise is None else noise.to(DEV))
    torch.cuda.synchronize()
    return out.cpu()


@contextlib.contextmanager
def forced_draws(additive=None, noise=None):
    """The CPU functions draw their own parameter; with torch.rand returning 0 a range (v, v + 1) yields exactly v, torch.normal / torch.randn return
    the given offset / field."""
    def zeros(*a, **kw):
        return torch.zeros(kw['size'] if 'size' in kw else a)
    with mock.patch.object(torch, 'rand', zeros), \
            mock.patch.object(torch, 'normal', lambda *a, **kw: torch.full(kw['size'], additive, dtype=torch.float32)), \
            mock.patch.object(torch, 'randn', lambda *a, **kw: noise.reshape(a[0])):
        yield


def cpu_chain(x, plan, b, noise=None):
    """Sample b of the plan through the CPU functions of training/augmentation.py in the loader's order; x (1, 1, D, H, W)."""
    a, on = A(), lambda k: plan.flags[b] >> k & 1
    with forced_draws(plan.additive[b], noise):
        if on(0):
            x = a.brightness_multiply(x, multiply_range=(plan.multiply[b], plan.multiply[b] + 1))
        if on(1):
            x = a.brightness_additive(x, std=0.1)
        if on(2):
            x = a.gamma(x, gamma_range=(plan.gamma[b], plan.gamma[b] + 1))
        if on(3):
            x = a.contrast(x, contrast_range=(plan.contrast[b], plan.contrast[b] + 1))
        if on(4):
            x = a.gaussian_blur(x, sigma_range=(plan.sigma[b], plan.sigma[b] + 1))
        if on(5):
            x = a.gaussian_noise(x, std=plan.noise_std[b])
    return x


RATIOS = {}


def check(what, got, R, E64):
    got, R = np.asarray(got, dtype=np.float64), np.asarray(R, dtype=np.float64)
    e_ref = float(np.abs(R - E64).max())
    err = float(np.abs(got - E64).max())
    bound = max(2 * e_ref, float(np.spacing(np.float32(np.abs(E64).max()))))
    RATIOS[what] = err / bound
    print('%s: |kernel - f64| %.3g, e_ref %.3g, bound %.3g, ratio %.3f' % (what, err, e_ref, bound, err / bound))
    assert np.isfinite(E64).all() and err <= bound, '%s: error %.3g exceeds max(2 * e_ref, ulp) = %.3g (e_ref %.3g)' % (what, err, bound, e_ref)


def volume(shape, seed, scale=1.0, shift=0.0):
    rs = np.random.RandomState(seed)
    return torch.from_numpy((rs.standard_normal((1, 1) + tuple(shape)) * scale + shift).astype(np.float32))


def fixture_input():
    return torch.from_numpy(synth.loader_crop(0, synth.TINY_CLASSES)[0]).unsqueeze(0)


# ------------------------------------------------------------------------------------------------------------------ 1: the reference fixtures
@pytest.mark.parametrize('s', [11, 12])
@pytest.mark.parametrize('name', ['brightness_multiply', 'brightness_additive', 'gamma', 'contrast', 'gaussian_blur', 'gaussian_noise'])
def test_single_transform_matches_reference_fixture(name, s):
    x = fixture_input()
    R = G['aug_%s_%d' % (name, s)]
    torch.manual_seed(s)                                   # the parameter is re-drawn exactly as tests/test_loader_cpu.py draws it
    noise = None
    if name == 'brightness_multiply':
        kw = dict(multiply=[torch.rand(size=(1, 1, 1, 1, 1)) * (1.3 - 0.7) + 0.7])
    elif name == 'brightness_additive':
        kw = dict(additive=[torch.normal(0.0, 0.1, size=(1, 1, 1, 1, 1))])
    elif name == 'gamma':
        kw = dict(gamma=[torch.rand(1, 1) * (1.5 - 0.7) + 0.7])
    elif name == 'contrast':
        kw = dict(contrast=[torch.rand(1, 1) * (1.3 - 0.7) + 0.7])
    elif name == 'gaussian_blur':
        kw = dict(sigma=[torch.rand(1) * (1.5 - 0.5) + 0.5])
    else:
        kw = dict(noise_std=[NOISE_STD])
        noise = torch.from_numpy(((R.astype(np.float64) - x.numpy()) / NOISE_STD).astype(np.float32))
    plan = A().make_intensity_plan(1, **kw)
    got = run(x, plan, noise)
    assert got.shape == x.shape and got.dtype == torch.float32
    check('%s seed %d' % (name, s), got[0, 0], R[0, 0], IR.apply_plan(x[0, 0].numpy(), plan, 0, None if noise is None else noise[0, 0].numpy()))


# ------------------------------------------------------------------------------------------------------------------ 2, 3, 6: combinations and sizes
ALL = dict(multiply=[1.2], additive=[-0.07], gamma=[1.3], contrast=[1.25], sigma=[1.1], noise_std=[0.15])
CASES = {
    'all six': ((16, 20, 12), ALL),
    'gamma + contrast': ((16, 20, 12), dict(gamma=[0.8], contrast=[1.3])),
    'contrast + blur, offset 2': ((16, 20, 12), dict(additive=[2.0], contrast=[0.75], sigma=[0.9])),
    'ragged 9x10x13 r=5': ((9, 10, 13), dict(ALL, sigma=[1.5])),
    '33x34x36 r=2': ((33, 34, 36), dict(ALL, sigma=[0.6])),
    '33x34x36 r=5': ((33, 34, 36), dict(ALL, sigma=[1.45])),
}


def case(name):
    shape, kw = CASES[name]
    x = volume(shape, len(name), scale=1.3, shift=0.4)
    noise = volume(shape, 100 + len(name)) if 'noise_std' in kw else None
    return x, noise, A().make_intensity_plan(1, **kw)


@pytest.mark.parametrize('name', list(CASES))
def test_combinations_against_the_cpu_functions(name):
    x, noise, plan = case(name)
    assert plan.radius[0] == {'ragged 9x10x13 r=5': 5, '33x34x36 r=2': 2, '33x34x36 r=5': 5}.get(name, plan.radius[0])
    got = run(x, plan, noise)
    check(name, got[0, 0], cpu_chain(x, plan, 0, noise)[0, 0], IR.apply_plan(x[0, 0].numpy(), plan, 0, None if noise is None else noise[0, 0].numpy()))


def test_two_runs_are_bit_identical():
    x, noise, plan = case('all six')
    a, b = run(x, plan, noise), run(x, plan, noise)
    assert torch.equal(a, b)
    x, noise, plan = case('33x34x36 r=5')
    plan.seed[0] = 99
    assert torch.equal(run(x, plan), run(x, plan))         # the in-kernel field as well


# ------------------------------------------------------------------------------------------------------------------ 4: batches
def test_batch_equals_single_samples_and_an_unfired_sample_is_the_input():
    B, shape = 3, (12, 20, 24)
    x = torch.cat([volume(shape, 40 + b, scale=1 + b, shift=b - 1.0) for b in range(B)])
    plan = A().make_intensity_plan(B, multiply=[0.8, None, None], additive=[None, None, 0.3], gamma=[1.4, None, None], contrast=[1.1, None, 0.8],
                                   sigma=[0.5, None, 1.4], noise_std=[0.1, None, 0.05], seed=[5, 6, (1 << 63) + 7])
    assert plan.flags[1] == 0 and plan.radius == [2, 0, 5]
    got = run(x, plan)
    assert torch.equal(got[1].view(torch.int32), x[1].view(torch.int32))
    for b in range(B):
        one = A().make_intensity_plan(1, **{k: [getattr(plan, k)[b] if plan.flags[b] >> j & 1 else None]
                                            for j, k in enumerate(('multiply', 'additive', 'gamma', 'contrast', 'sigma', 'noise_std'))}, seed=[plan.seed[b]])
        assert one.flags == [plan.flags[b]] and one.taps[0] == plan.taps[b]
        single = run(x[b:b + 1], one) if one.flags[0] else x[b:b + 1]
        assert torch.equal(got[b:b + 1].view(torch.int32), single.view(torch.int32)), b
    # more than one launch's worth of samples: sample 9 of a batch of 10 is sample 0 above
    big = A().make_intensity_plan(10, **{k: [None] * 9 + [getattr(plan, k)[0]] for k in ('multiply', 'additive', 'gamma', 'contrast', 'sigma', 'noise_std')},
                                  seed=[0] * 9 + [5])
    out = run(torch.cat([x[1:2]] * 9 + [x[0:1]]), big)
    assert torch.equal(out[9], got[0]) and torch.equal(out[:9], torch.cat([x[1:2]] * 9))


def test_nothing_fired_returns_the_input_without_a_launch():
    x = volume((8, 8, 8), 1).to(DEV)
    assert A().intensity_augment_batch(x, A().make_intensity_plan(1)) is x


# ------------------------------------------------------------------------------------------------------------------ 5: the in-kernel noise field
def test_in_kernel_noise_field():
    shape, seed = (32, 32, 64), 0x1234567890ABCDEF
    N = int(np.prod(shape))
    zeros = torch.zeros((1, 1) + shape)
    mk = lambda seeds: A().make_intensity_plan(len(seeds), noise_std=[1.0] * len(seeds), seed=seeds)
    got = run(zeros, mk([seed]))
    f64 = IR.noise_field(seed, N).reshape(shape)
    f32 = IR.noise_field(seed, N, np.float32).astype(np.float64).reshape(shape)
    err, ref = float(np.abs(got[0, 0].numpy() - f64).max()), float(np.abs(f32 - f64).max())
    print('noise field: |kernel - f64| %.3g, |f32 numpy - f64| %.3g, ratio %.3f of 4' % (err, ref, err / ref))
    assert err <= 4 * ref
    v = got.double()
    assert abs(float(v.mean())) <= 5 / np.sqrt(N) and abs(float(v.std()) - 1) <= 5 / np.sqrt(2 * N)
    assert torch.equal(got, run(zeros, mk([seed])))
    assert not torch.equal(got, run(zeros, mk([seed + 1])))
    both = run(torch.zeros((2, 1) + shape), mk([seed + 1, seed]))           # another batch size and position: the same field for the same seed
    assert torch.equal(both[1:2], got)
    ragged = run(torch.zeros((1, 1, 5, 7, 9)), mk([seed]))                   # scalar path: the field is a function of the linear index
    assert np.array_equal(ragged.numpy().reshape(-1), got.numpy().reshape(-1)[:5 * 7 * 9])


# ------------------------------------------------------------------------------------------------------------------ 7: degenerate input
def test_constant_volume_under_gamma_is_nan_where_the_cpu_function_is():
    x = torch.full((1, 1, 8, 12, 16), 0.75)
    plan = A().make_intensity_plan(1, gamma=[1.2])
    exp = cpu_chain(x, plan, 0)
    assert bool(torch.isnan(exp).all())
    got = run(x, plan)
    assert torch.equal(torch.isnan(got), torch.isnan(exp))
    plan = A().make_intensity_plan(1, gamma=[1.2], contrast=[1.1], sigma=[0.5], noise_std=[0.1])
    assert torch.equal(torch.isnan(run(x, plan)), torch.isnan(cpu_chain(x, plan, 0, torch.zeros_like(x))))


# ------------------------------------------------------------------------------------------------------------------ 8: rejections
def test_rejections_launch_nothing():
    from rsuper_amd.hip import lib
    L, R = lib.lib(), lib.BLUR_MAX_RADIUS
    x = volume((8, 12, 16), 2).to(DEV)
    big = A().make_intensity_plan(1, sigma=[(R + 1) / 3.0 + 0.2])
    assert big.radius[0] > R
    with pytest.raises(lib.RSuperHipError):
        A().intensity_augment_batch(x, big)
    with pytest.raises(ValueError):
        A().intensity_augment_batch(torch.cat([x, x], 1), A().make_intensity_plan(1, multiply=[1.1]))
    with pytest.raises(ValueError):
        A().intensity_augment_batch(x.double(), A().make_intensity_plan(1, multiply=[1.1]))
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.rsuper.intensity_augment(x.cpu(), [1], [1.1, 0.0, 0.0, 0.0, 0.0], [0], [0.0] * (2 * R + 1), [0])
    # the C ABI itself: error code, output untouched
    out = torch.full_like(x, 7.0)
    ws = torch.empty(L.rsuper_intensity_augment_workspace_bytes(1, 8, 12, 16), device=DEV, dtype=torch.uint8)
    st = torch.cuda.current_stream().cuda_stream

    def call(flags=16, radius=1, img=x.data_ptr(), dst=out.data_ptr(), dims=(8, 12, 16), wsp=ws.data_ptr(), wsb=ws.numel()):
        return L.rsuper_intensity_augment(img, dst, 1, *dims, (ctypes.c_int * 1)(flags), (ctypes.c_float * 5)(1, 0, 1, 1, 0), (ctypes.c_int * 1)(radius),
                                          (ctypes.c_float * (2 * R + 1))(0.25, 0.5, 0.25), (ctypes.c_ulonglong * 1)(0), None, wsp, wsb, st)
    for kw in (dict(radius=R + 1), dict(radius=-1), dict(flags=64), dict(flags=-1), dict(img=None), dict(dst=None), dict(dst=x.data_ptr()), dict(dims=(0, 12, 16)),
               dict(flags=4, wsp=None), dict(flags=8, wsb=8)):
        assert call(**kw) == 1, kw
    torch.cuda.synchronize()
    assert bool((out == 7).all()), 'a rejected call must not launch'
    assert call() == 0 and call(flags=1, wsp=None, wsb=0) == 0               # no workspace needed without gamma / contrast
    torch.cuda.synchronize()
    assert torch.equal(out, x)                                               # multiply by 1


# ------------------------------------------------------------------------------------------------------------------ 9: full size, and downstream
def test_full_size_everything_fired_then_spatial_augmentation():
    B, shape = 2, (116, 136, 136)
    x = torch.cat([volume(shape, 70 + b, scale=0.8 + 0.3 * b, shift=0.2 * b) for b in range(B)])
    noise = torch.cat([volume(shape, 80 + b) for b in range(B)])
    plan = A().make_intensity_plan(B, multiply=[1.25, 0.75], additive=[0.05, -0.1], gamma=[0.75, 1.45], contrast=[1.3, 0.7], sigma=[0.55, 1.5],
                                   noise_std=[0.19, 0.02])
    assert plan.radius == [2, 5] and A().intensity_launches(plan) == 3
    dev = A().intensity_augment_batch(x.to(DEV), plan, noise.to(DEV))
    got = dev.cpu()
    for b in range(B):
        check('full size sample %d' % b, got[b, 0], cpu_chain(x[b:b + 1], plan, b, noise[b:b + 1])[0, 0],
              IR.apply_plan(x[b, 0].numpy(), plan, b, noise[b, 0].numpy()))
    np.random.seed(4)
    lab = torch.zeros((B, 1) + shape, dtype=torch.uint8, device=DEV)
    crop, _ = A().spatial_augment_batch(dev, (lab,), [96, 96, 96], 0.3, 45, 0.1)
    assert crop.shape == (B, 1, 96, 96, 96) and bool(torch.isfinite(crop).all())


@pytest.mark.parametrize('aug_device', ['gpu', 'cpu'])
def test_training_with_intensity_aug_device_gpu_on_the_synthetic_dataset(tmp_path, aug_device):
    from rsuper_amd.train_ddp import get_parser, main_worker, SOURCE_MARGIN
    from rsuper_amd.training.dataset import SyntheticUFODataset
    classes = ['kidney_left', 'kidney_right', 'liver', 'pancreas', 'pancreatic_lesion']
    args = get_parser(['--epochs', '1', '--batch_size', '2', '--cp_path', str(tmp_path) + '/', '--unique_name', 'intdev', '--loss', 'ball_dice_last',
                       '--report_volume_loss_basic', '0.1', '--aug_device', aug_device, '--intensity_aug_device', 'gpu', '--crop_size', '32'])
    args.base_chan, args.iter_per_epoch, args.print_freq, args.compute_dtype = 8, 2, 100, 'f32'
    gpu = aug_device == 'gpu'
    ds = SyntheticUFODataset(classes, size=32, length=6, seed=3, packed=gpu, margin=SOURCE_MARGIN if gpu else (0, 0, 0))
    np.random.seed(0); torch.manual_seed(0)
    with mock.patch('rsuper_amd.train_ddp.intensity_augment_batch', wraps=A().intensity_augment_batch) as spy:
        hist = main_worker(0, 1, 0, args, trainset=ds)
    assert spy.call_count >= 2 and all(tuple(c.args[0].shape[2:]) == ((52, 72, 72) if gpu else (32, 32, 32)) for c in spy.call_args_list)
    assert len(hist) == 1 and 'overall' in hist[0] and all(np.isfinite(v) for v in hist[0].values()), hist
