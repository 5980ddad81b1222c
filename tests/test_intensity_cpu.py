"""Host side of the device intensity augmentation (training/augmentation.py plan_intensity_augment / make_intensity_plan / intensity_augment_batch,
kernel csrc/augment_intensity.hip): the plan's draws against the reference's recorded gates and generator positions (tests/golden/loader.npz) and
against the CPU functions under the same seeds, the C ABI's declarations, the training option, and the Philox restatement of tests/intensity_ref.py
against the published known-answer vectors.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import intensity_ref as IR  # noqa: E402
import synth  # noqa: E402
from rsuper_amd.training import augmentation as aug  # noqa: E402
from rsuper_amd.training.dataset import augmented as A  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'loader.npz'))
SEEDS = [int(s) for s in G['seeds']]
HDR = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()


def seeded_plan(s, batch=1):
    np.random.seed(s)
    torch.manual_seed(s)
    return aug.plan_intensity_augment(batch)


@pytest.mark.parametrize('k', range(len(SEEDS)))
def test_plan_fires_the_reference_gates_and_leaves_numpy_where_the_reference_does(k):
    plan = seeded_plan(SEEDS[k])
    assert plan.flags == [int(G['gates'][k])]
    assert np.random.random() == float(G['load_%d_next_np' % k])
    assert plan.fired(0) == [n for j, n in enumerate(aug.INTENSITY_TRANSFORMS) if int(G['gates'][k]) >> j & 1]


@pytest.mark.parametrize('k', range(len(SEEDS)))
def test_plan_parameters_are_the_cpu_functions_draws_bit_for_bit(k, monkeypatch):
    """The CPU functions run under the same seeds with torch.rand / torch.normal recorded: the plan's f, a, g, c, sigma are the values those draws give
    (multiply and additive are also read back exactly from the functions' outputs on ones / zeros), and the taps are gaussian_kernel_1d's."""
    s, gates = SEEDS[k], int(G['gates'][k])
    plan = seeded_plan(s)
    draws = []
    rand, normal = torch.rand, torch.normal

    def rec(fn):
        def f(*a, **kw):
            draws.append(fn(*a, **kw))
            return draws[-1]
        return f
    monkeypatch.setattr(torch, 'rand', rec(rand))
    monkeypatch.setattr(torch, 'normal', rec(normal))
    torch.manual_seed(s)
    one, zero = torch.ones(1, 1, 2, 2, 2), torch.zeros(1, 1, 2, 2, 2)
    x = torch.from_numpy(synth.loader_crop(0, synth.TINY_CLASSES)[0]).unsqueeze(0)
    if gates & 1:
        f = aug.brightness_multiply(one, multiply_range=[0.7, 1.3])
        assert draws[-1].shape == (1, 1, 1, 1, 1) and float(f[0, 0, 0, 0, 0]) == plan.multiply[0]
    if gates & 2:
        a = aug.brightness_additive(zero, std=0.1)
        assert draws[-1].shape == (1, 1, 1, 1, 1) and float(a[0, 0, 0, 0, 0]) == plan.additive[0]
    if gates & 4:
        aug.gamma(x, gamma_range=[0.7, 1.5])
        assert draws[-1].shape == (1, 1) and float(draws[-1] * (1.5 - 0.7) + 0.7) == plan.gamma[0]
    if gates & 8:
        aug.contrast(x, contrast_range=[0.7, 1.3])
        assert draws[-1].shape == (1, 1) and float(draws[-1] * (1.3 - 0.7) + 0.7) == plan.contrast[0]
    if gates & 16:
        aug.gaussian_blur(x, sigma_range=[0.5, 1.5])
        sigma = draws[-1] * (1.5 - 0.5) + 0.5
        ks = 2 * int(np.ceil(3 * float(sigma))) + 1
        assert draws[-1].shape == (1,) and float(sigma) == plan.sigma[0] and plan.radius[0] == ks // 2
        assert plan.taps[0] == [float(t) for t in aug.gaussian_kernel_1d(ks, sigma)] and len(plan.taps[0]) == ks
    assert len(draws) == bin(gates & 31).count('1')
    for j, v in enumerate((plan.multiply, plan.additive, plan.gamma, plan.contrast, None, plan.noise_std)):
        if v is not None and not gates >> j & 1:
            assert v[0] == 0.0
    if gates & 32:
        assert 0.0 <= plan.noise_std[0] < 0.2 and 0 <= plan.seed[0] < 1 << 64 and plan.noise_std[0] == float(np.float32(plan.noise_std[0]))


@pytest.mark.parametrize('k', [k for k in range(len(SEEDS)) if not int(G['gates'][k]) & 32])
def test_loader_image_is_the_float64_chain_of_the_plan(k):
    """Ties the plan to what the loader computes: without noise (whose field differs by design) online_intensity_augmentation under the same seeds is the
    float64 restatement of the plan to float32 rounding -- the tolerance test_loader_cpu.py pins the CPU functions to the reference with."""
    s = SEEDS[k]
    x = torch.from_numpy(synth.loader_crop(int(G['load_%d_idx' % k]), synth.TINY_CLASSES)[0]).unsqueeze(0)
    plan = seeded_plan(s)
    np.random.seed(s)
    torch.manual_seed(s)
    y = A.online_intensity_augmentation(x)
    assert np.abs(y[0, 0].numpy() - IR.apply_plan(x[0, 0].numpy(), plan, 0)).max() <= 2e-5
    assert np.abs(G['load_%d_image' % k][0] - IR.apply_plan(x[0, 0].numpy(), plan, 0)).max() <= 2e-5


def test_batch_plan_is_the_per_sample_sequence():
    np.random.seed(3)
    torch.manual_seed(3)
    single = [aug.plan_intensity_augment(1) for _ in range(4)]
    both = seeded_plan(3, 4)
    assert both.flags == [p.flags[0] for p in single] and both.seed == [p.seed[0] for p in single]
    for name in ('multiply', 'additive', 'gamma', 'contrast', 'noise_std', 'sigma', 'radius', 'taps'):
        assert getattr(both, name) == [getattr(p, name)[0] for p in single], name


def test_make_intensity_plan_explicit_values():
    plan = aug.make_intensity_plan(3, multiply=[1.1, None, None], gamma=[None, 0.9, None], sigma=[0.5, 1.5, None], noise_std=[None, 0.1, None],
                                   seed=[None, (1 << 64) - 1, None])
    assert plan.flags == [1 | 16, 4 | 16 | 32, 0] and plan.radius == [2, 5, 0] and [len(t) for t in plan.taps] == [5, 11, 0]
    assert plan.multiply[0] == float(np.float32(1.1)) and plan.gamma[1] == float(np.float32(0.9)) and plan.seed[1] == (1 << 64) - 1
    assert plan.taps[1] == [float(t) for t in aug.gaussian_kernel_1d(11, torch.tensor([1.5]))]
    assert aug.make_intensity_plan(2).flags == [0, 0]
    with pytest.raises(ValueError):
        aug.make_intensity_plan(2, multiply=[1.0])


def test_c_abi_is_declared_in_header_and_signatures():
    from rsuper_amd.hip import lib
    for name in ('rsuper_intensity_augment', 'rsuper_intensity_augment_workspace_bytes', 'rsuper_intensity_augment_launches'):
        m = re.search(r'\b(?:int|long)\s+%s\s*\(([^;]*)\)\s*;' % name, HDR)
        assert m, '%s is not declared in include/rsuper_hip.h' % name
        assert name in lib._SIGS and len(lib._SIGS[name][1]) == len(m.group(1).split(',')), name
    m = re.search(r'#define\s+RSUPER_BLUR_MAX_RADIUS\s+(\d+)', HDR)
    assert m and int(m.group(1)) >= 5 and int(m.group(1)) == lib.BLUR_MAX_RADIUS


def test_workspace_query_runs_on_the_host():
    from rsuper_amd.hip import lib
    L = lib.lib()
    assert L.rsuper_intensity_augment_workspace_bytes(2, 116, 136, 136) > 0
    for shape in ((2, 0, 136, 136), (2, 116, 0, 136), (2, 116, 136, 0), (0, 116, 136, 136)):
        assert L.rsuper_intensity_augment_workspace_bytes(*shape) == 0, shape


def test_launch_budget():
    """The counts DESIGN 6f states: none fired 0, no gamma / contrast / blur 1, blur alone 1, contrast without gamma 2, everything at most 4."""
    mk = lambda **kw: aug.intensity_launches(aug.make_intensity_plan(2, **kw))
    assert mk() == 0
    assert mk(multiply=[1.1, None], additive=[None, 0.1], noise_std=[0.1, 0.1]) == 1
    assert mk(sigma=[1.0, None]) == 1
    assert mk(contrast=[None, 1.2], sigma=[1.0, None]) == 2
    assert mk(multiply=[1.1] * 2, additive=[0.1] * 2, gamma=[0.9] * 2, contrast=[1.2] * 2, sigma=[1.5] * 2, noise_std=[0.1] * 2) <= 4
    assert mk(gamma=[0.9, None]) == 3
    assert aug.intensity_launches(aug.make_intensity_plan(9, contrast=[1.2] + [None] * 8)) == 3      # 8 samples per launch: groups 0-7 and 8


def test_intensity_aug_device_option_reaches_the_training_loop(tmp_path):
    from rsuper_amd import train_ddp
    base = ['--model', 'unet', '--dimension', '3d', '--dataset', 'abdomenatlas_ufo', '--synthetic', '2']
    args = train_ddp.get_parser(base + ['--intensity_aug_device', 'gpu'])
    assert args.intensity_aug_device == 'gpu' and args.aug_device == 'cpu'
    assert train_ddp.source_size(args) == list(args.training_size)              # --aug_device keeps its own meaning
    assert train_ddp.get_parser(base).intensity_aug_device == 'cpu'
    # the YAML value is honoured when the flag is absent, and the flag wins over it
    src = os.path.join(ROOT, 'r-super_amd', 'config', 'abdomenatlas_ufo', 'unet_3d.yaml')
    text = open(src).read()
    assert re.search(r"^intensity_aug_device: 'cpu'", text, re.M)
    os.makedirs(tmp_path / 'abdomenatlas_ufo')
    with open(tmp_path / 'abdomenatlas_ufo' / 'unet_3d.yaml', 'w') as f:
        f.write(re.sub(r"(?m)^intensity_aug_device: 'cpu'", "intensity_aug_device: 'gpu'", text))
    assert train_ddp.get_parser(base, config_root=str(tmp_path)).intensity_aug_device == 'gpu'
    assert train_ddp.get_parser(base + ['--intensity_aug_device', 'cpu'], config_root=str(tmp_path)).intensity_aug_device == 'cpu'
    med = open(os.path.join(ROOT, 'r-super_amd', 'config', 'abdomenatlas_ufo', 'medformer_3d.yaml')).read()
    assert re.search(r"^aug_device: 'cpu'\nintensity_aug_device: 'cpu'", med, re.M)


def test_cpu_tensors_and_wrong_inputs_are_refused():
    from rsuper_amd.hip.lib import RSuperHipError
    plan = aug.make_intensity_plan(1, multiply=[1.1])
    with pytest.raises(RSuperHipError):
        aug.intensity_augment_batch(torch.zeros(1, 1, 4, 4, 4), plan)
    with pytest.raises(RSuperHipError):
        aug.intensity_augment_batch(torch.zeros(1, 1, 4, 4, 4))
    with pytest.raises(RSuperHipError):
        aug._intensity_augment(torch.zeros(1, 1, 4, 4, 4), [1], [1.1, 0, 0, 0, 0], [0], [0.0] * 11, [0])


@pytest.mark.parametrize('ctr,key,out', [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0), (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1))])
def test_philox_restatement_reproduces_the_known_answer_vectors(ctr, key, out):
    """Random123 kat_vectors, philox4x32 10 rounds: all zero, all ones, the digits of pi."""
    assert tuple(int(v[0]) for v in IR.philox4x32_10(ctr, key)) == out


def test_noise_field_is_a_function_of_seed_and_index():
    a, b = IR.noise_field(7, 1001), IR.noise_field(7, 4096)
    assert np.array_equal(a, b[:1001]) and not np.array_equal(a, IR.noise_field(8, 1001))
    big = IR.noise_field(12345, 1 << 16)
    assert abs(big.mean()) <= 5 / np.sqrt(big.size) and abs(big.std() - 1) <= 5 / np.sqrt(2 * big.size)
    assert np.abs(IR.noise_field(12345, 1 << 16, np.float32) - big).max() < 1e-3
