"""Host side of the spatial augmentation (training/augmentation.py: draw_affine_3d, crop_3d, plan_spatial_augment) against the reference's
draws recorded in tests/golden/augment.npz (tests/golden/gen_golden_augment.py), and the C ABI's three declarations.  No GPU needed."""
import os
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden_augment as GA  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment.npz'))
CASES = list(range(len(GA.CASES)))


def test_fixture_is_the_one_the_generator_describes():
    assert int(G['n_cases']) == len(GA.CASES) and tuple(G['size']) == GA.SIZE and tuple(G['crop']) == GA.CROP
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'augment.npz')) < (1 << 20)
    n = int(np.prod(GA.CROP))
    for k in CASES:
        tie = np.unpackbits(G['tie_%d' % k])[:n]
        assert tie.mean() <= GA.TIE_MAX_FRACTION
        # the stored mask is the one the committed theta gives
        assert np.array_equal(tie.reshape(GA.CROP).astype(bool), GA.center(GA.tie_mask(GA.source_coords(G['theta_%d' % k], GA.SIZE))))


@pytest.mark.parametrize('k', CASES)
def test_draw_affine_3d_is_bit_identical_and_leaves_the_generator_where_the_reference_does(k):
    from rsuper_amd.training.augmentation import draw_affine_3d
    seed, _, kw, _ = GA.CASES[k]
    np.random.seed(seed)
    theta = draw_affine_3d(**kw)
    nxt = np.random.random()
    assert theta.dtype == torch.float32 and tuple(theta.shape) == (3, 4)
    assert np.array_equal(theta.numpy().view(np.uint32), G['theta_%d' % k].view(np.uint32))
    assert nxt == float(G['next_%d' % k])


def test_draw_affine_3d_defaults_are_the_reference_defaults():
    from rsuper_amd.training.augmentation import draw_affine_3d
    np.random.seed(GA.CASES[0][0])
    assert np.array_equal(draw_affine_3d().numpy(), G['theta_0'])


@pytest.mark.parametrize('seed', GA.CROP_SEEDS)
def test_crop_3d_random_offsets(seed):
    from rsuper_amd.training.augmentation import crop_3d, crop_offsets
    D, H, W = GA.SIZE
    idx = torch.arange(D * H * W, dtype=torch.float32).reshape(1, 1, D, H, W)
    z, y, x = (int(v) for v in G['crop_seed_%d' % seed])
    np.random.seed(seed)
    a, b = crop_3d(idx, idx.long(), list(GA.CROP), 'random')
    exp = idx[:, :, z:z + GA.CROP[0], y:y + GA.CROP[1], x:x + GA.CROP[2]]
    assert a.is_contiguous() and b.is_contiguous() and b.dtype == torch.int64
    assert torch.equal(a, exp) and torch.equal(b, exp.long())
    np.random.seed(seed)
    assert crop_offsets(GA.SIZE, GA.CROP, 'random') == [z, y, x]


def test_crop_3d_center_and_int_size():
    from rsuper_amd.training.augmentation import crop_3d, crop_offsets
    D, H, W = GA.SIZE
    idx = torch.arange(D * H * W, dtype=torch.float32).reshape(1, 1, D, H, W)
    assert crop_offsets(GA.SIZE, GA.CROP, 'center') == [int(v) for v in G['crop_center']]
    a, _ = crop_3d(idx, idx, list(GA.CROP), 'center')
    assert torch.equal(a, GA.center(idx))
    a, _ = crop_3d(idx, idx, 20, 'center')
    assert tuple(a.shape) == (1, 1, 20, 20, 20) and torch.equal(a, GA.center(idx, (20, 20, 20)))
    with pytest.raises(AssertionError):
        crop_3d(idx, idx, 20, 'corner')
    # a crop as large as the source: randint(0, max(0, 1)) is still drawn, as in the reference
    np.random.seed(3)
    st = np.random.RandomState(3)
    a, _ = crop_3d(idx, idx, list(GA.SIZE), 'random')
    for _ in range(3):
        st.randint(0, 1)
    assert torch.equal(a, idx) and np.random.random() == st.random_sample()


def test_spatial_augment_branch_sequence():
    from rsuper_amd.training.augmentation import plan_spatial_augment
    np.random.seed(GA.SEQ_SEED)
    theta, offs, branch = plan_spatial_augment(GA.SEQ_LEN, GA.SIZE, GA.CROP, **GA.SEQ_ARGS)
    nxt = np.random.random()
    assert [int(b) for b in branch] == [int(b) for b in G['branch_taken']]
    assert offs == [int(v) for v in G['branch_offsets'].reshape(-1)]
    assert theta.dtype == torch.float32 and np.array_equal(theta.numpy().view(np.uint32), G['branch_thetas'].view(np.uint32))
    assert nxt == float(G['branch_next'])


def test_cpu_tensors_are_refused():
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.training import augmentation as A
    img, lab, _ = GA.case_inputs(0, 3, (8, 9, 10))
    theta = torch.tensor(A.IDENTITY_THETA).unsqueeze(0)
    with pytest.raises(RSuperHipError):
        A.affine_center_crop(img, (lab,), theta, (4, 4, 4))
    with pytest.raises(RSuperHipError):
        A.random_scale_rotate_translate_3d(img, lab.long(), 0.3, 45, 0.1)
    with pytest.raises(RSuperHipError):
        A.spatial_augment_batch(img, (lab,), [4, 4, 4], 0.3, 45, 0.1)


def test_c_abi_is_declared_in_header_and_signatures():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    m = re.search(r'int\s+rsuper_affine_crop\s*\(([^;]*)\)\s*;', hdr)
    assert m, 'rsuper_affine_crop is not declared in include/rsuper_hip.h'
    assert 'rsuper_affine_crop' in lib._SIGS
    res, args = lib._SIGS['rsuper_affine_crop']
    assert len(args) == len(m.group(1).split(','))
    assert re.search(r'#define\s+RSUPER_AFFINE_MAX_PLANES\s+\d+', hdr) and re.search(r'#define\s+RSUPER_AFFINE_MAX_VOLUMES\s+3\b', hdr)


def test_aug_device_option_reaches_the_training_loop():
    from rsuper_amd import train_ddp
    args = train_ddp.get_parser(['--model', 'unet', '--dimension', '3d', '--dataset', 'abdomenatlas_ufo', '--aug_device', 'gpu', '--synthetic', '2'])
    assert args.aug_device == 'gpu'
    assert train_ddp.source_size(args) == [args.training_size[0] + 20, args.training_size[1] + 40, args.training_size[2] + 40]
    args.aug_device = 'cpu'
    assert train_ddp.source_size(args) == list(args.training_size)
