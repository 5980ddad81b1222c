"""Host side of the Models Genesis pre-training (baselines/model_genesis/utils.py, kernel csrc/genesis.hip): the numpy restatement of the device's
stages (tests/genesis_ref.py) against the reference's own pairs (tests/golden/genesis.npz, written by tests/golden/gen_golden_genesis.py), the
Bezier knots, the plan's draws, the device-style permutations, the C ABI's declarations, the training option and the loss's guard.  No GPU needed."""
import hashlib
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
import genesis_ref as GR  # noqa: E402
from rsuper_amd.baselines import model_genesis as mg  # noqa: E402

G = np.load(os.path.join(ROOT, 'tests', 'golden', 'genesis.npz'))
N_CASES = int(G['n_cases'])
NAMES = [str(n) for n in G['names']]
HDR = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()


def fixture_case(k):
    """Case k of the fixture as the keyword arguments of genesis_ref.apply / make_genesis_plan (one sample) -> (input, arguments, noise)."""
    img = G['input_%s' % str(G['shape_%d' % k])]
    kw = dict(flip=[bool(f) for f in G['flip_%d' % k]])
    if 'blocks_%d' % k in G:
        blocks = G['blocks_%d' % k].astype(np.int64)
        n = blocks[:, 3] * blocks[:, 4] * blocks[:, 5]
        kw['blocks'] = blocks
        kw['perms'] = np.split(G['perm_%d' % k].astype(np.int64), np.cumsum(n)[:-1])
    if 'control_%d' % k in G:
        c = G['control_%d' % k]
        kw['control'] = (tuple(c[0]), tuple(c[1]), bool(G['sort_both_%d' % k]))
    noise = None
    if 'paint_%d' % k in G:
        kw['paint'], kw['boxes'] = str(G['paint_%d' % k]), [tuple(int(v) for v in q) for q in G['boxes_%d' % k]]
        noise = G['noise_%d' % k]
    return img, kw, noise


def test_fixture_covers_every_transform_and_both_curve_branches():
    seen = set()
    for k in range(N_CASES):
        _, kw, _ = fixture_case(k)
        seen |= {'flip'} if any(kw['flip']) else set()
        seen |= {'shuffle'} if 'blocks' in kw else set()
        seen |= {'curve_both' if kw['control'][2] else 'curve_x'} if 'control' in kw else set()
        seen |= {kw['paint']} if 'paint' in kw else set()
        if len(kw) == 1 and not any(kw['flip']) and len(G['draws_%d' % k]) == 0:
            seen.add('nothing')
        if len(G['draws_%d' % k]) == 2 and not any(kw['flip']):
            seen.add('flip_twice')
    assert seen == {'nothing', 'flip', 'flip_twice', 'shuffle', 'curve_x', 'curve_both', 'in', 'out'}
    assert os.path.getsize(os.path.join(ROOT, 'tests', 'golden', 'genesis.npz')) < 1000 * 1000


@pytest.mark.parametrize('k', range(N_CASES), ids=NAMES)
def test_restatement_equals_the_reference_bit_for_bit(k):
    img, kw, noise = fixture_case(k)
    plan = mg.make_genesis_plan(1, img.shape, **{n: [v] for n, v in kw.items()})
    x, y = GR.apply_plan(img, plan, 0, noise)
    assert x.dtype == np.float32 and np.array_equal(x.view(np.uint32), G['x_%d' % k].view(np.uint32)), '%d voxels of x differ' % (x != G['x_%d' % k]).sum()
    assert np.array_equal(y.view(np.uint32), G['y_%d' % k].view(np.uint32))


@pytest.mark.parametrize('k', [k for k in range(N_CASES) if 'control_%d' % k in G])
def test_bezier_curve_equals_the_reference_knots_bit_for_bit(k):
    c = G['control_%d' % k]
    xv, yv = mg.bezier_curve([[0, 0], list(c[0]), list(c[1]), [1, 1]], nTimes=100000)
    assert xv.dtype == np.float64 and xv.shape == (100000,)
    assert hashlib.sha256(xv.tobytes() + yv.tobytes()).hexdigest() == str(G['knots_sha_%d' % k])
    assert np.array_equal(np.stack([xv[::1000], yv[::1000]]), G['knots_every_%d' % k])
    # the plan's knots are those np.interp takes: abscissae sorted, ordinates sorted on that branch only
    plan = mg.make_genesis_plan(1, (16, 16, 16), control=[(tuple(c[0]), tuple(c[1]), bool(G['sort_both_%d' % k]))])
    assert np.array_equal(plan.curve[0][0], np.sort(xv))
    assert np.array_equal(plan.curve[0][1], np.sort(yv) if G['sort_both_%d' % k] else yv)


def test_bernstein_basis_is_kept():
    from rsuper_amd.baselines.model_genesis import utils
    mg.bezier_curve([[0, 0], [0.3, 0.7], [0.6, 0.2], [1, 1]], nTimes=1000)
    basis = utils._BASIS[(4, 1000)]
    mg.bezier_curve([[0, 0], [0.1, 0.2], [0.3, 0.4], [1, 1]], nTimes=1000)
    assert utils._BASIS[(4, 1000)] is basis


@pytest.mark.parametrize('size', [(14, 16, 20), (32, 40, 96)])
def test_plan_draws_stay_inside_the_reference_ranges(size):
    sz = np.array(size)
    seen = set()
    for s in range(12):
        plan = mg.plan_genesis_pair(2, size, num_block=200, seed=s, host_permutations=(s % 2 == 0))
        for b in range(2):
            assert not plan.flip[b][2]                   # the reference never flips W
            if plan.blocks[b] is not None:
                blk = plan.blocks[b]
                assert blk.shape == (200, 6)
                assert (blk[:, 3:] >= 1).all() and (blk[:, 3:] <= np.maximum(sz // 10, 1)).all()
                assert (blk[:, :3] >= 0).all() and (blk[:, :3] + blk[:, 3:] <= sz).all()
                if plan.perms[b] is not None:
                    for p, q in zip(plan.perms[b], blk):
                        assert np.array_equal(np.sort(p), np.arange(q[3] * q[4] * q[5]))
            if plan.control[b] is not None:
                (x1, y1), (x2, y2), _ = plan.control[b]
                assert all(0.0 <= v < 1.0 for v in (x1, y1, x2, y2))
                xp, fp = plan.curve[b]
                assert len(xp) == 100000 and (np.diff(xp) >= 0).all() and xp[0] == 0.0 and fp.min() >= 0.0 and fp.max() <= 1.0
            boxes = np.array(plan.boxes[b]).reshape(-1, 6)
            if plan.paint[b] == 'in':
                assert len(boxes) <= 5
                assert (boxes[:, 3:] >= sz // 6).all() and (boxes[:, 3:] <= sz // 3).all()
            if plan.paint[b] == 'out':
                assert 1 <= len(boxes) <= 5
                assert (boxes[:, 3:] >= sz - 4 * sz // 7).all() and (boxes[:, 3:] <= sz - 3 * sz // 7).all()
            if plan.paint[b] is not None:                # the 3-voxel margin on both sides
                assert (boxes[:, :3] >= 3).all() and (boxes[:, :3] + boxes[:, 3:] <= sz - 3).all()
            seen |= set(plan.fired(b))
            assert 0 <= plan.seed[b] < 1 << 64
    assert seen >= {'flip_d', 'flip_h', 'shuffle', 'curve', 'inpaint', 'outpaint'}
    a, b = mg.plan_genesis_pair(1, size, num_block=50, seed=3), mg.plan_genesis_pair(1, size, num_block=50, seed=3)
    assert a.flags == b.flags and a.seed == b.seed and a.boxes == b.boxes


def test_plan_firing_rates():
    """Over n = 2000 samples every gate fires within 4 standard errors sqrt(p (1 - p) / n) of its rate; the flip gate is the first draw of the loop
    (at least one flip drawn), painting splits into in- and out-painting by inpaint_rate."""
    n = 2000
    rates = dict(flip_rate=0.4, local_rate=0.5, nonlinear_rate=0.9, paint_rate=0.9, inpaint_rate=0.2)
    hits = dict(local=0, nonlinear=0, paint=0, inpaint=0)
    np.random.seed(11)
    plan = mg.plan_genesis_pair(n, (14, 16, 20), num_block=1, n_knots=64, **rates)       # the global generator, as the training loop uses it
    for b in range(n):
        hits['local'] += plan.blocks[b] is not None
        hits['nonlinear'] += plan.curve[b] is not None
        hits['paint'] += plan.paint[b] is not None
        hits['inpaint'] += plan.paint[b] == 'in'
    within = lambda k, p, m: abs(k / m - p) <= 4 * np.sqrt(p * (1 - p) / m)
    assert within(hits['local'], 0.5, n) and within(hits['nonlinear'], 0.9, n) and within(hits['paint'], 0.9, n)
    assert within(hits['inpaint'], 0.2, hits['paint'])
    # a net flip of D needs an odd number of draws of that axis among up to three: P = sum over the number of flips drawn
    q = 0.4
    p_k = [1 - q, q * (1 - q), q * q * (1 - q), q ** 3]                      # 0, 1, 2, 3 flips drawn
    odd = [0.0, 1 / 3, 2 * (1 / 3) * (2 / 3), 3 * (1 / 3) * (2 / 3) ** 2 + (1 / 3) ** 3]
    p_d = sum(a * o for a, o in zip(p_k, odd))
    assert within(sum(plan.flip[b][0] for b in range(n)), p_d, n) and within(sum(plan.flip[b][1] for b in range(n)), p_d, n)


@pytest.mark.parametrize('size', [(10, 14, 14), (13, 20, 20), (20, 20, 12)])
def test_a_side_below_14_raises(size):
    with pytest.raises(ValueError, match='at least 14'):
        mg.plan_genesis_pair(1, size)
    with pytest.raises(ValueError, match='at least 14'):
        mg.make_genesis_plan(1, size)


def test_explicit_plans_are_checked():
    with pytest.raises(ValueError, match='inside the volume'):
        mg.make_genesis_plan(1, (16, 16, 16), blocks=[[[15, 0, 0, 2, 1, 1]]])
    with pytest.raises(ValueError, match='sides 1 .. 16'):
        mg.make_genesis_plan(1, (20, 20, 20), blocks=[[[0, 0, 0, 17, 1, 1]]])
    with pytest.raises(ValueError, match='permutation'):
        mg.make_genesis_plan(1, (16, 16, 16), blocks=[[[0, 0, 0, 2, 1, 1]]], perms=[[[0, 0]]])
    with pytest.raises(ValueError, match='painted boxes'):
        mg.make_genesis_plan(1, (16, 16, 16), paint=['in'], boxes=[[(3, 3, 3, 14, 2, 2)]])
    with pytest.raises(ValueError, match='every shuffling sample'):
        mg.make_genesis_plan(2, (16, 16, 16), blocks=[[[0, 0, 0, 2, 1, 1]]] * 2, perms=[[[1, 0]], None])


def test_device_style_permutations_are_permutations():
    sizes = [1, 2, 7, 64, 729, 4096, 3, 1]
    perms = GR.device_perms(0x0123456789ABCDEF, sizes)
    assert [len(p) for p in perms] == sizes
    for p, n in zip(perms, sizes):
        assert np.array_equal(np.sort(p), np.arange(n))
    assert not np.array_equal(perms[4], np.arange(729))
    # one block's permutation is a function of (seed, block index, size) alone
    again = GR.device_perms(0x0123456789ABCDEF, sizes[:5])
    assert all(np.array_equal(a, b) for a, b in zip(again, perms))
    other = GR.device_perms(0x0123456789ABCDEE, sizes)
    assert not np.array_equal(other[5], perms[5])


def test_paint_noise_is_uniform_and_differs_from_the_gaussian_stream():
    import intensity_ref as IR
    u = GR.paint_noise(7, 40000)
    assert u.dtype == np.float32 and u.min() > 0.0 and u.max() <= 1.0
    assert abs(u.mean() - 0.5) < 4 * np.sqrt(1 / 12 / 40000)
    r0 = IR.philox4x32_10([0, 0, 0, 0], [7, 0])[0]
    r1 = IR.philox4x32_10([0, 0, 1, 0], [7, 0])[0]
    assert r0 != r1


def test_abi_names_are_declared_and_bound():
    from rsuper_amd.hip import lib
    for name in ('rsuper_genesis_launches', 'rsuper_genesis_workspace_bytes', 'rsuper_genesis_pair', 'rsuper_mse_fwd', 'rsuper_mse_bwd',
                 'rsuper_mse_workspace_bytes'):
        assert re.search(r'\b%s\s*\(' % name, HDR), name
        assert name in lib.exported_symbols()
    for macro, value in (('RSUPER_GENESIS_MAX_BOXES', lib.GENESIS_MAX_BOXES), ('RSUPER_GENESIS_MAX_BLOCK_SIDE', lib.GENESIS_MAX_BLOCK_SIDE),
                         ('RSUPER_GENESIS_MAX_AXIS', lib.GENESIS_MAX_AXIS)):
        assert int(re.search(r'#define %s (\d+)' % macro, HDR).group(1)) == value
    assert lib.GENESIS_MAX_AXIS // 10 == lib.GENESIS_MAX_BLOCK_SIDE and (lib.GENESIS_MAX_AXIS + 1) // 10 > lib.GENESIS_MAX_BLOCK_SIDE


def test_parser_sets_one_class_without_deep_supervision():
    from rsuper_amd import train_ddp
    args = train_ddp.get_parser(['--model_genesis_pretrain'])
    assert args.classes == 1 and args.classes_number == 1 and args.aux_loss is False
    args = train_ddp.get_parser(['--model_genesis_pretrain', '--model', 'medformer'])
    assert args.classes == 1 and args.aux_loss is False
    assert train_ddp.get_parser([]).classes != 1
    with pytest.raises(ValueError, match='hip_graph'):
        train_ddp.get_parser(['--model_genesis_pretrain', '--hip_graph'])


def test_model_genesis_loss_rejects_deep_supervision():
    from rsuper_amd.training import losses_foundation as lf
    t = torch.zeros(1, 1, 4, 4, 4)
    for result in ([t, t], (t, t)):
        with pytest.raises(ValueError, match='deep supervision'):
            lf.model_genesis_loss(result, t)


def test_model_genesis_loss_refuses_a_segmentation_label():
    """An integer / boolean label never went through the pair (the reference keeps the label float in this mode): refused before any launch."""
    from rsuper_amd.training import losses_foundation as lf
    r = torch.zeros(1, 1, 4, 4, 4)
    for dtype in (torch.uint8, torch.int64, torch.bool):
        with pytest.raises(NotImplementedError, match='pretext target'):
            lf.model_genesis_loss(r, torch.zeros(1, 1, 4, 4, 4, dtype=dtype))
        with pytest.raises(NotImplementedError, match='pretext target'):
            lf.calculate_loss({'segmentation': r}, torch.zeros(1, 1, 4, 4, 4, dtype=dtype), None, None, None, None, None, None, ['model_genesis'],
                              model_genesis=True)


def test_cpu_tensors_raise():
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.training import losses_foundation as lf
    with pytest.raises(RSuperHipError):
        mg.generate_pair_batch(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(RSuperHipError):
        mg.generate_one_pair(torch.zeros(16, 16, 16))
    with pytest.raises(RSuperHipError):
        lf.mse_loss(torch.zeros(4), torch.zeros(4))
