"""MI355X tests of the Models Genesis pre-training path (baselines/model_genesis/utils.py generate_pair_batch, kernels csrc/genesis.hip through the C ABI
rsuper_genesis_pair / rsuper_mse_fwd / rsuper_mse_bwd; training/losses_foundation.py model_genesis_loss; train_ddp.py --model_genesis_pretrain).

The pair is exact: with the plan of a fixture case (tests/golden/genesis.npz, the reference's own generate_one_pair) x and y equal the reference's
bit for bit, and with device-drawn permutations and noise they equal the numpy restatement tests/genesis_ref.py (which tests/test_genesis_cpu.py
pins to the same fixture) bit for bit -- 0 differing voxels everywhere.

The MSE bound: with L64 = mean((r - y)^2) in float64 on the same operands and d_ref = |torch's CPU float32 mse_loss - L64|, the device value must
lie within 4 * d_ref + ulp32(L64) -- another order of the partial sums, plus the rounding any float32 result carries.  The gradient: every element
within 2 ulp32 of 2 (r - y) / N evaluated in float64.  Measured on MI355X: see DESIGN.md section 6l."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import genesis_ref as GR  # noqa: E402
from test_genesis_cpu import G, N_CASES, NAMES, fixture_case  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'


def MG():
    from rsuper_amd.baselines import model_genesis
    return model_genesis


def run(img, plan, noise=None):
    """img (B, D, H, W) numpy -> the device pair as numpy arrays of that shape."""
    t = torch.from_numpy(np.ascontiguousarray(img))[:, None].to(DEV)
    n = None if noise is None else torch.from_numpy(np.ascontiguousarray(noise))[:, None].to(DEV)
    x, y = MG().generate_pair_batch(t, plan, n)
    torch.cuda.synchronize()
    assert x.shape == t.shape and y.shape == t.shape and x.dtype == torch.float32
    return x[:, 0].cpu().numpy(), y[:, 0].cpu().numpy()


def same_bits(a, b):
    return int((np.ascontiguousarray(a).view(np.uint32) != np.ascontiguousarray(b).view(np.uint32)).sum())


def volume(shape, seed):
    rs = np.random.RandomState(seed)
    z = np.linspace(-1.0, 1.0, shape[0])[:, None, None]
    return (rs.standard_normal(shape) * 0.7 + 0.5 * z - 0.3).astype(np.float32)


def drawn_blocks(rs, shape, nb, max_side):
    sz = np.array(shape)
    n = rs.randint(1, np.minimum(max_side, sz) + 1, size=(nb, 3))
    return np.concatenate([rs.randint(0, sz - n + 1), n], axis=1)


# shape, blocks, largest block side: the reference's side // 10 except where larger boxes are to take the ranking loop's other paths
# (more voxels than threads; the largest box the kernel accepts, 16 x 16 x 16 = all of its LDS keys)
DEVICE_CASES = {
    'small_with_full_boxes': ((16, 20, 24), 300, 16),
    'odd_rows': ((17, 19, 23), 3000, 2),
    'sides_to_4': ((40, 36, 44), 6000, 4),
    'full_size': ((96, 96, 96), 10000, 9),
}


@functools.lru_cache(maxsize=None)
def device_case(name):
    """-> (img, plan, the restatement's x and y): everything fired, permutations and noise left to the device's generator."""
    shape, nb, side = DEVICE_CASES[name]
    rs = np.random.RandomState(len(name) + shape[0])
    img = volume(shape, shape[2])
    sz = np.array(shape)
    boxes = []
    for _ in range(3):
        n = sz - rs.randint(3 * sz // 7, 4 * sz // 7 + 1)
        boxes.append(tuple(int(v) for v in np.concatenate([rs.randint(3, sz - n - 3 + 1), n])))
    plan = MG().make_genesis_plan(1, shape, flip=[(True, name != 'odd_rows', name == 'odd_rows')], blocks=[drawn_blocks(rs, shape, nb, side)],
                                  control=[((rs.rand(), rs.rand()), (rs.rand(), rs.rand()), name == 'sides_to_4')],
                                  paint=['in' if name == 'sides_to_4' else 'out'], boxes=[boxes], seed=[0x9E3779B97F4A7C15 ^ nb])
    ref = GR.apply_plan(img, plan, 0)
    for a in (img,) + ref:
        a.setflags(write=False)
    return img, plan, ref


@pytest.mark.parametrize('k', range(N_CASES), ids=NAMES)
def test_fixture_plan_gives_the_reference_pair_bit_for_bit(k):
    img, kw, noise = fixture_case(k)
    plan = MG().make_genesis_plan(1, img.shape, **{n: [v] for n, v in kw.items()})
    x, y = run(img[None], plan, None if noise is None else noise[None])
    dx, dy = same_bits(x[0], G['x_%d' % k]), same_bits(y[0], G['y_%d' % k])
    print('case %s: %d voxels of x and %d of y differ from the reference' % (NAMES[k], dx, dy))
    assert dx == 0 and dy == 0


@pytest.mark.parametrize('name', list(DEVICE_CASES))
def test_device_drawn_permutations_and_noise_equal_the_restatement(name):
    img, plan, (rx, ry) = device_case(name)
    x, y = run(img[None], plan)
    dx, dy = same_bits(x[0], rx), same_bits(y[0], ry)
    print('%s: %d voxels of x and %d of y differ from genesis_ref' % (name, dx, dy))
    assert dx == 0 and dy == 0
    assert same_bits(x[0], y[0]) > x[0].size // 2       # the transforms did something


def test_batch_of_three_with_different_flags_equals_three_single_calls():
    shape = (17, 19, 23)
    rs = np.random.RandomState(5)
    imgs = np.stack([volume(shape, s) for s in (1, 2, 3)])
    blocks = drawn_blocks(rs, shape, 500, 2)
    cols = dict(flip=[(False, True, False), None, (True, False, True)], blocks=[None, blocks, None],
                control=[((0.2, 0.9), (0.7, 0.1), False), None, ((0.5, 0.1), (0.4, 0.8), True)],
                paint=['in', None, 'out'], boxes=[[(3, 4, 5, 4, 5, 6), (5, 5, 5, 3, 3, 3)], None, [(3, 3, 3, 9, 10, 12)]], seed=[11, 12, 13])
    plan = MG().make_genesis_plan(3, shape, **cols)
    assert len(set(plan.flags)) == 3 and MG().genesis_launches(plan) == 4
    x, y = run(imgs, plan)
    for b in range(3):
        one = MG().make_genesis_plan(1, shape, **{k: [v[b]] for k, v in cols.items()})
        xb, yb = run(imgs[b:b + 1], one)
        assert same_bits(x[b], xb[0]) == 0 and same_bits(y[b], yb[0]) == 0
        rx, ry = GR.apply_plan(imgs[b], plan, b)
        assert same_bits(x[b], rx) == 0 and same_bits(y[b], ry) == 0
    # a sample in which nothing fired leaves as (img - min) / span * span + min on both sides
    idle = MG().make_genesis_plan(1, shape)
    xi, yi = run(imgs[:1], idle)
    assert same_bits(xi, yi) == 0 and np.abs(xi - imgs[:1]).max() <= 4 * np.spacing(imgs[0].max() - imgs[0].min())


def test_two_runs_are_bit_identical():
    img, plan, (rx, _) = device_case('sides_to_4')
    a = run(img[None], plan)
    b = run(img[None], plan)
    assert same_bits(a[0], b[0]) == 0 and same_bits(a[1], b[1]) == 0 and same_bits(a[0][0], rx) == 0


def test_launch_counts_match_the_abi():
    from torch.profiler import ProfilerActivity, profile
    from rsuper_amd.baselines.model_genesis import utils
    shape = (16, 20, 24)
    rs = np.random.RandomState(9)
    img = torch.from_numpy(np.stack([volume(shape, s) for s in range(9)]))[:, None].to(DEV)
    blocks = drawn_blocks(rs, shape, 64, 2)
    plans = {
        'nothing': MG().make_genesis_plan(2, shape),
        'no_shuffle': MG().make_genesis_plan(2, shape, flip=[(True, False, False), None], control=[None, ((0.3, 0.6), (0.6, 0.2), True)],
                                             paint=['out', 'in'], boxes=[[(3, 3, 3, 8, 9, 10)], [(4, 4, 4, 3, 4, 5)]]),
        'one_shuffles': MG().make_genesis_plan(2, shape, blocks=[None, blocks]),
        'nine_samples': MG().make_genesis_plan(9, shape, blocks=[None] * 8 + [blocks]),
    }
    expect = {'nothing': 2, 'no_shuffle': 2, 'one_shuffles': 4, 'nine_samples': 2 + 4}
    for name, plan in plans.items():
        assert MG().genesis_launches(plan) == expect[name], name
        t = img[:plan.batch].contiguous()
        blk, perm, off, curve = utils._plan_tensors(plan, t.device)
        boxes = []
        for b in range(plan.batch):
            flat = [v for q in plan.boxes[b] for v in q]
            boxes += flat + [0] * (30 - len(flat))
        args = (t, plan.flags, blk, perm, off, curve, [len(q) for q in plan.boxes], boxes, plan.seed)
        utils._genesis_pair(*args)
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            utils._genesis_pair(*args)
            torch.cuda.synchronize()
        names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
        kernels = [n for n in names if 'genesis_' in n]
        print(name, kernels)
        assert len(kernels) == expect[name], (name, names)
        assert not any('memset' in n.lower() for n in names), names


def test_cpu_tensors_and_oversized_volumes_raise():
    from rsuper_amd.baselines.model_genesis import utils
    from rsuper_amd.hip.lib import RSuperHipError
    with pytest.raises(RSuperHipError):
        MG().generate_pair_batch(torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises(RSuperHipError):
        MG().generate_pair_batch(torch.zeros(1, 1, 16, 16, 16, device=DEV), noise=torch.zeros(1, 1, 16, 16, 16))
    with pytest.raises((RSuperHipError, NotImplementedError, RuntimeError)):
        MG().generate_pair_batch(torch.zeros(1, 1, 16, 16, 16, device=DEV))         # registers the op
        torch.ops.rsuper.genesis_pair(torch.zeros(1, 1, 16, 16, 16), [0], None, None, None, None, [0], [0] * 30, [0])
    wide = torch.zeros(1, 1, 14, 14, 180, device=DEV)
    with pytest.raises(RSuperHipError, match='RSUPER_ERR_ARG'):
        MG().generate_pair_batch(wide)
    with pytest.raises(RSuperHipError, match='RSUPER_ERR_ARG'):                       # the C ABI's own refusal
        utils._genesis_pair(wide, [0], None, None, None, None, [0], [0] * 30, [0])
    with pytest.raises(RSuperHipError, match='RSUPER_ERR_ARG'):                       # in- and out-painting together
        utils._genesis_pair(torch.zeros(1, 1, 16, 16, 16, device=DEV), [96], None, None, None, None, [0], [0] * 30, [0])
    with pytest.raises(RSuperHipError, match='RSUPER_ERR_ARG'):                       # a painted box outside the volume
        utils._genesis_pair(torch.zeros(1, 1, 16, 16, 16, device=DEV), [32], None, None, None, None, [1], [10, 0, 0, 7, 1, 1] + [0] * 24, [0])
    x, y = MG().generate_one_pair(torch.rand(20, 24, 28, device=DEV))
    assert x.shape == (20, 24, 28) and y.shape == (20, 24, 28)
    x, y = MG().generate_one_pair(torch.rand(2, 1, 14, 16, 18, device=DEV))
    assert x.shape == (2, 1, 14, 16, 18) and bool(torch.isfinite(x).all()) and bool(torch.isfinite(y).all())


@pytest.mark.parametrize('shape', [(2, 1, 16, 20, 24), (1, 1, 17, 19, 23)])
def test_mse_loss_value_and_gradient(shape):
    from rsuper_amd.training import losses_foundation as lf
    g = torch.Generator().manual_seed(shape[2])
    r, y = torch.randn(shape, generator=g) * 1.5, torch.randn(shape, generator=g)
    l64 = float(((r.double() - y.double()) ** 2).mean())
    d_ref = abs(float(torch.nn.functional.mse_loss(r, y)) - l64)
    bound = 4 * d_ref + float(np.spacing(np.float32(l64)))
    rd = r.to(DEV).requires_grad_(True)
    loss = lf.mse_loss(rd, y.to(DEV))
    assert loss.shape == () and loss.dtype == torch.float32
    loss.backward()
    torch.cuda.synchronize()
    d_dev = abs(float(loss.detach()) - l64)
    print('mse %s: float64 %.9g, torch CPU f32 off by %.3g, device off by %.3g, bound %.3g' % (shape, l64, d_ref, d_dev, bound))
    assert d_dev <= bound
    g64 = (2 * (r.double() - y.double()) / r.numel()).numpy()
    ulp = np.spacing(np.abs(g64).astype(np.float32)).astype(np.float64)
    err = np.abs(rd.grad.cpu().numpy().astype(np.float64) - g64) / ulp
    print('mse gradient %s: max error %.3f ulp' % (shape, err.max()))
    assert err.max() <= 2
    # the forward-only kernel (below autograd) gives the same bits; the label takes no gradient
    with torch.no_grad():
        assert float(lf.mse_loss(r.to(DEV), y.to(DEV))) == float(loss.detach())
    yd = y.to(DEV).requires_grad_(True)
    lf.mse_loss(r.to(DEV).requires_grad_(True), yd).backward()
    assert yd.grad is None


def test_calculate_loss_model_genesis_on_a_one_class_unet():
    from rsuper_amd.model.dim3.unet import UNet
    from rsuper_amd.training import losses_foundation as lf
    torch.manual_seed(0)
    net = UNet(1, 8, num_classes=1, compute_dtype='f32').to(DEV)
    img = torch.randn(1, 1, 32, 32, 32, device=DEV)
    x, y = MG().generate_pair_batch(img)
    out = net(x)
    loss = lf.calculate_loss(out, y, None, None, None, None, None, None, ['model_genesis'], model_genesis=True)
    assert set(loss) == {'genesis_loss', 'overall'} and loss['overall'] is loss['genesis_loss']
    loss['overall'].backward()
    torch.cuda.synchronize()
    ref = float(((out['segmentation'].detach().double() - y.double()) ** 2).mean())
    assert abs(float(loss['overall'].detach()) - ref) <= 1e-5 * ref
    gw = net.outc.weight.grad
    assert gw is not None and bool(torch.isfinite(gw).all()) and float(gw.abs().max()) > 0
    assert all(p.grad is not None and bool(torch.isfinite(p.grad).all()) for p in net.parameters())


def test_train_step_with_model_genesis_pretrain_changes_the_parameters(tmp_path):
    from unittest import mock
    from rsuper_amd import train_ddp
    from rsuper_amd.training.dataset import SyntheticUFODataset
    from rsuper_amd.training.utils import get_optimizer
    args = train_ddp.get_parser(['--model_genesis_pretrain', '--epochs', '1', '--batch_size', '2', '--cp_path', str(tmp_path) + '/',
                                 '--unique_name', 'genesis', '--intensity_aug_device', 'gpu', '--crop_size', '32'])
    args.base_chan, args.iter_per_epoch, args.print_freq, args.compute_dtype = 8, 2, 100, 'f32'
    np.random.seed(0); torch.manual_seed(0)
    net, ema = train_ddp.init_network(args, classes=['a', 'b', 'c'])
    assert net.outc.out_channels == 1
    opt = get_optimizer(args, net)
    before = [p.detach().clone() for p in net.parameters()]
    x, y = MG().generate_pair_batch(torch.randn(2, 1, 32, 32, 32, device=DEV))
    loss, _ = train_ddp.train_step(net, ema, opt, dict(image=x, label=y), args, ['model_genesis'], 0)
    torch.cuda.synchronize()
    assert set(loss) == {'genesis_loss', 'overall'} and np.isfinite(float(loss['overall']))
    assert any(not torch.equal(a, b.detach()) for a, b in zip(before, net.parameters()))
    # the epoch loop makes the pair from the loader's final image, whatever the dataset's class list
    classes = ['kidney_left', 'kidney_right', 'liver', 'pancreas', 'pancreatic_lesion']
    ds = SyntheticUFODataset(classes, size=32, length=6, seed=3)
    with mock.patch('rsuper_amd.baselines.model_genesis.generate_pair_batch', wraps=MG().generate_pair_batch) as spy:
        hist = train_ddp.main_worker(0, 1, 0, args, trainset=ds)
    assert spy.call_count >= 2 and all(tuple(c.args[0].shape) == (2, 1, 32, 32, 32) for c in spy.call_args_list)
    assert len(hist) == 1 and set(hist[0]) >= {'genesis_loss', 'overall'} and all(np.isfinite(v) for v in hist[0].values()), hist
    args.hip_graph = True
    with pytest.raises(ValueError, match='hip_graph'):
        train_ddp.train_epoch(None, net, ema, opt, 0, None, None, args)
