"""MI355X tests of the prediction post-processing and detection volumes (inference/detection.py, inference/postprocess.py; kernels in
csrc/postproc.hip) against scipy's literal forms (tests/golden/postprocess.npz, tests/golden/gen_golden_postprocess.py) and the numpy
restatement tests/postprocess_ref.py."""
import argparse
import os
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import postprocess_ref as R  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'postprocess.npz'))
DET = sorted({k[4:-2] for k in G.files if k.startswith('det_') and k.endswith('_x')})
CC = sorted({k[3:-5] for k in G.files if k.startswith('cc_') and k.endswith('_mask')})


def _cc_case(name):
    shape = tuple(int(v) for v in G[f'cc_{name}_shape'])
    n = int(np.prod(shape))
    return (np.unpackbits(G[f'cc_{name}_mask'])[:n].reshape(shape), np.unpackbits(G[f'cc_{name}_out'])[:n].reshape(shape))


def _smooth(shape, seed, coarse=8):
    """CT-like smooth probability volume: a coarse random grid resampled to `shape` (float32)."""
    r = np.random.default_rng(seed)
    c = r.standard_normal(tuple(max(2, s // coarse) for s in shape))
    v = R.zoom(c, [s / n for s, n in zip(shape, c.shape)])[:shape[0], :shape[1], :shape[2]]
    assert v.shape == tuple(shape)
    v = (v - v.mean()) / v.std()
    return (1.0 / (1.0 + np.exp(-2.0 * v))).astype(np.float32)


@pytest.mark.parametrize('erode', [True, False])
@pytest.mark.parametrize('name', DET)
def test_detection_matches_scipy_fixture(name, erode):
    from rsuper_amd.inference import detection
    x = G[f'det_{name}_x']
    sp = tuple(float(v) for v in G[f'det_{name}_spacing'])
    vols, m = detection(x, spacing=sp, erode=erode)
    exp = [int(v) for v in G[f'det_{name}_vol_' + ('erode' if erode else 'plain')]]
    assert list(vols) == list(R.THRESHOLDS)
    assert [vols[t] for t in R.THRESHOLDS] == exp
    assert all(type(v) is int for v in vols.values()) and type(m) is float
    e = float(G[f'det_{name}_max'])
    assert abs(m - e) <= 1e-12 * abs(e)


def test_detection_planes_in_one_launch_and_threshold_order():
    """(P, D, H, W) input: one launch, per-plane results equal to single calls; unsorted / duplicate thresholds map back to their keys."""
    from rsuper_amd.inference import detection
    xs = np.stack([_smooth((21, 30, 26), s) for s in (1, 2, 3)])
    ths = (0.7, 0.1, 0.5, 0.5, 0.3)
    many = detection(torch.from_numpy(xs).to(DEV), spacing=(1.3, 0.8, 0.75), thresholds=ths)
    for p in range(3):
        one = detection(xs[p], spacing=(1.3, 0.8, 0.75), thresholds=ths)
        assert many[p] == one
        rv, rm = R.detection(xs[p], (1.3, 0.8, 0.75), ths)
        assert one[0] == rv and abs(one[1] - rm) <= 1e-12 * abs(rm)


def test_detection_ct_sized_matches_numpy():
    """A CT-sized case (160 x 256 x 256 at 2.5 x 0.8 x 0.8 mm -> 400 x 205 x 205 after resampling) against the numpy restatement."""
    from rsuper_amd.inference import detection
    x = _smooth((160, 256, 256), 7, coarse=16)
    sp = (2.5, 0.8, 0.8)
    for erode in (True, False):
        vols, m = detection(x, spacing=sp, erode=erode)
        rv, rm = R.detection(x, sp, erode=erode)
        assert vols == rv
        assert abs(m - rm) <= 1e-12 * abs(rm)


def test_detection_workspace_contents_and_repeat():
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import detection
    x = torch.from_numpy(_smooth((33, 40, 37), 11)).to(DEV)
    base = detection(x, spacing=(1.5, 0.7, 0.9))
    nbytes = lib.lib().rsuper_detection_workspace_bytes(1)
    ws = torch.full((nbytes,), 0xFF, dtype=torch.uint8, device=DEV)
    assert detection(x, spacing=(1.5, 0.7, 0.9), workspace=ws) == base
    ws.view(torch.float32).fill_(float('nan'))
    assert detection(x, spacing=(1.5, 0.7, 0.9), workspace=ws) == base
    assert detection(x, spacing=(1.5, 0.7, 0.9), workspace=ws) == base


@pytest.mark.parametrize('dt', ['u8', 'f32'])
@pytest.mark.parametrize('lname', ['tiny', 'm42'])
def test_organ_masking_matches_scipy_fixture(lname, dt):
    from rsuper_amd.inference import postprocess_npz
    classes = synth.TINY_CLASSES if lname == 'tiny' else synth.MASK42_CLASSES
    pred = G[f'om_{lname}_{dt}']
    out = postprocess_npz(torch.from_numpy(pred).to(DEV)[None], classes, argparse.Namespace(organ_mask_on_lesion=True, connected_components=False))
    assert list(out) == [c for c in classes if 'lesion' not in c] + [c for c in classes if 'lesion' in c]
    les = np.stack([out[c].cpu().numpy() for c in classes if 'lesion' in c])
    exp = G[f'om_{lname}_{dt}_out']
    assert les.dtype == exp.dtype and np.array_equal(les.view(np.uint8), exp.view(np.uint8))
    for i, c in enumerate(classes):
        if 'lesion' not in c:
            assert np.array_equal(out[c].cpu().numpy(), pred[i])
    plain = postprocess_npz(torch.from_numpy(pred).to(DEV), classes, argparse.Namespace())
    for i, c in enumerate(classes):
        assert np.array_equal(plain[c].cpu().numpy(), pred[i])


@pytest.mark.parametrize('dt', [np.uint8, np.float32])
def test_postprocess_bone_copy_pairs_and_components(dt):
    """bone lesions keep their plane (all-ones organ), adrenal / lung pairs, uterus -> prostate, then the largest component."""
    from rsuper_amd.inference import postprocess_npz
    classes = ['adrenal_gland_left', 'adrenal_gland_right', 'adrenal_lesion', 'bone_lesion', 'lung_left', 'lung_lesion', 'lung_right',
               'prostate', 'uterus_lesion']
    r = np.random.default_rng(3)
    shape = (len(classes), 19, 23, 41)
    if dt == np.uint8:
        pred = (r.random(shape) < 0.35).astype(np.uint8)
    else:
        pred = (r.random(shape) * (r.random(shape) < 0.6)).astype(np.float32)
    for cc in (False, True):
        out = postprocess_npz(torch.from_numpy(pred).to(DEV), classes, argparse.Namespace(organ_mask_on_lesion=True, connected_components=cc))
        ref = R.postprocess(pred, classes, True, cc)
        for c in classes:
            got = out[c].cpu().numpy()
            assert got.dtype == ref[c].dtype and np.array_equal(got.view(np.uint8), ref[c].view(np.uint8)), c
    with pytest.raises(KeyError):         # bone_lesion without a prostate plane
        postprocess_npz(torch.from_numpy(pred[:7]).to(DEV), classes[:7], argparse.Namespace(organ_mask_on_lesion=True))


@pytest.mark.parametrize('name', CC)
def test_largest_component_matches_scipy_fixture(name):
    from rsuper_amd.inference import keep_largest_component
    m, exp = _cc_case(name)
    got = keep_largest_component(torch.from_numpy(m).to(DEV))
    assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), exp)
    prob = m.astype(np.float32) * np.random.default_rng(1).uniform(0.01, 1.0, m.shape).astype(np.float32)
    assert np.array_equal(keep_largest_component(torch.from_numpy(prob).to(DEV)).cpu().numpy(), exp)
    assert np.array_equal(keep_largest_component(torch.from_numpy(m).to(DEV).bool()).cpu().numpy(), exp)


def test_largest_component_percolating_512x512x96():
    """Density 0.31, near the face-connectivity percolation point: long snakes crossing many tiles."""
    from rsuper_amd.inference import keep_largest_component
    m = (np.random.default_rng(0).random((96, 512, 512)) < 0.31).astype(np.uint8)
    got = keep_largest_component(torch.from_numpy(m).to(DEV)).cpu().numpy()
    assert np.array_equal(got, R.largest_component(m))


def test_largest_component_root_beyond_2_24():
    """Linear indices above 2^24: the winning component starts past voxel 2^24; a size tie across that line goes to the earlier root."""
    from rsuper_amd.inference import keep_largest_component
    D, H, W = 300, 256, 256
    assert D * H * W > 1 << 24
    m = np.zeros((D, H, W), np.uint8)
    r = np.random.default_rng(5)
    m[280:300, 100:180, 30:230] = r.random((20, 80, 200)) < 0.45
    m[2:5, 3:9, 10:20] = 1
    got = keep_largest_component(torch.from_numpy(m).to(DEV)).cpu().numpy()
    ref = R.largest_component(m)
    assert np.flatnonzero(ref.ravel())[0] > (1 << 24)
    assert np.array_equal(got, ref)
    t = np.zeros((D, H, W), np.uint8)
    t[290:293, 3:9, 10:20] = 1
    t[2:5, 3:9, 10:20] = 1
    got = keep_largest_component(torch.from_numpy(t).to(DEV)).cpu().numpy()
    assert got.sum() == 180 and got[2:5, 3:9, 10:20].all()


def test_largest_component_workspace_contents_and_repeat():
    from rsuper_amd.inference import keep_largest_component
    from rsuper_amd.inference.postprocess import largest_component_workspace
    m, exp = _cc_case('d31')
    x = torch.from_numpy(m).to(DEV)
    ws = largest_component_workspace(m.shape, x.device)
    ws.fill_(0xFF)
    a = keep_largest_component(x, ws).cpu().numpy()
    ws.view(torch.float32).fill_(float('nan'))
    b = keep_largest_component(x, ws).cpu().numpy()
    c = keep_largest_component(x, ws).cpu().numpy()
    assert np.array_equal(a, exp) and np.array_equal(b, exp) and np.array_equal(c, exp)


def _nets(n):
    from oracle import unet_oracle as uo
    from rsuper_amd.model.dim3.unet import UNet
    classes = synth.TINY_CLASSES
    nets = []
    for seed in range(3, 3 + n):
        net = UNet(1, 8, num_classes=len(classes), block='BasicBlock', norm='in', compute_dtype='f32')
        sd = synth.fill_state_dict(uo.unet_param_shapes(1, 8, len(classes)), seed)
        net.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        nets.append(net.to(DEV))
    return nets


def test_prediction_two_model_ensemble_is_the_sum():
    from rsuper_amd.inference import inference_sliding_window, prediction
    nets = _nets(2)
    img = torch.from_numpy(synth.volume((40, 48, 36), 21)[0, 0])
    args = argparse.Namespace(window_size=[32, 32, 32], classes=len(synth.TINY_CLASSES))
    label, raw = prediction(nets, img, args)
    assert label.is_cuda and label.dtype == torch.uint8 and raw.dtype == torch.float32 and tuple(raw.shape) == (5, 40, 48, 36)
    total = torch.zeros((5, 40, 48, 36), device=DEV)
    for net in nets:
        total += inference_sliding_window(net, img[None, None], args, to_cpu=False).squeeze(0)
    assert torch.equal(raw, total)
    assert torch.equal(label, (total > 0.5).to(torch.uint8))
    lc, rc = prediction(nets, img, args, to_cpu=True)
    assert not rc.is_cuda and torch.equal(rc, total.cpu()) and torch.equal(lc, label.cpu())


def test_prediction_deep_case_in_independent_chunks():
    """D = 808 > 800: two 404-deep chunks, each inferred on its own."""
    from rsuper_amd.inference import inference_sliding_window, prediction
    nets = _nets(1)
    img = torch.from_numpy(synth.volume((808, 32, 32), 22)[0, 0])
    args = argparse.Namespace(window_size=[32, 32, 32], classes=len(synth.TINY_CLASSES))
    label, raw = prediction(nets, img, args)
    parts = [inference_sliding_window(nets[0], img[None, None, z0:z0 + 404], args, to_cpu=False).squeeze(0) for z0 in (0, 404)]
    exp = torch.cat(parts, dim=1)
    assert torch.equal(raw, exp)
    assert torch.equal(label, (exp > 0.5).to(torch.uint8))
    whole = inference_sliding_window(nets[0], img[None, None], args, to_cpu=False).squeeze(0)
    assert not torch.equal(raw, whole)           # windows across the chunk boundary would give other numbers


@pytest.mark.parametrize('pair', [((8, 8, 32), (7, 7, 31)), ((8, 7, 31), (7, 8, 32)), ((4, 8, 31), (4, 7, 32))])
def test_largest_component_ignores_a_diagonal_pair_across_a_tile_corner(pair):
    """6-connectivity at a corner of the 8 x 8 x 32 labelling tile: two voxels that touch only diagonally are two singletons, so the three-voxel
    run across the x = 31 | 32 tile face is the largest component."""
    from rsuper_amd.inference import keep_largest_component
    m = np.zeros((9, 9, 33), np.uint8)
    m[pair[0]] = m[pair[1]] = 1
    m[2, 2, 30:33] = 1
    want = np.zeros_like(m)
    want[2, 2, 30:33] = 1
    ref = R.largest_component(m)
    assert np.array_equal(ref, want)
    assert np.array_equal(keep_largest_component(torch.from_numpy(m).to(DEV)).cpu().numpy(), ref)
