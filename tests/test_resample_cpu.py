"""CPU tests of the whole-CT preprocessing and the class-stack resampler: the numpy restatement (tests/resample_ref.py) against the reference's own
outputs in tests/golden/resample.npz, the host-side index logic, and the C ABI surface that needs no device."""
import argparse
import os
import re

import numpy as np
import pytest
import torch

import resample_ref as rr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_RS, N_NZ, N_PAD = 10, 5, 8
NEW_SYMBOLS = {'rsuper_ct_stats_workspace_bytes': 0, 'rsuper_ct_stats': 10, 'rsuper_ct_normalize': 18, 'rsuper_pad_box': 13,
               'rsuper_resample3d': 21}


@pytest.fixture(scope='module')
def g(golden):
    return golden['resample']


def exact_of(g, key):
    return g[key].astype(np.float64) + g[key + '_delta'].astype(np.float64)


@pytest.mark.parametrize('i', range(N_RS))
@pytest.mark.parametrize('dt', ['u8', 'f32'])
def test_restatement_reproduces_the_reference_resampling(g, i, dt):
    x, out = g[f'rs{i}_{dt}_x'], tuple(int(v) for v in g[f'rs{i}_out'])
    assert x.shape[1:] == tuple(g[f'rs{i}_in']) and 2 <= x.shape[0] <= 3
    near = rr.resample(x, out, 'nearest')
    assert near.dtype == x.dtype and np.array_equal(near, g[f'rs{i}_{dt}_nearest'])                      # bit-exact
    exact = rr.resample(x, out, 'trilinear', np.float64)
    idx = rr.sample_index(exact.size)
    bound = rr.trilinear_bound(x)
    assert np.abs(exact.reshape(-1)[idx] - exact_of(g, f'rs{i}_{dt}_tri')).max() <= 1e-12             # the recorded float64 evaluation itself
    assert np.abs(exact.reshape(-1)[idx] - g[f'rs{i}_{dt}_tri'].astype(np.float64)).max() <= bound    # the reference's float32 values
    np.testing.assert_allclose([exact.sum(), (exact * exact).sum(), np.abs(exact).max(), exact.size], g[f'rs{i}_{dt}_tri_sums'], rtol=1e-12)
    f32 = rr.resample(x, out, 'trilinear', np.float32)
    assert f32.dtype == np.float32 and np.abs(f32.astype(np.float64) - exact).max() <= bound          # the kernel's own order stays inside too
    thr = rr.THRESHOLD[dt]
    assert np.abs(exact - thr).min() > 1e-6
    assert np.array_equal(np.packbits((exact > thr).reshape(-1)), g[f'rs{i}_{dt}_thr'])
    assert np.array_equal(f32 > np.float32(thr), exact > thr)


def test_fixture_covers_the_cases_of_the_issue(g):
    cases = [((7, 9, 8), (11, 5, 13)), ((5, 6, 7), (5, 6, 7)), ((1, 4, 3), (3, 1, 7)), ((2, 2, 2), (1, 1, 1)), ((12, 20, 22), (30, 16, 18)),
             ((16, 17, 19), (7, 33, 10)), ((9, 1, 5), (4, 3, 2)), ((4, 4, 300), (4, 4, 77)), ((5, 3, 100), (5, 3, 333)), ((97, 5, 3), (291, 5, 3))]
    assert [(tuple(g[f'rs{i}_in']), tuple(g[f'rs{i}_out'])) for i in range(N_RS)] == cases
    assert all(int(v) % 2 == 1 for v in g['box_offset'])
    shapes = [(5, 7, 9), (1, 1, 2), (33, 65, 130), (40, 50, 60), (64, 128, 128)]
    assert [tuple(g[f'nz{i}_shape']) for i in range(N_NZ)] == shapes
    short = {tuple(int(n) < 16 for n in g[f'pad{i}_x'].shape) for i in range(N_PAD)}
    assert len(short) == 8                                                                            # every subset of short axes


def test_new_size_rounding_equals_the_reference(g):
    from rsuper_amd.inference.resample import new_size_from_spacing
    for row, out in zip(g['ns_in'], g['ns_out']):
        osp, osz, nsp = tuple(row[:3]), tuple(int(v) for v in row[3:6]), tuple(row[6:])
        assert rr.new_size(osp, osz, nsp) == out.tolist()
        assert new_size_from_spacing(osp, osz, nsp) == out.tolist()
    assert rr.new_size((1., 1., 1.), (5, 7, 9), (2., 2., 2.)) == [4, 4, 2]                            # 4.5, 3.5, 2.5: half to even


@pytest.mark.parametrize('i', range(N_NZ))
@pytest.mark.parametrize('dt', ['i16', 'f32'])
def test_restatement_reproduces_the_reference_zscore(g, i, dt):
    shape = tuple(int(v) for v in g[f'nz{i}_shape'])
    mean, sigma, seed = g[f'nz{i}_params']
    x = rr.ct_volume(shape, mean, sigma, int(seed), np.int16 if dt == 'i16' else np.float32)
    x64 = x.astype(np.float64)
    assert np.array_equal([x64.sum(), (x64 ** 2).sum()], g[f'nz{i}_{dt}_checksum'])                     # the same draw as the generator's
    assert x.min() < rr.CLIP[0] and x.max() > rr.CLIP[1]
    exact, m, s = rr.zscore(x)
    np.testing.assert_allclose([m, s], g[f'nz{i}_{dt}_stats'], rtol=1e-13)
    k = rr.sample_index(exact.size, 512, 512)
    assert np.abs(exact.reshape(-1)[k] - exact_of(g, f'nz{i}_{dt}_ref')).max() <= 1e-12 * max(1.0, np.abs(exact).max())
    assert np.abs(exact.reshape(-1)[k] - g[f'nz{i}_{dt}_ref'].astype(np.float64)).max() <= rr.zscore_bound(x, m, s)


def test_restatement_reproduces_the_reference_preprocess_with_padding(g):
    mean, sigma, seed = g['nz0_params']
    x = rr.ct_volume(tuple(int(v) for v in g['nz0_shape']), mean, sigma, int(seed), np.int16)
    exact, m, s = rr.zscore(x)
    padded, idx = rr.pad(exact, g['pp_training_size'].tolist())
    assert padded.shape == g['pp_out'].shape == (5, 9, 13) and idx == g['pp_idx'].tolist()                 # z is short: x widened (the quirk)
    assert np.abs(padded - g['pp_out'].astype(np.float64)).max() <= rr.zscore_bound(x, m, s)
    assert np.array_equal(padded == 0, g['pp_out'] == 0)


@pytest.mark.parametrize('i', range(N_PAD))
def test_pad_geometry_is_bit_exact(g, i):
    from rsuper_amd.inference.preprocess import _pad_geometry, unpad_img
    x, ts = g[f'pad{i}_x'], g['pad_training_size'].tolist()
    padded, idx = rr.pad(x, ts)
    assert padded.shape == g[f'pad{i}_out'].shape and np.array_equal(padded, g[f'pad{i}_out']) and idx == g[f'pad{i}_idx'].tolist()
    args = argparse.Namespace(dimension='3d', training_size=ts)
    shape, off, pidx = _pad_geometry(x.shape, args)
    assert shape == padded.shape and pidx == idx and off == rr.pad_geometry(x.shape, ts)[1]
    cut = unpad_img(torch.from_numpy(padded), idx, args)                                              # plain slicing: no device involved
    assert np.array_equal(cut.numpy(), g[f'pad{i}_unpad'])


def test_pad_quirk_example_and_dimension_errors():
    from rsuper_amd.inference.preprocess import _pad_geometry, unpad_img
    a = argparse.Namespace(dimension='3d', training_size=[96, 96, 96])
    shape, off, idx = _pad_geometry((10, 100, 120), a)
    assert shape == (10, 100, 208) and off == (0, 0, 44) and idx == [44, 54, 0, 100, 0, 120]
    with pytest.raises(NotImplementedError):
        _pad_geometry((4, 4, 4), argparse.Namespace(dimension='2d', training_size=[8, 8]))
    with pytest.raises(NotImplementedError):
        unpad_img(torch.zeros(2, 2, 2), [0, 1, 0, 1], argparse.Namespace(dimension='2d'))
    with pytest.raises(ValueError):
        _pad_geometry((4, 4, 4), argparse.Namespace(dimension='4d', training_size=[8, 8, 8]))


def test_symbols_are_declared_and_bound_with_matching_arity():
    from rsuper_amd.hip import lib
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    hdr = re.sub(r'/\*.*?\*/', '', hdr, flags=re.S)
    for name, arity in NEW_SYMBOLS.items():
        m = re.search(r'\b' + name + r'\s*\(([^)]*)\)\s*;', hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        params = [p for p in m.group(1).split(',') if p.strip() and p.strip() != 'void']
        assert len(params) == arity == len(lib._SIGS[name][1]), name
        assert hasattr(lib.lib(), name)


def test_argument_validation_without_a_device():
    """Everything here is rejected before a launch (the pointers are never dereferenced on the host)."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    ws_bytes = L.rsuper_ct_stats_workspace_bytes()
    assert ws_bytes > 0 and ws_bytes % 8 == 0
    x, out, ws = 4096, 8192, 16384                    # stand-ins for device addresses
    assert L.rsuper_ct_stats(None, 2, 4, 4, 4, -991., 500., ws, ws_bytes, None) == 1
    assert L.rsuper_ct_stats(x, 2, 4, 4, 4, -991., 500., None, ws_bytes, None) == 1
    assert L.rsuper_ct_stats(x, 2, 0, 4, 4, -991., 500., ws, ws_bytes, None) == 1
    assert L.rsuper_ct_stats(x, 0, 4, 4, 4, -991., 500., ws, ws_bytes, None) == 1                   # uint8 is no CT dtype
    assert L.rsuper_ct_stats(x, 2, 4, 4, 4, -991., 500., ws, ws_bytes - 1, None) == 1                # workspace too small
    assert L.rsuper_ct_stats(x, 2, 2048, 2048, 512, -991., 500., ws, ws_bytes, None) == 1            # 2^31 voxels
    ok = (x, 2, 4, 4, 4, -991., 500., ws, ws_bytes, out, 6, 6, 6, 1, 1, 1)
    for bad in [(None,) + ok[1:], ok[:9] + (None,) + ok[10:], ok[:7] + (None,) + ok[8:], ok[:8] + (8,) + ok[9:],
                ok[:10] + (6, 6, 4, 1, 1, 1), ok[:13] + (3, 1, 1), ok[:13] + (-1, 1, 1), ok[:2] + (4, -4, 4) + ok[5:]]:
        assert L.rsuper_ct_normalize(*bad, 32768, None) == 1
    assert L.rsuper_ct_normalize(*ok, None, None) == 1                                               # nowhere to store (mean, std)
    assert L.rsuper_pad_box(x, 1, 4, 4, 4, out, 4, 4, 3, 0, 0, 0, None) == 1
    assert L.rsuper_pad_box(x, 1, 4, 4, 4, x, 4, 4, 4, 0, 0, 0, None) == 1                           # in place
    rs = (x, 1, 2, 8, 8, 8, 1, 1, 1, 7, 7, 7, out, 1, 5, 5, 5, 1, 0, 0., None)
    for k, v in [(0, None), (12, None), (2, 0), (3, 0), (9, 0), (14, -5), (6, 2), (6, -1), (1, 2), (13, 7), (17, 2), (2, 70000)]:
        assert L.rsuper_resample3d(*(rs[:k] + (v,) + rs[k + 1:])) == 1, (k, v)
    assert L.rsuper_resample3d(*(rs[:18] + (1, 0.5, None))) == 1                                      # a threshold needs a uint8 output
    assert L.rsuper_resample3d(*(rs[:13] + (0,) + rs[14:])) == 3                                      # float32 -> uint8 without a threshold
    assert L.rsuper_resample3d(*(rs[:1] + (0,) + rs[2:13] + (0,) + rs[14:])) == 3                     # trilinear uint8 -> uint8 without one


def test_ops_are_registered_for_the_device_only():
    from rsuper_amd import inference  # noqa: F401  (import registers)
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.inference import normalize_ct, pad_to_training_size, resample_image_with_gpu
    for n in ('ct_normalize', 'resample3d'):
        assert getattr(torch.ops.rsuper, n).default._schema.name == f'rsuper::{n}'
        assert torch._C._dispatch_has_kernel_for_dispatch_key(f'rsuper::{n}', 'CUDA')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'rsuper::{n}', 'CPU')
        assert not torch._C._dispatch_has_kernel_for_dispatch_key(f'rsuper::{n}', 'AutogradCUDA')
    with pytest.raises(RSuperHipError):
        normalize_ct(torch.zeros(2, 3, 4))
    with pytest.raises(RSuperHipError):
        pad_to_training_size(torch.zeros(2, 3, 4), argparse.Namespace(dimension='3d', training_size=[4, 4, 4]))
    with pytest.raises(RSuperHipError):
        resample_image_with_gpu(torch.zeros(2, 3, 4), new_size=(4, 3, 2))
    with pytest.raises(NotImplementedError):
        resample_image_with_gpu(torch.zeros(2, 3, 4), new_size=(4, 3, 2), interp='bicubic')
    with pytest.raises(NotImplementedError):
        torch.ops.rsuper.resample3d(torch.zeros(1, 2, 3, 4), [0, 2, 0, 3, 0, 4], [2, 3, 4], 'nearest', None)
