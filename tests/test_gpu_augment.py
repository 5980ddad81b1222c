"""MI355X tests of the device spatial augmentation (training/augmentation.py, kernel csrc/augment.hip; every launch goes through the C ABI
rsuper_affine_crop) against the reference's outputs in tests/golden/augment.npz (tests/golden/gen_golden_augment.py) and, at the sizes the
fixture cannot hold, against torch's CPU affine_grid / grid_sample computed in the test.

The rules of every comparison (check_case):
  bytes  bit-identical to the expectation at every voxel outside the tie mask -- voxels whose float64 source coordinate lies within 2e-4 of a
         half-integer on some axis, where an f32 coordinate may round to either neighbour; inside the mask the byte must be the source byte of
         one of the candidate voxels (floor or ceil on the tied axes, rint on the others; 0 out of bounds).  The mask may hold 0.5 % of the voxels.
  image  max |kernel - float64 trilinear| <= 2 * e_ref, e_ref = the expectation's own (f32) maximum distance from the float64 value on that case;
         the factor 2 allows a different but equally valid f32 operation order.
"""
import argparse
import ctypes
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden_augment as GA  # noqa: E402
import synth  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
G = np.load(os.path.join(ROOT, 'tests', 'golden', 'augment.npz'))
IDENT = torch.tensor([[1., 0, 0, 0], [0, 1., 0, 0], [0, 0, 1., 0]])


def A():
    from rsuper_amd.training import augmentation
    return augmentation


def run(img, vols, theta, out_size, offsets=None):
    """One C ABI call on device copies; offsets default to the centre crop.  Returns CPU tensors."""
    B = img.shape[0]
    theta = torch.as_tensor(theta, dtype=torch.float32).reshape(-1, 3, 4).expand(B, 3, 4)
    if offsets is None:
        offsets = A().crop_offsets(img.shape[2:], out_size, 'center') * B
    out, outs = A()._affine_crop(img.to(DEV), [v.to(DEV) for v in vols], theta, out_size, offsets)
    torch.cuda.synchronize()
    return out.cpu(), [o.cpu() for o in outs]


def window(a, out_size, off):
    return a[..., off[0]:off[0] + out_size[0], off[1]:off[1] + out_size[1], off[2]:off[2] + out_size[2]]


def torch_cpu_expectation(img, vols, theta):
    """The ATen composition on the CPU for one sample: (f32 trilinear image, nearest byte volumes, float64 trilinear image), full grid."""
    t = torch.as_tensor(theta, dtype=torch.float32).reshape(1, 3, 4)
    grid = F.affine_grid(t, list(img.shape), align_corners=True)
    e_img = F.grid_sample(img, grid, mode='bilinear', padding_mode='zeros', align_corners=True)
    e_vols = [F.grid_sample(v.float(), grid, mode='nearest', padding_mode='zeros', align_corners=True).to(torch.uint8) for v in vols]
    return e_img, e_vols, GA.trilinear_f64(img, t)


def check_bytes(got, exp, src, coords, tie, what):
    """got, exp: (P, d, h, w) u8; src: (P, D, H, W) u8; coords: (3, d, h, w) f64 in x, y, z order; tie: (d, h, w) bool."""
    got, exp, src = (np.asarray(a) for a in (got, exp, src))
    bad = (got != exp).any(0)
    assert not (bad & ~tie).any(), '%s: %d voxels outside the tie mask differ' % (what, int((bad & ~tie).sum()))
    n = src.shape[1:][::-1]                                                   # W, H, D
    for z, y, x in zip(*np.nonzero(bad)):                                     # only tie voxels that differ need the candidate test
        s = coords[:, z, y, x]
        cands = [[]] * 3
        for ax in range(3):
            f = np.floor(s[ax])
            cands[ax] = [int(f), int(f) + 1] if abs(s[ax] - f - 0.5) < GA.TIE_BAND else [int(np.rint(s[ax]))]
        allowed = []
        for cx in cands[0]:
            for cy in cands[1]:
                for cz in cands[2]:
                    inb = 0 <= cx < n[0] and 0 <= cy < n[1] and 0 <= cz < n[2]
                    allowed.append(src[:, cz, cy, cx] if inb else np.zeros(src.shape[0], np.uint8))
        assert any(np.array_equal(got[:, z, y, x], a) for a in allowed), '%s: tie voxel %s holds none of its candidates' % (what, (z, y, x))
    return int(bad.sum())


def check_case(what, img, vols, theta, out_size, off, got_img, got_vols, exp_img, exp_vols, f64_img, e_ref=None):
    """One sample: img (1, Ci, D, H, W), vols / got_vols / exp_vols lists of (1, P, ...), exp_* and f64_img already cut to the crop."""
    coords = window(GA.source_coords(np.asarray(theta), img.shape[2:]), out_size, off)
    tie = GA.tie_mask(coords)
    frac = tie.mean()
    assert frac <= GA.TIE_MAX_FRACTION, '%s: %.3f %% of the voxels in the tie band' % (what, 100 * frac)
    diff = [check_bytes(g[0], e[0], v[0], coords, tie, what) for g, e, v in zip(got_vols, exp_vols, vols)]
    if e_ref is None:
        e_ref = float((exp_img.double() - f64_img).abs().max())
    err = float((got_img.double() - f64_img).abs().max())
    print('%s: tie band %.3f %%, differing tie voxels %s, image |kernel - f64| %.3g, e_ref %.3g' % (what, 100 * frac, diff, err, e_ref))
    assert err <= 2 * e_ref, '%s: image error %.3g exceeds 2 * e_ref = %.3g' % (what, err, 2 * e_ref)
    return err, e_ref


def fixture_case(k):
    from rsuper_amd.training.dataset import pack_bits
    seed, classes, kw, with_fg = GA.CASES[k]
    img, lab, fg = GA.case_inputs(seed, classes)
    vols = [torch.from_numpy(pack_bits(lab))] + ([fg.to(torch.uint8)[None, None]] if with_fg else [])
    exp = [torch.from_numpy(G['lab_%d' % k])] + ([torch.from_numpy(G['fg_%d' % k])] if with_fg else [])
    return img, lab, fg, vols, exp


# ------------------------------------------------------------------------------------------------------------------ the reference fixture
@pytest.mark.parametrize('k', range(len(GA.CASES)))
def test_fused_center_crop_matches_reference_fixture(k):
    img, lab, fg, vols, exp = fixture_case(k)
    theta = torch.from_numpy(G['theta_%d' % k])
    out, outs = A().affine_center_crop(img.to(DEV), tuple(v.to(DEV) for v in vols), theta.unsqueeze(0), GA.CROP)
    assert out.shape == (1, 1) + GA.CROP and out.dtype == torch.float32 and [o.dtype for o in outs] == [torch.uint8] * len(vols)
    off = A().crop_offsets(GA.SIZE, GA.CROP, 'center')
    f64 = GA.center(GA.trilinear_f64(img, theta))
    check_case('fixture case %d' % k, img, vols, theta, GA.CROP, off, out.cpu(), [o.cpu() for o in outs], torch.from_numpy(G['img_%d' % k]), exp, f64,
               e_ref=float(G['e_ref_%d' % k]))


@pytest.mark.parametrize('k,lab_dtype', [(0, torch.int64), (3, torch.uint8), (4, torch.int64), (5, torch.bool)])
def test_reference_signatures_on_device(k, lab_dtype):
    """random_scale_rotate_translate_3d + crop_3d as the reference calls them: same draws (seeded), same shapes and dtypes, fixture values."""
    from rsuper_amd.training.dataset import pack_bits
    seed, classes, kw, with_fg = GA.CASES[k]
    img, lab, fg, vols, exp = fixture_case(k)
    np.random.seed(seed)
    r = A().random_scale_rotate_translate_3d(img.to(DEV), lab.to(lab_dtype).to(DEV), foreground=fg.to(DEV) if with_fg else None, **kw)
    assert np.random.random() == float(G['next_%d' % k])
    assert len(r) == (3 if with_fg else 2) and r[0].shape == img.shape and r[1].shape == lab.shape and r[1].dtype == torch.int64
    ci, cl = A().crop_3d(r[0], r[1], list(GA.CROP), 'center')
    assert ci.device.type == torch.device(DEV).type and cl.dtype == torch.int64 and cl.shape == (1, classes) + GA.CROP
    got = [torch.from_numpy(pack_bits(cl.cpu()))]
    if with_fg:
        assert r[2].dtype == torch.bool and r[2].shape == fg.shape
        got.append(GA.center(r[2].cpu()).to(torch.uint8)[None, None])
    theta = torch.from_numpy(G['theta_%d' % k])
    off = A().crop_offsets(GA.SIZE, GA.CROP, 'center')
    check_case('signature case %d' % k, img, vols, theta, GA.CROP, off, ci.cpu(), got, torch.from_numpy(G['img_%d' % k]), exp,
               GA.center(GA.trilinear_f64(img, theta)), e_ref=float(G['e_ref_%d' % k]))


# ------------------------------------------------------------------------------------------------------------------ equivalences, bit-exact
def _three_volumes(seed, classes=26, size=GA.SIZE):
    from rsuper_amd.training.dataset import pack_bits
    img, lab, fg = GA.case_inputs(seed, classes, size)
    _, unk, _ = GA.case_inputs(seed + 50, classes, size)
    return img, lab, [torch.from_numpy(pack_bits(lab)), torch.from_numpy(pack_bits(unk)), fg.to(torch.uint8)[None, None]]


def test_fused_crop_equals_full_transform_then_center_slice():
    img, _, vols = _three_volumes(0)
    theta = G['theta_0']
    a, av = run(img, vols, theta, GA.CROP)
    f, fv = run(img, vols, theta, GA.SIZE)
    assert torch.equal(a, GA.center(f)) and all(torch.equal(x, GA.center(y)) for x, y in zip(av, fv))
    off = [3, 7, 5]                                                           # any other window of the full grid as well
    a, av = run(img, vols, theta, GA.CROP, off)
    assert torch.equal(a, window(f, GA.CROP, off)) and all(torch.equal(x, window(y, GA.CROP, off)) for x, y in zip(av, fv))


def test_batch_equals_single_calls_with_per_sample_theta_and_offset():
    B = 11                                                                    # more than one launch's worth of samples
    parts = [_three_volumes(s) for s in range(3)]
    img = torch.cat([parts[b % 3][0] for b in range(B)])
    vols = [torch.cat([parts[b % 3][2][k] for b in range(B)]) for k in range(3)]
    theta = torch.stack([torch.from_numpy(G['theta_%d' % (b % 5)]) for b in range(B)])
    offs = [[b % 4, 2 * b % 9, 3 * b % 7] for b in range(B)]
    out, outs = A()._affine_crop(img.to(DEV), [v.to(DEV) for v in vols], theta, GA.CROP, sum(offs, []))
    for b in range(B):
        o1, v1 = run(img[b:b + 1], [v[b:b + 1] for v in vols], theta[b], GA.CROP, offs[b])
        assert torch.equal(out[b:b + 1].cpu(), o1) and all(torch.equal(x[b:b + 1].cpu(), y) for x, y in zip(outs, v1)), b


def test_packed_volumes_equal_unpacked_planes_packed_afterwards():
    from rsuper_amd.training.dataset import pack_bits
    img, lab, vols = _three_volumes(1)
    _, pv = run(img, vols[:1], G['theta_1'], GA.CROP)
    _, uv = run(img, [lab], G['theta_1'], GA.CROP)                            # 26 plain u8 planes
    assert uv[0].shape == (1, 26) + GA.CROP and set(np.unique(uv[0].numpy())) <= {0, 1}
    assert np.array_equal(pack_bits(uv[0]), pv[0].numpy())


def test_three_volumes_in_one_launch_equal_separate_launches():
    img, _, vols = _three_volumes(2)
    out, outs = run(img, vols, G['theta_2'], GA.CROP)
    for k in range(3):
        o1, v1 = run(img, [vols[k]], G['theta_2'], GA.CROP)
        assert torch.equal(o1, out) and torch.equal(v1[0], outs[k])
    o0, v0 = run(img, [], G['theta_2'], GA.CROP)
    assert torch.equal(o0, out) and v0 == []


@pytest.mark.parametrize('size,crop,off', [(GA.SIZE, GA.CROP, [5, 1, 13]), ((37, 41, 29), (19, 23, 13), [18, 0, 7]), ((37, 41, 29), (37, 41, 29), [0, 0, 0])])
def test_identity_theta_is_an_exact_copy(size, crop, off):
    img, _, vols = _three_volumes(3, size=size)
    out, outs = run(img, vols, IDENT, crop, off)
    assert torch.equal(out, window(img, crop, off)) and all(torch.equal(o, window(v, crop, off)) for o, v in zip(outs, vols))


def test_random_plain_crop_of_spatial_augment_batch_is_a_copy_and_affine_branch_is_the_fused_crop():
    from rsuper_amd.training.dataset import PackedBits
    B = 6
    parts = [_three_volumes(s) for s in range(2)]
    img = torch.cat([parts[b % 2][0] for b in range(B)]).to(DEV)
    packed = [torch.cat([parts[b % 2][2][k] for b in range(B)]).to(DEV) for k in range(2)]
    vols = (PackedBits(packed[0], 26), PackedBits(packed[1], 26))
    np.random.seed(GA.SEQ_SEED)
    theta, offs, branch = A().plan_spatial_augment(B, GA.SIZE, GA.CROP, **GA.SEQ_ARGS)
    assert any(branch) and not all(branch)
    np.random.seed(GA.SEQ_SEED)
    out, outs = A().spatial_augment_batch(img, vols, list(GA.CROP), **GA.SEQ_ARGS)
    assert all(isinstance(o, PackedBits) and o.C == 26 and o.packed.shape == (B, 4) + GA.CROP for o in outs) and out.shape == (B, 1) + GA.CROP
    for b in range(B):
        off = offs[3 * b:3 * b + 3]
        if branch[b]:
            e, ev = A().affine_center_crop(img[b:b + 1], tuple(PackedBits(p[b:b + 1], 26) for p in packed), theta[b:b + 1], GA.CROP)
            assert torch.equal(out[b:b + 1], e) and all(torch.equal(o.packed[b:b + 1], x.packed) for o, x in zip(outs, ev))
        else:
            assert torch.equal(out[b:b + 1], window(img[b:b + 1], GA.CROP, off))
            assert all(torch.equal(o.packed[b:b + 1], window(p[b:b + 1], GA.CROP, off)) for o, p in zip(outs, packed))


def test_dispatcher_op_is_registered_and_refuses_cpu_tensors():
    from rsuper_amd.hip.lib import RSuperHipError
    img, _, vols = _three_volumes(0)
    out, outs = A().affine_center_crop(img.to(DEV), (vols[0].to(DEV),), IDENT.unsqueeze(0), GA.CROP)
    o2, v2 = torch.ops.rsuper.affine_crop(img.to(DEV), [vols[0].to(DEV)], IDENT.unsqueeze(0), list(GA.CROP), A().crop_offsets(GA.SIZE, GA.CROP, 'center'))
    assert torch.equal(out, o2) and torch.equal(outs[0], v2[0])
    with pytest.raises(RSuperHipError):
        A().affine_center_crop(img, (vols[0],), IDENT.unsqueeze(0), GA.CROP)
    with pytest.raises((RuntimeError, NotImplementedError)):
        torch.ops.rsuper.affine_crop(img, [vols[0]], IDENT.unsqueeze(0), list(GA.CROP), [0, 0, 0])


# ------------------------------------------------------------------------------------------------------------------ edges
@pytest.mark.parametrize('size,crop,off,planes', [((37, 41, 29), (19, 23, 13), None, 4), ((37, 41, 29), (37, 41, 29), None, 1),
                                                  ((23, 30, 34), (20, 17, 32), [3, 13, 2], 4), ((40, 48, 44), (21, 28, 24), [0, 20, 20], 1)])
@pytest.mark.parametrize('k', [0, 2])
def test_odd_and_ragged_sizes_against_torch_cpu(size, crop, off, planes, k):
    from rsuper_amd.training.dataset import pack_bits
    img, lab, _ = GA.case_inputs(10 + k, 26 if planes == 4 else 3, size)
    vols = [torch.from_numpy(pack_bits(lab))] if planes == 4 else [lab[:, :1].contiguous()]
    assert vols[0].shape[1] == planes
    theta = G['theta_%d' % k]
    off = off or A().crop_offsets(size, crop, 'center')
    out, outs = run(img, vols, theta, crop, off)
    e_img, e_vols, f64 = torch_cpu_expectation(img, vols, theta)
    check_case('ragged %s -> %s' % (size, crop), img, vols, theta, crop, off, out, outs, window(e_img, crop, off), [window(v, crop, off) for v in e_vols],
               window(f64, crop, off))


def test_theta_that_leaves_the_volume_gives_zeros():
    img, _, vols = _three_volumes(4)
    for theta in ([[1., 0, 0, 5.], [0, 1., 0, 0], [0, 0, 1., 0]], [[1., 0, 0, 0], [0, 1., 0, -3.5], [0, 0, 1., 0]], [[1e30, 0, 0, 1e30], [0, 1., 0, 0], [0, 0, 1., 0]],
                  [[float('nan')] * 4, [0, 1., 0, 0], [0, 0, 1., 0]]):
        out, outs = run(img, vols, torch.tensor(theta), GA.CROP)
        assert not out.any() and not any(o.any() for o in outs), theta
    # half out: the in-bounds side is untouched by the guard (a shift by exactly 10 voxels along x)
    shift = torch.tensor([[1., 0, 0, 20.0 / (GA.SIZE[2] - 1)], [0, 1., 0, 0], [0, 0, 1., 0]])
    out, outs = run(img, vols, shift, GA.SIZE)
    e_img, e_vols, f64 = torch_cpu_expectation(img, vols, shift)
    check_case('shift', img, vols, shift, GA.SIZE, [0, 0, 0], out, outs, e_img, e_vols, f64)
    assert not out[..., -9:].any() and not any(o[..., -9:].any() for o in outs)


def test_rejected_arguments_return_an_error_code():
    from rsuper_amd.hip import lib
    L = lib.lib()
    D, H, W, d, h, w = 8, 9, 10, 4, 5, 6
    img = torch.full((1, 1, D, H, W), 3.0, device=DEV)
    vol = torch.ones((1, 2, D, H, W), device=DEV, dtype=torch.uint8)
    out = torch.full((1, 1, d, h, w), 7.0, device=DEV)
    vout = torch.full((1, 2, d, h, w), 7, device=DEV, dtype=torch.uint8)
    theta = IDENT.unsqueeze(0).to(DEV).contiguous()
    st = torch.cuda.current_stream().cuda_stream

    def call(theta_p=theta.data_ptr(), img_p=img.data_ptr(), out_p=out.data_ptr(), B=1, Ci=1, dims=(D, H, W), nvol=1, src=vol.data_ptr(), dst=vout.data_ptr(),
             planes=2, crop=(d, h, w), off=(0, 0, 0), arrays=True):
        s, t, p = (ctypes.c_void_p * 1)(src), (ctypes.c_void_p * 1)(dst), (ctypes.c_int * 1)(planes)
        o = (ctypes.c_int * 3)(*off)
        return L.rsuper_affine_crop(theta_p, img_p, out_p, B, Ci, *dims, nvol, s if arrays else None, t if arrays else None, p if arrays else None, *crop, o, st)

    ARG = 1
    assert call() == 0
    torch.cuda.synchronize()
    assert bool((out == 3).all()) and bool((vout == 1).all())
    out.fill_(7.0); vout.fill_(7)
    bad = [dict(dims=(1, H, W), crop=(1, h, w)), dict(dims=(D, 1, W), crop=(d, 1, w)), dict(dims=(D, H, 1), crop=(d, h, 1)),      # N == 1 on an axis
           dict(crop=(D + 1, h, w)), dict(off=(D - d + 1, 0, 0)), dict(off=(0, H - h + 1, 0)), dict(off=(0, 0, W - w + 1)), dict(off=(-1, 0, 0)),
           dict(crop=(0, h, w)),
           dict(planes=lib_max_planes() + 1), dict(planes=0), dict(nvol=4), dict(nvol=-1), dict(B=0), dict(Ci=0),
           dict(theta_p=None), dict(img_p=None), dict(out_p=None), dict(src=None), dict(dst=None), dict(arrays=False)]
    for kw in bad:
        assert call(**kw) == ARG, kw
    assert L.rsuper_affine_crop(theta.data_ptr(), img.data_ptr(), out.data_ptr(), 1, 1, D, H, W, 0, None, None, None, d, h, w, None, st) == ARG   # no offsets
    torch.cuda.synchronize()
    assert bool((out == 7).all()) and bool((vout == 7).all()), 'a rejected call must not launch'
    assert call(planes=2, nvol=0, arrays=False) == 0                          # no byte volume at all is a valid call


def lib_max_planes():
    import re
    hdr = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    return int(re.search(r'#define\s+RSUPER_AFFINE_MAX_PLANES\s+(\d+)', hdr).group(1))


def test_maximum_plane_count_runs():
    P = lib_max_planes()
    rs = np.random.RandomState(0)
    img = torch.from_numpy(rs.standard_normal((1, 2, 9, 10, 12)).astype(np.float32))        # two image channels as well
    vol = torch.from_numpy(rs.randint(0, 256, (1, P, 9, 10, 12)).astype(np.uint8))
    out, outs = run(img, [vol], IDENT, (9, 10, 12))
    assert torch.equal(out, img) and torch.equal(outs[0], vol)
    theta = G['theta_2']
    out, outs = run(img, [vol], theta, (9, 10, 12))
    e_img, e_vols, f64 = torch_cpu_expectation(img, [vol], theta)
    check_case('P = %d' % P, img, [vol], theta, (9, 10, 12), [0, 0, 0], out, outs, e_img, e_vols, f64)


# ------------------------------------------------------------------------------------------------------------------ full size
def _fullsize_inputs(seed, size, classes=26):
    """White-noise image; labels built at a quarter of the resolution and repeated (cheap on the host, still blob-shaped)."""
    from rsuper_amd.training.dataset import pack_bits
    small = tuple((s + 3) // 4 for s in size)
    rs = np.random.RandomState(seed)
    img = torch.from_numpy(rs.standard_normal((1, 1) + tuple(size)).astype(np.float32))
    vols = []
    for j in range(2):
        _, lab, _ = GA.case_inputs(seed + 100 * j, classes, small)
        big = lab.numpy().repeat(4, 2).repeat(4, 3).repeat(4, 4)[:, :, :size[0], :size[1], :size[2]]
        vols.append(torch.from_numpy(pack_bits(big)))
    return img, vols


@pytest.mark.parametrize('size,crop,kw', [((116, 136, 136), (96, 96, 96), dict(scale=0.3, rotate=45, translate=0.1)),
                                          ((148, 168, 168), (128, 128, 128), dict(scale=0, rotate=30, translate=0))])
def test_full_size_against_torch_cpu(size, crop, kw):
    B = 2
    np.random.seed(size[0])
    theta = torch.stack([A().draw_affine_3d(**kw) for _ in range(B)])
    parts = [_fullsize_inputs(b, size) for b in range(B)]
    img = torch.cat([p[0] for p in parts])
    vols = [torch.cat([p[1][k] for p in parts]) for k in range(2)]
    out, outs = A().affine_center_crop(img.to(DEV), tuple(v.to(DEV) for v in vols), theta, crop)
    out, outs = out.cpu(), [o.cpu() for o in outs]
    off = A().crop_offsets(size, crop, 'center')
    for b in range(B):
        e_img, e_vols, f64 = torch_cpu_expectation(img[b:b + 1], [v[b:b + 1] for v in vols], theta[b])
        check_case('full size %s sample %d' % (size, b), img[b:b + 1], [v[b:b + 1] for v in vols], theta[b], crop, off, out[b:b + 1],
                   [o[b:b + 1] for o in outs], window(e_img, crop, off), [window(v, crop, off) for v in e_vols], window(f64, crop, off))


# ------------------------------------------------------------------------------------------------------------------ downstream
def test_augmented_packed_batch_gives_the_loss_of_the_unpacked_crops():
    """spatial_augment_batch's PackedBits outputs go into calculate_loss unchanged and give the loss of the same crops as uint8 volumes."""
    from rsuper_amd.training import losses_foundation as lf
    from rsuper_amd.training.dataset import PackedBits, pack_bits
    classes = synth.TINY_CLASSES
    B, S, T = 2, 40, 32
    bt = synth.batch(B, S, classes, ['mask', 'report'], seed=11)
    img = torch.from_numpy(synth.image(B, S, seed=2)).to(DEV)
    packed = tuple(PackedBits(torch.from_numpy(pack_bits(bt[k])).to(DEV), len(classes)) for k in ('label', 'unk_channels', 'mask'))
    np.random.seed(1)
    _, _, branch = A().plan_spatial_augment(B, (S,) * 3, (T,) * 3, 0.3, 45, 0.1)
    assert branch == [False, True]                                             # one sample of each kind
    np.random.seed(1)
    crop, (lab, unk, msk) = A().spatial_augment_batch(img, packed, T, 0.3, 45, 0.1)
    assert crop.shape == (B, 1, T, T, T) and all(isinstance(v, PackedBits) and tuple(v.shape) == (B, len(classes), T, T, T) for v in (lab, unk, msk))
    la = argparse.Namespace(loss='ball_dice_last', aux_weight=[0.5, 0.5], seg_loss=1.0, report_volume_loss_basic=0.1, volume_loss_tolerance=0.2,
                            ball_bce_weight=1.0, ball_dice_weight=1.0, ball_volume_margin=0.2, multi_ch_tumor=False, stardard_ce_ball=False,
                            classification_branch=False)
    logits = torch.from_numpy(synth.logits(B, len(classes), T, seed=5)).to(DEV)
    vol, dia = torch.from_numpy(bt['volumes']).to(DEV), torch.from_numpy(bt['diameters']).to(DEV)

    def loss(lab, unk, msk):
        x = logits.clone().requires_grad_(True)
        r = lf.calculate_loss({'segmentation': x}, lab, unk, la, None, msk, vol, dia, classes)
        r['overall'].backward()
        return {k: float(v) for k, v in r.items()}, x.grad
    plain = [PackedBits(v.packed.clone(), v.C).unpack() for v in (lab, unk, msk)]
    ra, ga = loss(*plain)
    rb, gb = loss(lab, unk, msk)
    assert all(np.isfinite(v) for v in rb.values()) and ra == rb, (ra, rb)
    assert torch.equal(ga, gb)


def test_training_with_aug_device_gpu_on_the_synthetic_dataset(tmp_path):
    from rsuper_amd.train_ddp import get_parser, main_worker, source_size, SOURCE_MARGIN
    from rsuper_amd.training.dataset import SyntheticUFODataset
    classes = ['kidney_left', 'kidney_right', 'liver', 'pancreas', 'pancreatic_lesion']
    args = get_parser(['--epochs', '1', '--batch_size', '2', '--cp_path', str(tmp_path) + '/', '--unique_name', 'augdev', '--loss', 'ball_dice_last',
                       '--report_volume_loss_basic', '0.1', '--aug_device', 'gpu', '--crop_size', '32'])
    args.base_chan, args.iter_per_epoch, args.print_freq, args.compute_dtype = 8, 3, 100, 'f32'
    assert source_size(args) == [52, 72, 72]
    ds = SyntheticUFODataset(classes, size=32, length=8, seed=3, packed=True, margin=SOURCE_MARGIN)
    assert tuple(ds[0]['image'].shape) == (1, 52, 72, 72) and tuple(ds[1]['label'].shape) == (1, 52, 72, 72)
    np.random.seed(0); torch.manual_seed(0)
    hist = main_worker(0, 1, 0, args, trainset=ds)
    assert len(hist) == 1 and 'overall' in hist[0] and all(np.isfinite(v) for v in hist[0].values()), hist
    # the network saw training_size crops: a dataset without the packed volumes is refused
    with pytest.raises(ValueError):
        main_worker(0, 1, 0, args, trainset=SyntheticUFODataset(classes, size=32, length=8, seed=3, margin=SOURCE_MARGIN))
