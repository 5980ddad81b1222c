"""MI355X tests of training from whole CTs: rsuper_pack_bits against numpy, the chunked label upload, the samples of WholeVolumeLoader against the
reference's `__getitem__` (tests/golden/whole_ct.npz / .json from tests/golden/gen_golden_whole_ct.py, on the tree of tests/whole_ct_tree.py), the
producer's files against the reference's save(), prefetch on / off, train_ddp end to end and the two tools.

Bounds.  Everything is compared bit for bit, except a sample that took the resampling branch (crop, random affine, centre crop): there the rules of
tests/test_gpu_augment.py apply unchanged (its check_case is called): label bytes identical outside the tie mask (source coordinate within 2e-4 of a
half-integer) and one of the candidate source bytes inside it, the mask at most 0.5 % of the voxels; image max |kernel - float64 trilinear| <= 2 * e_ref,
e_ref = the reference's own distance from the float64 value on that sample (in the fixture)."""
import argparse
import ctypes
import json
import os
import random
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests'), os.path.join(ROOT, 'tests', 'golden')):
    if p not in sys.path:
        sys.path.insert(0, p)
import gen_golden_augment as GA  # noqa: E402
import whole_ct_tree as T  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = 'cuda'
with open(os.path.join(ROOT, 'tests', 'golden', 'whole_ct.json')) as f:
    G = json.load(f)
GZ = np.load(os.path.join(ROOT, 'tests', 'golden', 'whole_ct.npz'))


def D():
    from rsuper_amd.training import dataset
    return dataset


def W():
    from rsuper_amd.training.dataset import whole_ct
    return whole_ct


def L():
    from rsuper_amd.hip import lib
    return lib.lib()


def stream():
    return torch.cuda.current_stream().cuda_stream


def values(shape, dtype, seed):
    """Bytes with every kind of non-zero: 1, 2, 128 (-128 as int8), 255 (-1), and about half zeros."""
    rng = np.random.RandomState(seed)
    a = rng.choice(np.array([0, 0, 0, 0, 1, 2, 128, 255], np.uint8), size=shape)
    return (a != 0) if dtype == np.bool_ else a.view(dtype)


# ------------------------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize('C', [1, 7, 8, 9, 26, 42, 64])
def test_pack_bits_matches_numpy(C):
    for V in (1, 15, 16, 17, 255, 4099):
        for B in (1, 3):
            for k, dtype in enumerate((np.int8, np.uint8, np.bool_)):
                a = values((B, C, V), dtype, 100 * C + V + B + k)
                exp = np.stack([np.packbits(a[b].astype(bool), axis=0) for b in range(B)])
                got = D().pack_bits_device(torch.from_numpy(a).to(DEV).reshape(B, C, 1, 1, V))
                assert got.C == C and got.packed.dtype == torch.uint8 and tuple(got.packed.shape) == (B, (C + 7) // 8, 1, 1, V)
                assert np.array_equal(got.packed.cpu().numpy().reshape(exp.shape), exp), (C, V, B, dtype)
    # (C, D, H, W) without the batch axis, and the dispatcher op itself
    a = values((C, 3, 5, 7), np.int8, C)
    got = D().pack_bits_device(torch.from_numpy(a).to(DEV))
    assert np.array_equal(got.packed.cpu().numpy()[0], np.packbits(a.astype(bool), axis=0))
    assert torch.equal(torch.ops.rsuper.pack_bits(torch.from_numpy(a).to(DEV)[None]), got.packed)
    with pytest.raises(Exception):
        torch.ops.rsuper.pack_bits(torch.from_numpy(a)[None])              # no CPU kernel


@pytest.mark.parametrize('off', [1, 3])
def test_pack_bits_unaligned_source(off):
    for C, V in ((9, 4099), (26, 255), (8, 16)):
        a = values((C * V,), np.int8, C + off)
        buf = torch.zeros(C * V + 64, dtype=torch.int8, device=DEV)
        base = (-buf.data_ptr()) % 16 + off
        src = buf[base:base + C * V]
        src.copy_(torch.from_numpy(a))
        assert src.data_ptr() % 16 == off
        out = torch.full(((C + 7) // 8 * V,), 0xEE, dtype=torch.uint8, device=DEV)
        assert L().rsuper_pack_bits(src.data_ptr(), out.data_ptr(), 1, C, V, V, V, stream()) == 0
        assert np.array_equal(out.cpu().numpy().reshape(-1, V), np.packbits(a.reshape(C, V).astype(bool), axis=0)), (C, V)


@pytest.mark.parametrize('dst_off', [0, 16, 5, 37])
def test_pack_bits_strided_into_place(dst_off):
    """A slab in a staging buffer with plane stride > V goes to its place in a larger packed volume (plane stride > V, any offset); bytes outside the
    written ranges keep their sentinel."""
    for B, C, V, ss, ds in ((1, 26, 4099, 4112, 8192), (2, 9, 255, 256 + 16, 512), (1, 42, 17, 23, 61), (1, 8, 32, 48, 64)):
        P = (C + 7) // 8
        a = values((B, C, ss), np.uint8, C + V + dst_off)
        src = torch.from_numpy(a).to(DEV)
        out = torch.full((B * P * ds + dst_off + 16,), 0xEE, dtype=torch.uint8, device=DEV)
        assert L().rsuper_pack_bits(src.data_ptr(), out.data_ptr() + dst_off, B, C, V, ss, ds, stream()) == 0
        got = out.cpu().numpy()
        exp = np.full_like(got, 0xEE)
        for b in range(B):
            pk = np.packbits(a[b, :, :V].astype(bool), axis=0)
            for p in range(P):
                o = dst_off + (b * P + p) * ds
                exp[o:o + V] = pk[p]
        assert np.array_equal(got, exp), (B, C, V, ss, ds, dst_off)


def test_unpack_of_pack_is_nonzero():
    for C, shape in ((26, (5, 7, 9)), (42, (4, 8, 16)), (1, (3, 3, 3))):
        x = torch.from_numpy(values((2, C) + shape, np.int8, C)).to(DEV)
        p = D().pack_bits_device(x)
        assert torch.equal(D().unpack_bits_device(p.packed, C), (x != 0).to(torch.uint8))
        assert torch.equal(p.unpack(), (x != 0).to(torch.uint8))


# ------------------------------------------------------------------------------------------------------------------ upload_label
@pytest.mark.parametrize('C, shape', [(26, (37, 41, 43)), (42, (20, 33, 35))])
def test_upload_label_three_ways(C, shape, tmp_path):
    from rsuper_amd.training.dataset.packed import slab_depth
    lab = (values((C,) + shape, np.int8, C) * (np.random.RandomState(C).rand(C, 1, 1, 1) < 0.7)).astype(np.int8)
    exp = np.packbits(lab.astype(bool), axis=0)
    np.save(tmp_path / 'lab.npy', lab)
    mm = np.load(tmp_path / 'lab.npy', mmap_mode='r')                      # as a worker-less loader hands it over: a read-only map
    plane = C * shape[1] * shape[2]
    chunk = plane * 7                                                      # 7 rows per slab: at least 3 slabs, the last one ragged
    n = slab_depth(C, *shape, chunk)
    assert -(-shape[0] // n) >= 3 and shape[0] % n != 0
    for what, got in (('packed file form', D().upload_label(exp, C, DEV)),
                      ('slabs', D().upload_label(mm, C, DEV, chunk_bytes=chunk)),
                      ('one row per slab', D().upload_label(lab, C, DEV, chunk_bytes=1)),
                      ('bool', D().upload_label(lab.astype(bool), C, DEV, chunk_bytes=chunk)),
                      ('one slab', D().upload_label(torch.from_numpy(lab), C, DEV, chunk_bytes=1 << 40))):
        assert got.C == C and tuple(got.packed.shape) == (1,) + exp.shape
        assert np.array_equal(got.packed.cpu().numpy()[0], exp), what
    with pytest.raises(AssertionError):
        D().upload_label(np.zeros((C // 8 + 3,) + shape, np.uint8), C, DEV)      # the reference's `< num_classes + 10`


# ------------------------------------------------------------------------------------------------------------------ samples against the reference
@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return T.build(str(tmp_path_factory.mktemp('whole_ct_gpu') / 'tree'))


def dataset(tree, **kw):
    random.seed(0)
    kw = dict(dict(mode='train', all_train=True, balance_supervision=False, tumor_classes=list(T.TUMOR_CLASSES)), **kw)
    return W().WholeVolumeDataset(T.args_for(tree), seed=0, crop_on_tumor=True, **kw)


def seed_all(s):
    random.seed(s), np.random.seed(s), torch.manual_seed(s)


def index_of(ds, tree, rec):
    root = tree['data_root' if rec['root'] == 'atlas' else 'UFO_root']
    return [i for i, p in enumerate(ds.img_list) if os.path.dirname(p) == root and os.path.basename(p).startswith(rec['name'])][0]


def one_sample(loader, idx, seed):
    seed_all(seed)
    batch = loader._hand_over(loader._produce([loader.dataset[idx]]))
    nxt = {'np': float(np.random.random()), 'random': random.random(), 'torch': float(torch.rand(1))}
    return batch, nxt


@pytest.fixture(scope='module')
def samples(tree, tmp_path_factory):
    """Every fixture sample once: (record, batch, next draws, the producer's files)."""
    from rsuper_amd import augment_eternal
    ds = dataset(tree)
    loader = W().WholeVolumeLoader(ds, batch_size=1, prefetch=False)
    out = []
    for k, rec in enumerate(G['samples']):
        dest = str(tmp_path_factory.mktemp('crops_%d' % k))
        batch, nxt = one_sample(loader, index_of(ds, tree, rec), rec['seed'])
        names = augment_eternal.write_batch(loader, batch, dest)
        out.append((rec, batch, nxt, dest, names))
    return ds, out


def test_fixture_covers_every_branch():
    recs = G['samples']
    forms = {(T.ATLAS if r['root'] == 'atlas' else T.UFO)[r['name']][1] for r in recs}
    assert len(recs) >= 8 and forms == {'npy_packed', 'npy_unpacked', 'npz_unpacked'}
    assert any(r['affine'] for r in recs) and any(not r['affine'] and not r['ufo'] for r in recs)
    assert any(r['ufo'] and r['selected'] not in (None, 'random') for r in recs)
    assert any(r['ufo'] and r['selected'] == 'random' and 'random_crop_on_tumor' in r['entered'] for r in recs)
    assert any(r['ufo'] and r['entered'] == ['random_crop'] for r in recs)


@pytest.mark.parametrize('k', range(len(G['samples'])))
def test_sample_matches_reference_getitem(samples, k):
    import test_gpu_augment as TA
    from rsuper_amd.training import augmentation as A
    ds, out = samples
    rec, batch, nxt, _, _ = out[k]
    C, (d, h, w) = len(T.CLASSES), T.TRAINING_SIZE
    assert nxt == rec['next'], 'the draws consumed differ'
    assert set(batch) == {'image', 'label', 'unk_channels', 'mask', 'volumes', 'diameters'}
    assert batch['image'].shape == (1, 1, d, h, w) and batch['image'].dtype == torch.float32
    vols = {n: batch[n].packed.cpu().numpy()[0] for n in ('label', 'unk_channels', 'mask')}
    exp = {'label': GZ['label_%d' % k], 'unk_channels': GZ['unk_%d' % k], 'mask': GZ['mask_%d' % k]}
    assert all(batch[n].C == C and vols[n].shape == exp[n].shape for n in vols)
    assert batch['volumes'].cpu().tolist() == [[float(np.float32(v)) for v in rec['volumes']]]
    assert batch['diameters'].cpu().tolist() == [rec['diameters']]
    shape = (T.ATLAS if rec['root'] == 'atlas' else T.UFO)[rec['name']][0]
    full = [max(s, l) for s, l in zip(shape, T.LARGE)]
    img = batch['image'].cpu().numpy()
    if not rec['affine']:
        c = rec['corner']
        assert np.array_equal(img[0, 0], T.padded(T.image(shape), full)[c[0]:c[0] + d, c[1]:c[1] + h, c[2]:c[2] + w])
        for n in vols:
            assert np.array_equal(vols[n], exp[n]), n
    else:
        assert not rec['ufo']
        c, (ld, lh, lw) = rec['large_corner'], T.LARGE
        box = (slice(c[0], c[0] + ld), slice(c[1], c[1] + lh), slice(c[2], c[2] + lw))
        big = torch.from_numpy(np.ascontiguousarray(T.padded(T.image(shape), full)[box]))[None, None]
        lab = np.packbits(T.padded(T.atlas_label(rec['name']), full)[(slice(None),) + box].astype(bool), axis=0)
        theta = torch.tensor(rec['theta'], dtype=torch.float32)
        off = A.crop_offsets(T.LARGE, [d, h, w], 'center')
        f64 = GA.center(GA.trilinear_f64(big, theta), (d, h, w))
        TA.check_case('sample %d' % k, big, [torch.from_numpy(lab)[None]], theta, [d, h, w], off, torch.from_numpy(img),
                      [torch.from_numpy(vols['label'])[None]], torch.from_numpy(GZ['img_%d' % k])[None], [torch.from_numpy(exp['label'])[None]], f64,
                      e_ref=rec['e_ref'])
        assert not vols['unk_channels'].any() and not vols['mask'].any() and not exp['unk_channels'].any() and not exp['mask'].any()


@pytest.mark.parametrize('k', range(len(G['samples'])))
def test_producer_files_match_reference_save(samples, k):
    ds, out = samples
    rec, batch, _, dest, names = out[k]
    files = rec['files']
    assert sorted(os.listdir(dest)) == sorted(files) and names == [rec['name'] + '.npy']
    for f, exp in files.items():
        p = os.path.join(dest, f)
        if f.endswith('.npy'):
            a = np.load(p)
            assert [str(a.dtype), list(a.shape)] == exp, f
            key = {'_gt.npy': 'label', '_gt_unk.npy': 'unk_channels', '_gt_chosen_tumor_segment.npy': 'mask'}.get(f[len(rec['name']):])
            # the bytes the loader gave (compared with the reference's in test_sample_matches_reference_getitem, to its bound on the resampled branch)
            assert np.array_equal(a, batch[key].packed.cpu().numpy()[0] if key else batch['image'].cpu().numpy()[0]), f
            if not rec['affine']:
                assert key is None or np.array_equal(a, GZ[{'label': 'label', 'unk_channels': 'unk', 'mask': 'mask'}[key] + '_%d' % k]), f
        elif f.endswith('.json'):
            with open(p) as fh:
                assert json.load(fh) == exp, f
        else:
            with open(p) as fh:
                assert fh.read() == exp, f
    # and the crop directory reads back to the loader's batch
    back = D().AugmentedCropDataset.from_directory(dest, T.CLASSES, packed=True, augment=False, classes_ufo=T.CLASSES_UFO)
    assert len(back) == 1
    s = back[0]
    assert torch.equal(s['image'], batch['image'][0].cpu())
    for n in ('label', 'unk_channels', 'mask'):
        assert torch.equal(s[n], batch[n].packed[0].cpu()), n
    assert torch.equal(s['volumes'], batch['volumes'][0].cpu()) and torch.equal(s['diameters'], batch['diameters'][0].cpu())


# ------------------------------------------------------------------------------------------------------------------ prefetch, visits, cached totals
def batch_bytes(b):
    return [b['image'].cpu().numpy().tobytes()] + [b[n].packed.cpu().numpy().tobytes() for n in ('label', 'unk_channels', 'mask')] + \
        [b['volumes'].cpu().numpy().tobytes(), b['diameters'].cpu().numpy().tobytes()]


def test_prefetch_on_and_off_give_the_same_bytes(tree):
    ds = dataset(tree)
    order = [(3 * i) % len(ds) for i in range(12)]
    runs = {}
    for prefetch, explicit in ((False, False), (True, False), (True, True)):
        seed_all(11)
        loader = W().WholeVolumeLoader(ds, batch_size=2, sampler=order, prefetch=prefetch)
        got = []
        for b in loader:
            assert set(b) == {'image', 'label', 'unk_channels', 'mask', 'volumes', 'diameters'} and b['image'].shape[0] == 2
            if explicit:
                loader.prefetch_next()             # as the training loop does once the step is queued
            got.append(batch_bytes(b))
        assert len(got) == 6
        runs[(prefetch, explicit)] = got
    assert runs[(False, False)] == runs[(True, False)] == runs[(True, True)]


def test_crops_per_visit_equals_consecutive_visits(tree):
    ds = dataset(tree)
    for i in (0, [j for j in range(len(ds)) if ds.is_ufo(j)][0]):
        seed_all(5)
        (three,) = list(W().WholeVolumeLoader(ds, batch_size=1, sampler=[i], prefetch=False, crops_per_visit=3))
        assert three['image'].shape[0] == 3
        seed_all(5)
        singles = list(W().WholeVolumeLoader(ds, batch_size=1, sampler=[i, i, i], prefetch=True))
        assert len(singles) == 3
        for j, s in enumerate(singles):
            assert torch.equal(three['image'][j:j + 1], s['image'])
            for n in ('label', 'unk_channels', 'mask'):
                assert torch.equal(three[n].packed[j:j + 1], s[n].packed), (n, j)
            assert torch.equal(three['volumes'][j:j + 1], s['volumes'])


def test_revisit_reads_cached_totals(tree, monkeypatch):
    ds = dataset(tree)
    i = [j for j in range(len(ds)) if not ds.is_ufo(j)][0]
    loader = W().WholeVolumeLoader(ds, batch_size=1, prefetch=False)
    reads = []
    for name in ('cpu', 'item', 'tolist'):
        orig = getattr(torch.Tensor, name)
        monkeypatch.setattr(torch.Tensor, name, (lambda o, n: lambda self, *a, **k: (reads.append(n) if self.is_cuda else None, o(self, *a, **k))[1])(orig, name))
    seed_all(2)
    first = loader._crops(ds[i])
    n_first = len(reads)
    assert n_first >= 1 and ds.img_list[i] in loader.totals
    del reads[:]
    second = loader._crops(ds[i])
    assert reads == [], 'a revisit of an annotated volume read the device: %s' % reads
    monkeypatch.undo()
    seed_all(2)
    fresh = W().WholeVolumeLoader(ds, batch_size=1, prefetch=False)
    a = fresh._crops(ds[i])
    b = fresh._crops(ds[i])                       # with the cache the draws and the crops are those of an uncached visit
    seed_all(2)
    c = W().WholeVolumeLoader(ds, batch_size=1, prefetch=False)
    c1 = c._crops(ds[i])
    c.totals.clear()
    c2 = c._crops(ds[i])
    assert torch.equal(b[0][0], c2[0][0]) and torch.equal(b[0][1].packed, c2[0][1].packed) and torch.equal(a[0][0], c1[0][0])
    assert first and second


# ------------------------------------------------------------------------------------------------------------------ end to end, tools
CONFIG = """
classes: 26
modality: CT
arch: unet
in_chan: 1
base_chan: 8
down_scale: [[2,2,2], [2,2,2], [2,2,2], [2,2,2]]
kernel_size: [[3,3,3], [3,3,3], [3,3,3], [3,3,3], [3,3,3]]
block: BasicBlock
norm: in
compute_dtype: bf16
training_size: [32, 32, 32]
window_size: [32, 32, 32]
sliding_window: True
aux_loss: False
aux_weight: [0.5, 0.5]
optimizer: adamw
base_lr: 0.0006
betas: [0.9, 0.999]
weight_decay: 0.05
print_freq: 1
iter_per_epoch: 2
ema: True
ema_alpha: 0.99
val_freq: %d
split_seed: %d
reproduce_seed: 3
"""


def run_training(tree, tmp_path, val_freq, split_seed, extra=()):
    from rsuper_amd import train_ddp
    root = tmp_path / ('cfg_%d' % val_freq)
    os.makedirs(root / 'abdomenatlas_ufo')
    (root / 'abdomenatlas_ufo' / 'unet_3d.yaml').write_text(CONFIG % (val_freq, split_seed))
    argv = ['--dataset', 'abdomenatlas_ufo', '--model', 'unet', '--dimension', '3d', '--batch_size', '2', '--epochs', '1', '--crop_on_tumor',
            '--intensity_aug_device', 'gpu', '--tumor_classes', 'kidney', '--report_volume_loss_basic', '0.1', '--data_root', tree['data_root'],
            '--UFO_root', tree['UFO_root'], '--reports', tree['reports'], '--cp_path', str(tmp_path / 'exp'), '--unique_name', 'v%d' % val_freq] + list(extra)
    args = train_ddp.get_parser(argv, config_root=str(root))
    args.surface_area_table = np.load(os.path.join(ROOT, 'tests', 'golden', 'surface_metrics.npz'))['sm_ct_like_table']
    random.seed(0)
    trainset, testset = train_ddp.build_datasets(args)
    history = train_ddp.main_worker(0, 1, 0, args, trainset=trainset, testset=testset)
    return args, trainset, testset, history


def test_train_ddp_end_to_end(tree, tmp_path):
    from rsuper_amd import train_ddp
    from rsuper_amd.training.dataset.packed import PackedBits
    seen = []
    orig = train_ddp.train_step

    def spy(net, ema_net, optimizer, batch, *a, **k):
        seen.append({n: (type(v), tuple(v.shape), v.dtype if isinstance(v, torch.Tensor) else None) for n, v in batch.items()})
        return orig(net, ema_net, optimizer, batch, *a, **k)
    train_ddp.train_step = spy
    try:
        args, trainset, testset, history = run_training(tree, tmp_path, 10 ** 6, 0)
    finally:
        train_ddp.train_step = orig
    assert len(history) == 1 and np.isfinite(history[0]['overall']) and len(seen) == 2
    assert os.path.exists(os.path.join(args.cp_path, 'abdomenatlas_ufo', args.unique_name, 'fold_0_latest.pth'))
    # the batch is what ingest_packed_batch(keep_packed=True) yields
    ref = D().ingest_packed_batch({'image': torch.zeros(2, 1, 32, 32, 32), 'label': torch.zeros(2, 4, 32, 32, 32, dtype=torch.uint8),
                                   'unk_channels': torch.zeros(2, 4, 32, 32, 32, dtype=torch.uint8), 'mask': torch.zeros(2, 4, 32, 32, 32, dtype=torch.uint8),
                                   'volumes': torch.zeros(2, 10), 'diameters': torch.zeros(2, 10, 3)}, 26, DEV, keep_packed=True)
    want = {n: (type(v), tuple(v.shape), v.dtype if isinstance(v, torch.Tensor) else None) for n, v in ref.items()}
    assert all(s == want for s in seen) and want['label'][0] is PackedBits
    # without the device intensity stage the whole-CT path refuses to run rather than skip the transforms
    with pytest.raises(ValueError, match='no host intensity stage'):
        run_training(tree, tmp_path / 'cpu', 10 ** 6 + 1, 0, extra=['--intensity_aug_device', 'cpu'])


def test_train_ddp_validates_on_whole_test_volumes(tree, tmp_path):
    # a split seed whose one test case is an annotated volume (a report volume has no per-voxel labels of `classes` to validate against)
    for seed in range(50):
        te = W().WholeVolumeDataset(T.args_for(tree), mode='test', seed=seed, tumor_classes=list(T.TUMOR_CLASSES))
        if te.Atlas_paths:
            break
    assert te.Atlas_paths
    args, trainset, testset, history = run_training(tree, tmp_path, 1, seed)
    assert testset.img_list == te.img_list and len(history) == 1
    dice, asd, hd = args.best_validation
    name = os.path.basename(te.img_list[0])[:14]
    present = np.nonzero(T.atlas_label(name).reshape(26, -1).any(1))[0]
    assert len(dice) == 26 and len(present) >= 5
    assert np.isfinite(dice[present]).all() and np.isfinite(asd[present]).all() and np.isfinite(hd[present]).all()
    assert np.isnan(np.delete(dice, present)).all()
    assert os.path.exists(os.path.join(args.cp_path, 'abdomenatlas_ufo', args.unique_name, 'fold_0_best.pth'))


def test_pack_dataset_then_same_samples(tree, tmp_path):
    from rsuper_amd.tools import pack_dataset
    conv = {}
    for key in ('data_root', 'UFO_root'):
        conv[key] = str(tmp_path / key)
        pack_dataset.main(['--src', tree[key], '--dst', conv[key], '--chunk_bytes', str(1 << 20)])
        names = sorted(f for f in os.listdir(conv[key]) if f != 'list')
        ids = sorted(T.ATLAS if key == 'data_root' else T.UFO)
        assert names == sorted([i + '.npy' for i in ids] + [i + '_gt.npy' for i in ids])
        assert open(os.path.join(conv[key], 'list', 'label_names.yaml')).read() == open(os.path.join(tree[key], 'list', 'label_names.yaml')).read()
    i = 'BDMAP_00000003'
    lab = np.load(os.path.join(conv['data_root'], i + '_gt.npy'), mmap_mode='r')
    assert lab.dtype == np.uint8 and np.array_equal(lab, np.packbits(T.atlas_label(i).astype(bool), axis=0))
    assert np.array_equal(np.load(os.path.join(conv['data_root'], i + '.npy')), T.image(T.ATLAS[i][0]))
    a, b = dataset(tree), dataset(dict(tree, **conv))
    assert [os.path.basename(p)[:14] for p in a.img_list] == [os.path.basename(p)[:14] for p in b.img_list]
    la, lb = W().WholeVolumeLoader(a, batch_size=1, prefetch=False), W().WholeVolumeLoader(b, batch_size=1, prefetch=False)
    for idx in range(len(a)):
        (x, _), (y, _) = one_sample(la, idx, 20 + idx), one_sample(lb, idx, 20 + idx)
        assert batch_bytes(x) == batch_bytes(y), a.img_list[idx]


def test_augment_eternal_one_pass(tree, tmp_path):
    from rsuper_amd import augment_eternal
    dest = str(tmp_path / 'crops')
    seed_all(0)
    augment_eternal.main(['--data_root', tree['data_root'], '--UFO_root', tree['UFO_root'], '--reports', tree['reports'], '--save_destination', dest,
                          '--training_size'] + [str(s) for s in T.TRAINING_SIZE] + ['--tumor_classes', 'kidney', '--crop_on_tumor', '--passes', '1',
                                                                                      '--crops_per_visit', '2'])
    files = set(os.listdir(dest))
    ids = sorted(T.ATLAS) + [i for i in T.ELIGIBLE_UFO if i not in T.ATLAS]
    for i in ids:
        for stem in (i, i + '_v1'):
            want = {stem + s for s in ('.npy', '_gt.npy', '_gt_unk.npy', '_gt_chosen_tumor_segment.npy', '.json', '_tumor_volumes.json', '_tumor_diameters.json')}
            if i not in T.ATLAS:
                want.add(stem + '.csv')
            assert want <= files, sorted(want - files)
    assert len(files) == sum(2 * (7 if i in T.ATLAS else 8) for i in ids)
    back = D().AugmentedCropDataset.from_directory(dest, T.CLASSES, packed=True, augment=False, classes_ufo=T.CLASSES_UFO)
    assert len(back) == 2 * len(ids)
    for k in range(len(back)):
        s = back[k]
        assert s['image'].shape == (1,) + T.TRAINING_SIZE and s['label'].shape == (4,) + T.TRAINING_SIZE
