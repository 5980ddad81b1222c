"""Host-side tests of training from whole CTs (no device): the report cleaning and the dataset construction against the reference's results in
tests/golden/whole_ct.json (tests/golden/gen_golden_whole_ct.py, on the tree of tests/whole_ct_tree.py), the new command-line options, the C ABI of
rsuper_pack_bits, and what a DataLoader worker may touch."""
import argparse
import ctypes
import json
import os
import random
import re
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)
import whole_ct_tree as T  # noqa: E402

with open(os.path.join(ROOT, 'tests', 'golden', 'whole_ct.json')) as f:
    G = json.load(f)


def W():
    from rsuper_amd.training.dataset import whole_ct
    return whole_ct


@pytest.fixture(scope='module')
def tree(tmp_path_factory):
    return T.build(str(tmp_path_factory.mktemp('whole_ct') / 'tree'))


def make(tree, **kw):
    random.seed(0)
    kw.setdefault('tumor_classes', list(T.TUMOR_CLASSES))
    return W().WholeVolumeDataset(T.args_for(tree), seed=0, crop_on_tumor=True, **kw)


def base(paths):
    return sorted(os.path.basename(p) for p in paths)


# ------------------------------------------------------------------------------------------------------------------ report cleaning
@pytest.mark.parametrize('k', range(len(T.CLEAN_TUMORS)))
def test_clean_ufo_matches_reference(k):
    g = G['clean'][k]
    table = T.clean_table()
    assert 35 <= len(table) <= 45 and g['tumors'] == T.CLEAN_TUMORS[k]
    assert [bool(v) for v in W().normalize_no_lesion(table['no lesion'])] == g['healthy']
    rows, ids, per_type = W().clean_ufo(table.copy(), list(T.CLEAN_TUMORS[k]))
    assert [int(i) for i in rows.index] == g['kept']
    assert set(ids) == set(g['ids']) and len(ids) == len(g['ids'])
    assert per_type == g['per_type']
    # the table does what it was written for: the healthy cap acts (rows sampled with random_state=42) and every kind of case is dropped somewhere
    healthy_true = int((table['no lesion'] == True).sum())                      # noqa: E712
    assert len(per_type['healthy']) < healthy_true
    assert {'BDMAP_00000003', 'BDMAP_00000005', 'BDMAP_00000007', 'BDMAP_00000009', 'BDMAP_00000016'}.isdisjoint(ids)


def test_normalize_no_lesion_bool_column_passes_through():
    import pandas as pd
    col = pd.Series([True, False, True])
    assert W().normalize_no_lesion(col) is col


# ------------------------------------------------------------------------------------------------------------------ construction
@pytest.mark.parametrize('key, kw', [('train', dict(mode='train')), ('test', dict(mode='test')), ('all_train', dict(mode='train', all_train=True)),
                                     ('all_train_unbalanced', dict(mode='train', all_train=True, balance_supervision=False)),
                                     ('ufo_only', dict(mode='train', all_train=True, UFO_only=True, balance_supervision=False)),
                                     ('atlas_only', dict(mode='train', all_train=True, Atlas_only=True, balance_supervision=False))])
def test_construction_matches_reference_as_sets_and_counts(tree, key, kw):
    g = G['build'][key]
    ds = make(tree, **kw)
    assert ds.classes == g['classes'] == T.CLASSES and ds.classes_UFO == g['classes_ufo'] == T.CLASSES_UFO
    assert ds.lesion_classes == g['lesion_classes'] == [T.CLASSES.index('kidney_lesion')]
    assert sorted(set(ds.reports['BDMAP_ID'])) == g['report_ids'] == T.ELIGIBLE_UFO
    assert ds.eligible_ufo == T.ELIGIBLE_UFO and ds.eligible_atlas == sorted(T.ATLAS)           # the id without its _gt file is not a case
    assert len(ds) == len(ds.img_list) == len(ds.lab_list) == g['n']
    if key in ('train', 'test', 'all_train'):
        # which names the split takes and which names balance_supervision repeats follows the order of the name lists, which the reference takes
        # from sets (not pinned): the sizes are -- 10 distinct names, one of them tested; with all_train 6 + 6 names after the equalisation
        assert g['n'] == {'train': 9, 'test': 1, 'all_train': 12}[key]
        assert set(base(ds.img_list)) <= set(G['build']['all_train_unbalanced']['img_list'])
    else:
        assert base(ds.img_list) == g['img_list'] and base(ds.UFO_paths) == g['ufo'] and base(ds.Atlas_paths) == g['atlas']
    if key in ('atlas_only', 'ufo_only'):
        assert len(g['lab_list']) > len(g['img_list'])
        # the reference filters img_list alone and leaves lab_list misaligned; here the two stay aligned
        assert [p.replace('_gt', '') for p in ds.lab_list] == ds.img_list
    else:
        assert base(ds.lab_list) == g['lab_list'] or key in ('train', 'test', 'all_train')
    for p, q in zip(ds.img_list, ds.lab_list):
        assert os.path.exists(p) and os.path.exists(q) and os.path.dirname(p) == os.path.dirname(q)


def test_split_sizes_and_both_root_id(tree):
    # the reference equalises the two kinds of supervision in train mode only, so with balance_supervision the two modes shuffle different lists
    # (mirrored); without it both modes see one list and the split is a partition of the 10 distinct names
    tr, te = make(tree, mode='train', balance_supervision=False), make(tree, mode='test', balance_supervision=False)
    n = len(T.ATLAS) + len(T.ELIGIBLE_UFO)
    assert len(te) == min(200, n // 10) == 1 and len(tr) == 9 and set(tr.img_list).isdisjoint(te.img_list)
    assert len(make(tree, mode='train')) == 9 and len(make(tree, mode='test')) == 1
    un = make(tree, mode='train', all_train=True, balance_supervision=False)
    both = [p for p in un.img_list if 'BDMAP_00000003' in p]
    assert len(both) == 2 and all(os.path.dirname(p) == tree['data_root'] for p in both)         # an id of both roots is read from the annotated one
    uo = make(tree, mode='train', all_train=True, UFO_only=True, balance_supervision=False)
    assert not any('BDMAP_00000003' in p for p in uo.img_list) and len(uo) == 4
    ao = make(tree, mode='train', all_train=True, Atlas_only=True, balance_supervision=False)
    assert not any('BDMAP_00000003' in p for p in ao.img_list) and len(ao) == 5 and not ao.UFO_paths


def test_order_is_decided_by_the_seed(tree):
    a, b = make(tree, mode='train', all_train=True), make(tree, mode='train', all_train=True)
    assert a.img_list == b.img_list and a.lab_list == b.lab_list
    c = W().WholeVolumeDataset(T.args_for(tree), seed=1, all_train=True, tumor_classes=list(T.TUMOR_CLASSES), balance_supervision=False)
    d = W().WholeVolumeDataset(T.args_for(tree), seed=0, all_train=True, tumor_classes=list(T.TUMOR_CLASSES), balance_supervision=False)
    assert sorted(c.img_list) == sorted(d.img_list) and c.img_list != d.img_list
    code = ('import sys; sys.path[:0] = [%r, %r]; import whole_ct_tree as T, random; random.seed(0); '
            'from rsuper_amd.training.dataset.whole_ct import WholeVolumeDataset as D; '
            'print(D(T.args_for(%r), seed=0, all_train=True, tumor_classes=list(T.TUMOR_CLASSES)).img_list)') % (ROOT, os.path.join(ROOT, 'tests'), tree)
    import subprocess
    outs = {subprocess.run([sys.executable, '-c', code], env=dict(os.environ, PYTHONHASHSEED=h), capture_output=True, text=True, check=True).stdout
            for h in ('1', '2')}
    assert len(outs) == 1 and eval(outs.pop()) == a.img_list                                # the same in processes that hash strings differently


def test_errors(tree, tmp_path):
    with pytest.raises(ValueError, match='both UFO_only and Atlas_only'):
        make(tree, UFO_only=True, Atlas_only=True)
    # a lesion class among the report root's classes
    import shutil
    bad = str(tmp_path / 'ufo_bad')
    shutil.copytree(tree['UFO_root'], bad)
    with open(os.path.join(bad, 'list', 'label_names.yaml'), 'a') as f:
        f.write('- kidney_cyst\n')
    with pytest.raises(ValueError, match='UFO classes should not contain'):
        W().WholeVolumeDataset(T.args_for(tree, UFO_root=bad), tumor_classes=list(T.TUMOR_CLASSES))
    # ids without report rows: at construction, and when a case's rows are asked for
    ds = make(tree, mode='train', all_train=True, balance_supervision=False)
    i = ds.img_list.index([p for p in ds.UFO_paths if 'BDMAP_00001001' in p][0])
    assert list(ds.read_report(i)['Standardized Location']) == ['left']
    ds.reports = ds.reports[ds.reports['BDMAP_ID'] != 'BDMAP_00001001']
    with pytest.raises(ValueError, match='ID is not in the reports'):
        ds.read_report(i)
    orig = W().clean_ufo
    try:
        W().clean_ufo = lambda r, t: (orig(r, t)[0], orig(r, t)[1] + ['BDMAP_00008888'], {})
        with pytest.raises(ValueError, match='IDs not in reports'):
            make(tree)
    finally:
        W().clean_ufo = orig
    with pytest.raises(ValueError, match='need both'):
        W().WholeVolumeDataset(T.args_for(tree, reports=None))


def test_annotated_root_alone_serves_abdomenatlas(tree):
    ds = W().WholeVolumeDataset(T.args_for(tree, UFO_root=None, reports=None), all_train=True, tumor_classes=list(T.TUMOR_CLASSES))
    assert base(ds.img_list) == base(ds.Atlas_paths) and len(ds) == len(T.ATLAS) and ds.classes_UFO is None and ds.reports is None
    assert not ds.UFO_paths and all(not ds.is_ufo(i) for i in range(len(ds)))


# ------------------------------------------------------------------------------------------------------------------ parser, build_datasets
README_COMMANDS = [
    "--dataset abdomenatlas --model medformer --dimension 3d --batch_size 2 --unique_name mask_only_model_name --crop_on_tumor --gpu 0 --workers 4 "
    "--load_augmented --save_destination /path/to/crops/ --data_root /path/to/masks_npz/ --epochs 100 --lr 0.001 --dist_url tcp://127.0.0.1:8001 "
    "--report_volume_loss_basic 0",
    "--dataset abdomenatlas_ufo --model medformer --dimension 3d --batch_size 2 --unique_name mask_and_report_model_name --crop_on_tumor --gpu 0 "
    "--workers 2 --load_augmented --pretrain --pretrained exp/abdomenatlas/mask_only_model_name/fold_0_latest.pth --loss ball_dice_last "
    "--dist_url tcp://127.0.0.1:8002 --report_volume_loss_basic 0.1 --save_destination /path/to/crops/ --data_root /path/to/masks_npz/ "
    "--UFO_root /path/to/reports_npz/ --epochs 100 --lr 0.0001 --reports /path/to/LLM_per_CT_metadata.csv",
    "--dataset abdomenatlas_ufo --model medformer --dimension 3d --batch_size 4 --unique_name merlin_pancreas --crop_on_tumor --gpu 0,1 --workers 8 "
    "--load_augmented --pancreas_only --tumor_classes pancreas --all_train --save_destination /d/ --data_root /a/ --UFO_root /u/ --epochs 10 "
    "--reports /r.csv --ucsf_ids /ids.csv",
]


@pytest.mark.parametrize('cmd', README_COMMANDS)
def test_training_command_lines_parse(cmd, tmp_path):
    from rsuper_amd import train_ddp
    for ds in ('abdomenatlas', 'abdomenatlas_ufo'):
        os.makedirs(tmp_path / ds, exist_ok=True)
        (tmp_path / ds / 'medformer_3d.yaml').write_text('classes: 26\ntraining_size: [32, 32, 32]\nsplit_seed: 0\n')
    a = train_ddp.get_parser(cmd.split(), config_root=str(tmp_path))
    assert a.crop_on_tumor is True and a.gpu in ('0', '0,1') and a.load_augmented and a.training_size == [32, 32, 32]
    assert a.UFO_only is False and a.Atlas_only is False and a.kidney_only is False and a.save_augmented is False
    if 'merlin' in cmd:
        assert a.pancreas_only and a.tumor_classes == ['pancreas'] and a.all_train and a.ucsf_ids == '/ids.csv'
    else:
        assert a.tumor_classes is None and a.ucsf_ids is None and not a.all_train and not a.pancreas_only


def test_parser_defaults_and_abdomenatlas_config():
    from rsuper_amd import train_ddp
    for model in ('unet', 'medformer'):
        a = train_ddp.get_parser(['--dataset', 'abdomenatlas', '--model', model])
        assert a.crop_on_tumor is False and a.gpu == '0,1,2,3' and a.training_size and a.classes > 0 and a.iter_per_epoch > 0
    for f in ('unet_3d.yaml', 'medformer_3d.yaml'):              # this project's own text, not the reference's file
        mine = open(os.path.join(ROOT, 'r-super_amd', 'config', 'abdomenatlas', f)).read()
        assert 'rsuper_amd' in mine or 'abdomenatlas' in mine


def test_build_datasets(tree):
    from rsuper_amd import train_ddp
    a = T.args_for(tree, dataset='abdomenatlas_ufo', dimension='3d', crop_on_tumor=True, tumor_classes=list(T.TUMOR_CLASSES), all_train=False)
    random.seed(0)
    tr, te = train_ddp.build_datasets(a)
    assert tr.mode == 'train' and te.mode == 'test' and len(te) == 1 and tr.tumor_classes == ['kidney'] and tr.crop_on_tumor
    tr, te = train_ddp.build_datasets(T.args_for(tree, dataset='abdomenatlas_ufo', dimension='3d', kidney_only=True, all_train=True, UFO_only=True))
    assert te is None and tr.tumor_classes == ['kidney'] and not tr.Atlas_paths and not tr.crop_on_tumor
    tr, _ = train_ddp.build_datasets(T.args_for(tree, dataset='abdomenatlas', dimension='3d', all_train=True, tumor_classes=['kidney']))
    assert tr.classes_UFO is None and len(tr) == len(T.ATLAS) and tr.tumor_classes == ['kidney', 'pancreas']      # get_dataset passes none for this dataset
    for kw, msg in ((dict(dataset='abdomenatlas', pancreas_only=True), 'pancreas_only and kidney_only'),
                    (dict(dataset='abdomenatlas', kidney_only=True), 'pancreas_only and kidney_only'),
                    (dict(dataset='abdomenatlas', UFO_only=True), 'Atlas_only and UFO_only'),
                    (dict(dataset='abdomenatlas', Atlas_only=True), 'Atlas_only and UFO_only'),
                    (dict(dataset='lits'), "doesn't exist"),
                    (dict(dataset='abdomenatlas_ufo', data_root=None), 'needs --data_root')):
        with pytest.raises(ValueError, match=msg):
            train_ddp.build_datasets(T.args_for(tree, dimension='3d', **kw))


# ------------------------------------------------------------------------------------------------------------------ C ABI
def test_pack_bits_c_abi_surface():
    from rsuper_amd.hip import lib
    header = open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read()
    m = re.search(r'int rsuper_pack_bits\(([^)]*)\);', header)
    assert m, 'rsuper_pack_bits is not declared in include/rsuper_hip.h'
    res, args = lib._SIGS['rsuper_pack_bits']
    assert res is ctypes.c_int and len(args) == len(m.group(1).split(',')) == 8
    assert 'rsuper_pack_bits' in lib.exported_symbols()
    L = lib.lib()                                              # resolves the symbol in the shared library
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf)
    ARG = 1
    assert lib.ERR[ARG] == 'RSUPER_ERR_ARG'
    # refused before anything is launched: no device is needed
    assert L.rsuper_pack_bits(None, p, 1, 1, 16, 16, 16, None) == ARG
    assert L.rsuper_pack_bits(p, None, 1, 1, 16, 16, 16, None) == ARG
    assert L.rsuper_pack_bits(p, p, 0, 1, 16, 16, 16, None) == ARG
    assert L.rsuper_pack_bits(p, p, 1, 0, 16, 16, 16, None) == ARG
    assert L.rsuper_pack_bits(p, p, 1, -3, 16, 16, 16, None) == ARG
    assert L.rsuper_pack_bits(p, p, 1, 1, 0, 16, 16, None) == ARG
    assert L.rsuper_pack_bits(p, p, 1, 1, 16, 15, 16, None) == ARG
    assert L.rsuper_pack_bits(p, p, 1, 1, 16, 16, 15, None) == ARG


def test_device_entry_points_refuse_host_tensors():
    from rsuper_amd.hip.lib import RSuperHipError
    from rsuper_amd.training.dataset import pack_bits_device, upload_label
    with pytest.raises(RSuperHipError):
        pack_bits_device(torch.zeros(3, 2, 2, 2, dtype=torch.uint8))
    with pytest.raises(RSuperHipError):
        upload_label(np.zeros((3, 2, 2, 2), np.int8), 3, device='cpu')


def test_slab_depth():
    from rsuper_amd.training.dataset.packed import slab_depth
    assert slab_depth(26, 37, 41, 43, 1) == 1                                   # at least one row
    assert slab_depth(26, 37, 41, 43, 1 << 40) == 37                            # one slab
    assert slab_depth(42, 400, 512, 512, 64 << 20) == 6 and slab_depth(42, 400, 512, 512, 8 << 20) == 1
    n = slab_depth(26, 64, 10, 10, 26 * 100 * 7)                                # 100 voxels per row: depths that are multiples of 4 land 16-byte aligned
    assert n == 4 and (n * 100) % 16 == 0


# ------------------------------------------------------------------------------------------------------------------ workers
def test_getitem_returns_the_stored_bytes_and_workers_open_no_device(tree):
    ds = make(tree, mode='train', all_train=True, balance_supervision=False)
    seen = set()
    for i, p in enumerate(ds.img_list):
        s = ds[i]
        name = os.path.basename(p)[:T.ID_LEN] if hasattr(T, 'ID_LEN') else os.path.basename(p)[:14]
        ufo = os.path.dirname(p) == tree['UFO_root']
        shape, form = (T.UFO if ufo else T.ATLAS)[name][:2]
        lab = (T.ufo_label if ufo else T.atlas_label)(name)
        assert s['path'] == p and s['is_ufo'] == ufo and tuple(s['image'].shape) == shape and s['image'].dtype == np.float32
        stored = np.asarray(s['label'])
        if form == 'npy_packed':
            assert stored.dtype == np.uint8 and np.array_equal(stored, np.packbits(lab.astype(bool), axis=0))
        else:
            assert stored.dtype == np.int8 and np.array_equal(stored, lab)
        assert (s['report'] is not None) == ufo and 'spacing' not in s
        if ufo:
            assert list(s['report']['BDMAP_ID'].unique()) == [name]
        seen.add(form)
    assert seen == {'npy_packed', 'npy_unpacked', 'npz_unpacked'}
    te = make(tree, mode='test')
    assert list(te[0]['spacing']) == [1.0, 1.0, 1.0]
    loader = torch.utils.data.DataLoader(ds, batch_size=2, num_workers=2, collate_fn=W().collate_volumes)
    n = 0
    for batch in loader:
        assert isinstance(batch, list) and all(isinstance(b['label'], torch.Tensor) and b['label'].dtype in (torch.uint8, torch.int8) for b in batch)
        n += len(batch)
    assert n == len(ds) and not torch.cuda.is_initialized()


def test_a_file_that_cannot_be_read_is_replaced_once_then_raises(tree, tmp_path):
    import shutil
    root = str(tmp_path / 'atlas')
    shutil.copytree(tree['data_root'], root)
    ds = W().WholeVolumeDataset(T.args_for(tree, data_root=root, UFO_root=None, reports=None), all_train=True, tumor_classes=list(T.TUMOR_CLASSES))
    bad = [i for i, p in enumerate(ds.img_list) if 'BDMAP_00000001' in p][0]
    with open(ds.lab_list[bad], 'wb') as f:
        f.write(b'not a numpy file')
    np.random.seed(3)
    other = int(np.random.randint(len(ds)))
    assert other != bad
    np.random.seed(3)
    assert ds[bad]['path'] == ds.img_list[other]                  # another case, drawn from numpy's global generator
    for q in ds.lab_list:
        with open(q, 'wb') as f:
            f.write(b'not a numpy file')
    with pytest.raises(ValueError, match='Error loading'):
        ds[bad]
