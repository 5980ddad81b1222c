"""CPU tests of the NIfTI -> packed-case conversion (dataset_conversion/, csrc/nii_dataset.hip): the numpy restatement against the reference's own
outputs (tests/golden/nii_dataset.npz, written by the unmodified nii2npz.process_file), the host-side pieces of the command line, and the C ABI."""
import ctypes
import inspect
import json
import os
import re

import numpy as np
import pytest

import nifti_ref as nr
import nii_dataset_ref as ndr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, 'tests', 'golden')
IDENT = ((0, 1, 2), (False, False, False))


@pytest.fixture(scope='module')
def fixture():
    g = np.load(os.path.join(GOLDEN, 'nii_dataset.npz'))
    with open(os.path.join(GOLDEN, 'nii_dataset.json')) as f:
        meta = json.load(f)
    return g, meta


def _canon_masks(g, meta):
    shape = tuple(meta['shape'])
    n = int(np.prod(shape))
    return {k: np.unpackbits(g[k])[:n].reshape(shape) for k in ('liver', 'liver_lesion')}


def _as_file(canon_zyx):
    """A canonical (Z, Y, X) array as the (ni, nj, nk) array of a file in the identity orientation."""
    return nr.inverse_reorient(canon_zyx, *IDENT), IDENT[0], IDENT[1]


def test_restatement_matches_reference_fixture(fixture):
    """Labels bit for bit; the image within 4 x the distance between the reference's float32 arithmetic and the float64 restatement on this fixture.
    Measured when the fixture was written: reference vs float64 (ddof = 0) 1.500e-07, so the bound is 6.0e-07; for scale, the same image under
    ddof = 1 lies 2.193e-06 away.  Both numbers are read from nii_dataset.json, not restated here."""
    g, meta = fixture
    Z, Y, X = meta['shape']
    masks = {k: _as_file(v) for k, v in _canon_masks(g, meta).items()}
    masks['background'] = None
    lab = ndr.label_stack(meta['class_names'], masks, (X, Y, Z), (1.0, 1.0, 1.0))
    assert sorted(np.unique(lab[0]).tolist()) == g['ref_bkg_values'].tolist() == [-1, 0, 1]
    packed = ndr.packed_labels(lab, 128)
    assert packed.shape == (1,) + tuple(meta['padded_shape']) and np.array_equal(packed, g['ref_lab'])
    exact = ndr.zscore(g['img'], 128, ddof=0)
    dist = float(np.abs(g['ref_img'].astype(np.float64) - exact).max())
    assert dist == pytest.approx(meta['ref_vs_float64'], rel=1e-6) and meta['ref_vs_float64'] == pytest.approx(1.5e-7, rel=0.01)
    print(f'reference vs float64: {dist:.3e}, bound {4 * meta["ref_vs_float64"]:.3e}')
    assert dist <= 4 * meta['ref_vs_float64'] and meta['ref_vs_float64_ddof1'] > 4 * meta['ref_vs_float64']
    dz, dy, dx = ndr.pad_widths((Z, Y, X), 128)
    assert (dz, dy, dx) == (54, 1, 0)
    ref = g['ref_img']
    assert not ref[:dz].any() and not ref[-dz:].any() and not ref[:, :dy].any() and not ref[:, -dy:].any()


def test_background_quirk_on_overlap_and_empty_voxel():
    a = np.zeros((2, 3, 4), np.uint8)
    b = np.zeros((2, 3, 4), np.uint8)
    a[0, 0, :3] = 1
    b[0, 0, 2:] = 1                                # (0, 0, 2) is an overlap, (0, 0, 3) only b, (1, *, *) nothing
    masks = {'background': None, 'liver': _as_file(a), 'liver_lesion': _as_file(b)}
    lab = ndr.label_stack(['liver', 'background', 'liver_lesion'], masks, (4, 3, 2), (1.0, 1.0, 1.0))
    assert lab[0, 0, 0].tolist() == [0, 0, -1, 0] and (lab[0, 1] == 1).all()
    bits = np.packbits(lab.astype(bool), axis=0)[0]
    assert bits[0, 0].tolist() == [0x40, 0x40, 0xE0, 0x20] and (bits[1] == 0x80).all()      # overlap: background AND both classes; empty: background
    packed = ndr.packed_labels(lab, 6)
    assert packed.shape == (1, 6, 7, 6) and not packed[0, :2].any() and not packed[0, :, :2].any() and not packed[0, :, :, :1].any()
    # a present background file is read like any class
    masks['background'] = _as_file(np.ones((2, 3, 4), np.uint8))
    assert (ndr.label_stack(list(masks), masks, (4, 3, 2), (1.0, 1.0, 1.0))[0] == 1).all()


def test_parser_flags_and_defaults_equal_the_references(fixture):
    """Every flag of the reference's two parsers exists; the defaults are the reference's, except that the three paths -- whose reference defaults are
    directories of its authors' cluster and differ between the two scripts -- are required here."""
    from rsuper_amd.dataset_conversion import nii2packed
    _, meta = fixture
    p = nii2packed.build_parser()
    mine = {a.option_strings[0]: a for a in p._actions if a.option_strings and a.option_strings[0] != '-h'}
    paths = {'--src_path', '--label_path', '--tgt_path'}
    for script, flags in meta['parsers'].items():
        for flag, default in flags.items():
            assert flag in mine, f'{script}: {flag} is missing'
            if flag in paths:
                assert mine[flag].required and mine[flag].default is None
            else:
                assert mine[flag].default == default and not mine[flag].required, (script, flag)
    assert set(meta['parsers']['abdomenatlas_3d']) | set(meta['parsers']['nii2npz']) | {'--nnunet_labels', '--min_size'} == set(mine)
    assert mine['--min_size'].default == 128 and mine['--nnunet_labels'].default is None
    a = p.parse_args(['--src_path', 's', '--label_path', 'l', '--tgt_path', 't'])
    assert (a.parts, a.current_part, a.workers, a.overwrite, a.nnunet_labels_used) == (1, 0, 8, False, False)


def test_add_lesions_deduplicates_and_sorts():
    from rsuper_amd.dataset_conversion import nii2packed
    assert nii2packed.merge_lesions(['spleen', 'liver', 'kidney_lesion'], ['pancreatic_lesion', 'kidney_lesion', 'liver_lesion']) == \
        ['kidney_lesion', 'liver', 'liver_lesion', 'pancreatic_lesion', 'spleen']


def test_array_split_parts():
    from rsuper_amd.dataset_conversion import nii2packed
    names = ['BDMAP_%08d' % i for i in range(7)]
    parts = [nii2packed.split_part(names, 3, k) for k in range(3)]
    assert parts == [s.tolist() for s in np.array_split(names, 3)] and [len(p) for p in parts] == [3, 2, 2]
    assert nii2packed.split_part(names, 1, 0) == names and nii2packed.split_part(names[:2], 2, 1) == names[1:2]
    with pytest.raises(ValueError):
        nii2packed.split_part(names, 3, 3)


def test_lut_from_the_reference_table_with_joint_classes(fixture):
    from rsuper_amd.dataset_conversion import nii_dataset
    _, meta = fixture
    table = meta['nnunet_labels']
    names = sorted(table)
    assert len(names) == 35 and 'background' not in names and 'hepatic_vessel' not in names
    lut = nii_dataset.build_lut(names, table)
    assert lut.shape == (35, 5) and lut.dtype == np.uint8 and not lut[0].any()
    bits = np.unpackbits(lut, axis=1)[:, :len(names)]                         # (value, class)
    for c, n in enumerate(names):
        vals = table[n] if isinstance(table[n], list) else [table[n]]
        assert np.flatnonzero(bits[:, c]).tolist() == sorted(vals)
    liver, seg3 = names.index('liver'), names.index('liver_segment_3')
    assert np.flatnonzero(bits[26]).tolist() == sorted([liver, seg3])          # a segment's value sets the segment and the joint class
    assert np.flatnonzero(bits[17]).tolist() == [liver]                        # hepatic vessel: part of the liver, no class of its own
    assert np.flatnonzero(bits[33]).tolist() == sorted([names.index('pancreas'), names.index('pancreas_body')])
    assert not np.unpackbits(lut, axis=1)[:, len(names):].any()                # the padding bits of the last plane
    with pytest.raises(ValueError):
        nii_dataset.build_lut(['a'], {'a': -1})


def test_pad_geometry_and_tables():
    from rsuper_amd.dataset_conversion import nii_dataset
    assert nii_dataset.pad_geometry((20, 127, 128)) == ((128, 129, 128), (54, 1, 0))
    assert nii_dataset.pad_geometry((7, 16, 17), 16) == ((17, 16, 17), (5, 0, 0))
    for n, sp in ((9, 0.7), (5, 2.5), (13, 1.0), (4, 3.1)):
        t = nii_dataset.nearest_tables((n, n, n), (sp, sp, sp), (1.0, 1.0, 1.0))
        assert all(np.array_equal(v, nr.nearest_table(n, sp, 1.0)) for v in t)


def test_symbols_declared_bound_exported_with_matching_arity():
    from rsuper_amd.hip import lib, library
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read(), flags=re.S)
    for name, arity in (('rsuper_label_gather_pack', 24), ('rsuper_label_background', 13), ('rsuper_ct_normalize_pop', 18)):
        m = re.search(r'int %s\(([^)]*)\)' % name, hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        res, argtypes = lib._SIGS[name]
        assert res is ctypes.c_int and len(argtypes) == len(m.group(1).split(',')) == arity
        assert name in lib.exported_symbols() and hasattr(lib.lib(), name)
    assert lib._SIGS['rsuper_ct_normalize_pop'] == lib._SIGS['rsuper_ct_normalize'] and len(lib._SIGS['rsuper_ct_normalize'][1]) == 18
    assert re.search(r'#define RSUPER_LABEL_DESC_WORDS 8\b', hdr)
    assert list(inspect.signature(library.install_nii_dataset_ops).parameters) == ['label_gather_pack', 'label_background', 'ct_normalize_pop']
    assert 'nii_dataset.hip' in open(os.path.join(ROOT, 'r-super_amd', 'csrc', 'Makefile')).read()


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host side of the C ABI: the pointers are never dereferenced and no device is needed."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    raw, desc, t, dst = ctypes.c_void_p(1 << 20), ctypes.c_void_p(2 << 20), ctypes.c_void_p(3 << 20), ctypes.c_void_p(4 << 20)

    def gather(raw=raw, nbytes=4096, desc=desc, nclass=3, lut=None, n_values=0, P=1, box=(5, 6, 7), out=(9, 9, 9), off=(1, 1, 1), dst=dst):
        return L.rsuper_label_gather_pack(raw, nbytes, desc, nclass, lut, n_values, P, t, t, t, 5, 6, 7, box[0], box[1], box[2], dst, out[0], out[1], out[2],
                                          off[0], off[1], off[2], None)
    assert gather(raw=None) == 1 and gather(desc=None) == 1 and gather(dst=None) == 1 and gather(nbytes=0) == 1
    assert gather(raw=ctypes.c_void_p((1 << 20) + 2)) == 1 and gather(desc=ctypes.c_void_p((2 << 20) + 4)) == 1       # misaligned
    assert gather(nclass=0) == 1 and gather(nclass=9) == 1 and gather(P=2) == 1
    assert gather(lut=t, nclass=2, n_values=4) == 1 and gather(lut=t, nclass=1, n_values=0) == 1 and gather(lut=t, nclass=1, n_values=4, P=9) == 1
    assert gather(off=(5, 1, 1)) == 1 and gather(off=(-1, 1, 1)) == 1 and gather(box=(5, 6, 10)) == 1               # the box leaves the output
    assert gather(out=(2048, 1024, 1024), box=(5, 6, 7)) == 1                                                     # 2^31 voxels
    assert gather(dst=ctypes.c_void_p((1 << 20) + 100)) == 1                                                       # dst inside raw
    p = ctypes.c_void_p(1 << 20)
    bg = L.rsuper_label_background
    assert bg(None, 1, 0, 9, 9, 9, 1, 1, 1, 5, 6, 7, None) == 1 and bg(p, 0, 0, 9, 9, 9, 1, 1, 1, 5, 6, 7, None) == 1
    assert bg(p, 1, 8, 9, 9, 9, 1, 1, 1, 5, 6, 7, None) == 1 and bg(p, 1, -1, 9, 9, 9, 1, 1, 1, 5, 6, 7, None) == 1
    assert bg(p, 1, 0, 9, 9, 9, 5, 1, 1, 5, 6, 7, None) == 1 and bg(p, 9, 0, 9, 9, 9, 1, 1, 1, 5, 6, 7, None) == 1
    ws = L.rsuper_ct_stats_workspace_bytes()
    q = ctypes.c_void_p(8 << 20)
    pop = L.rsuper_ct_normalize_pop
    assert pop(p, 2, 4, 4, 4, -991.0, 500.0, q, ws - 8, dst, 4, 4, 4, 0, 0, 0, t, None) == 1                        # a short workspace
    assert pop(p, 2, 4, 4, 4, -991.0, 500.0, q, ws, dst, 4, 4, 3, 0, 0, 0, t, None) == 1                            # the box leaves the output
    assert pop(p, 0, 4, 4, 4, -991.0, 500.0, q, ws, dst, 4, 4, 4, 0, 0, 0, t, None) == 1                            # uint8 is no CT dtype


def test_cpu_tensors_are_refused():
    import torch
    from rsuper_amd.dataset_conversion import nii_dataset
    from rsuper_amd.hip.lib import RSuperHipError
    z = torch.zeros(4, dtype=torch.uint8)
    with pytest.raises(RSuperHipError):
        nii_dataset._label_background_impl(torch.zeros((1, 2, 2, 2), dtype=torch.uint8), 0, [0, 0, 0], [2, 2, 2])
    with pytest.raises(RSuperHipError):
        nii_dataset._label_gather_pack_impl(z, z, 1, None, z, z, z, [1, 1, 1], z, 0, [0, 0, 0])
    with pytest.raises(RSuperHipError):
        nii_dataset._ct_normalize_pop_impl(torch.zeros((2, 2, 2)), -991.0, 500.0, [2, 2, 2], [0, 0, 0])
    with pytest.raises(RSuperHipError):
        nii_dataset.convert_case('x.nii.gz', {}, ['liver'], device='cpu')
    assert set(nii_dataset.nii_dataset_launches()) == {'gather', 'background', 'normalize'}
