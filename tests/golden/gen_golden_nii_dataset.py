"""Writes tests/golden/nii_dataset.npz and nii_dataset.json by running the UNMODIFIED reference's dataset_conversion/nii2npz.py `process_file` and
`pad` on one case.  `sys.modules['SimpleITK']` is a stub whose ReadImage / GetArrayFromImage serve arrays from a dict keyed by path, so the
reference reads "files" that exist only in memory; its np.savez_compressed outputs land in a temporary directory and are read back.

    the case   1 mm, (Z, Y, X) = (20, 127, 128): one axis far below 128, one at 127 (-> 129), one at 128 (no pad).  Three classes: `background`
               (no file: process_file makes it as 1 - sum), `liver` and `liver_lesion`, which overlap.  The image takes few distinct HU values (blocks),
               some below -991 and some above 500, so the compressed fixture stays small.
    img        the int16 canonical image; liver, liver_lesion: the masks, np.packbits of the flat volume
    ref_img    the reference's float32 image (clip, np.mean / np.std in float32, pad)
    ref_lab    the reference's int8 (3, 128, 129, 128) stack as the dataset packs it: np.packbits(stack.astype(bool), axis=0)
    ref_bkg_values   the distinct values of the reference's background plane before astype(bool): -1 on the overlap, 0 inside one class, 1 elsewhere

The .json holds data read off the reference, no program text: the distance between ref_img and the float64 restatement (tests/nii_dataset_ref.py),
the flags and defaults of the two reference parsers (taken from the add_argument calls in their syntax trees), and the nnU-Net name -> value(s)
table that abdomenatlas_3d.py builds in its main block (those statements are executed as they stand).
Run from the repository root: python tests/golden/gen_golden_nii_dataset.py
"""
import ast
import importlib
import json
import os
import sys
import tempfile
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as gg  # noqa: E402
import nii_dataset_ref as ndr  # noqa: E402

SHAPE = (20, 127, 128)
NAMES = ['background', 'liver', 'liver_lesion']
PALETTE = np.array([-1024, -1000, -200, 40, 300, 1200], np.int16)
CONV = os.path.join(gg.REF, 'dataset_conversion')


def case():
    Z, Y, X = SHAPE
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    img = PALETTE[(zz // 5 + yy // 16 + 2 * (xx // 16)) % len(PALETTE)]
    liver = ((zz >= 3) & (zz < 15) & (yy >= 20) & (yy < 90) & (xx >= 30) & (xx < 100)).astype(np.uint8)
    lesion = ((zz >= 10) & (zz < 18) & (yy >= 70) & (yy < 110) & (xx >= 80) & (xx < 120)).astype(np.uint8)     # partly inside the liver, partly outside
    return img, liver, lesion


def run_reference(img, masks):
    store = {}
    sitk = types.ModuleType('SimpleITK')
    sitk.ReadImage = lambda path: path
    sitk.GetArrayFromImage = lambda key: store[key]
    sys.modules['SimpleITK'] = sitk
    sys.modules.setdefault('tqdm', types.SimpleNamespace(tqdm=lambda it, **k: it))
    sys.path.insert(0, CONV)
    n2n = importlib.import_module('nii2npz')
    with tempfile.TemporaryDirectory() as tmp:
        src, tgt = os.path.join(tmp, 'src'), os.path.join(tmp, 'tgt')
        os.makedirs(tgt)
        name = 'BDMAP_00000001.nii.gz'
        store[os.path.join(src, name)] = img
        for k, m in masks.items():
            store[os.path.join(src, name.replace('.nii.gz', ''), k + '.nii.gz')] = m
        n2n.lab_name_list = list(NAMES)
        assert n2n.process_file((name, src, tgt, 'ct')) == name, 'the reference did not process the case'
        out_img = np.load(os.path.join(tgt, 'BDMAP_00000001.npz'))['arr_0']
        out_lab = np.load(os.path.join(tgt, 'BDMAP_00000001_gt.npz'))['arr_0']
    # pad on its own, on an array with no short axis and one with all three short
    a, b = n2n.pad(np.ones((128, 130, 128), np.float32), np.ones((2, 128, 130, 128), np.int8))
    assert a.shape == (128, 130, 128) and b.shape == (2, 128, 130, 128)
    a, b = n2n.pad(np.ones((127, 20, 1), np.float32), np.ones((1, 127, 20, 1), np.int8))
    assert a.shape == (129, 128, 129) and b.shape == (1, 129, 128, 129)
    return out_img, out_lab


def parser_flags(path):
    """{flag: default} of every parser.add_argument call of a script ('store_true' flags default to False, a missing default is None)."""
    flags = {}
    for node in ast.walk(ast.parse(open(path).read())):
        if isinstance(node, ast.Call) and isinstance(node.func, ast.Attribute) and node.func.attr == 'add_argument':
            kw = {k.arg: ast.literal_eval(k.value) for k in node.keywords if k.arg in ('default', 'action')}
            flags[ast.literal_eval(node.args[0])] = False if kw.get('action') == 'store_true' else kw.get('default')
    return flags


def nnunet_table():
    """labels_nnunet as abdomenatlas_3d.py's main block builds it: the statements that define it, executed unchanged."""
    tree = ast.parse(open(os.path.join(CONV, 'abdomenatlas_3d.py')).read())
    main = [n for n in tree.body if isinstance(n, ast.If) and 'nnunet_labels_saved' in ast.dump(n)][0]
    wanted = ('nnunet_labels_saved', 'joint_labels_nnunet', 'names_labels_nnunet', 'tmp', 'labels_nnunet')
    keep = []
    for st in main.body:
        if isinstance(st, ast.Assign) and isinstance(st.targets[0], ast.Name) and st.targets[0].id in wanted:
            keep.append(st)
        elif isinstance(st, ast.For) and isinstance(st.iter, ast.Name) and st.iter.id == 'names_labels_nnunet':
            keep.append(st)
    ns = {}
    exec(compile(ast.Module(body=keep, type_ignores=[]), 'abdomenatlas_3d.py', 'exec'), ns)
    return {k: ns['labels_nnunet'][k] for k in sorted(ns['labels_nnunet'])}


def main():
    img, liver, lesion = case()
    ref_img, ref_lab = run_reference(img, {'liver': liver, 'liver_lesion': lesion})
    assert ref_img.dtype == np.float32 and ref_img.shape == (128, 129, 128) and ref_lab.dtype == np.int8 and ref_lab.shape == (3, 128, 129, 128)
    exact = ndr.zscore(img, 128, ddof=0)
    dist = float(np.abs(ref_img.astype(np.float64) - exact).max())
    dist1 = float(np.abs(ref_img.astype(np.float64) - ndr.zscore(img, 128, ddof=1)).max())
    bkg = ref_lab[0]
    out = dict(img=img, liver=np.packbits(liver.reshape(-1)), liver_lesion=np.packbits(lesion.reshape(-1)), ref_img=ref_img,
               ref_lab=np.packbits(ref_lab.astype(bool), axis=0), ref_bkg_values=np.unique(bkg).astype(np.int64))
    path = os.path.join(HERE, 'nii_dataset.npz')
    np.savez_compressed(path, **out)
    meta = dict(shape=list(SHAPE), class_names=NAMES, padded_shape=list(ref_img.shape), ref_vs_float64=dist, ref_vs_float64_ddof1=dist1,
                parsers=dict(abdomenatlas_3d=parser_flags(os.path.join(CONV, 'abdomenatlas_3d.py')), nii2npz=parser_flags(os.path.join(CONV, 'nii2npz.py'))),
                nnunet_labels=nnunet_table())
    with open(os.path.join(HERE, 'nii_dataset.json'), 'w') as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write('\n')
    print(f'wrote {path}: {os.path.getsize(path)} bytes; reference float32 image vs float64 restatement (ddof = 0): {dist:.3e} (ddof = 1: {dist1:.3e}); '
          f'background values {np.unique(bkg).tolist()}')


if __name__ == '__main__':
    main()
