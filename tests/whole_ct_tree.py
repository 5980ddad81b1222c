"""A small, deterministic whole-CT dataset tree for the tests of training/dataset/whole_ct.py (and for tests/golden/gen_golden_whole_ct.py, which runs the
reference on the same tree): an annotated root with 6 cases + one image without its `_gt` file, a report root with 5 eligible cases (one of them an id
that the annotated root holds too) + one case the report cleaning drops, `list/label_names.yaml` in both, and the report table.  Labels are stored in
the three forms the dataset accepts: bit-packed .npy, unpacked int8 .npy, unpacked int8 .npz.

The image of a case is (1 + the voxel's linear index) * 2 ** -13: exact in float32, below 100, and a crop gives its own corner (`corner_of`).
"""
import os

import numpy as np

IMG_SCALE = 2.0 ** -13
TRAINING_SIZE = (24, 28, 32)
LARGE = tuple(t + m for t, m in zip(TRAINING_SIZE, (20, 40, 40)))
TUMOR_CLASSES = ['kidney']          # forg = kidney_left / kidney_right (in both class lists), lesion class = kidney_lesion

_LIVER = ['liver_segment_%d' % i for i in range(1, 9)]
CLASSES_UFO = sorted(['background'] + _LIVER + ['pancreas_head', 'pancreas_body', 'pancreas_tail', 'kidney_left', 'kidney_right', 'spleen', 'aorta',
                                                'stomach'])
CLASSES = sorted(CLASSES_UFO + ['liver', 'pancreas', 'liver_lesion', 'pancreatic_lesion', 'kidney_lesion', 'femur_left', 'femur_right',
                                'hepatic_vessel', 'portal_vein_and_splenic_vein'])
assert len(CLASSES) == 26 and len(CLASSES_UFO) == 17

# id -> (shape, stored form, has a kidney lesion)
ATLAS = {
    'BDMAP_00000001': ((40, 60, 60), 'npy_packed', True),
    'BDMAP_00000002': ((48, 70, 64), 'npy_unpacked', False),
    'BDMAP_00000003': ((64, 90, 96), 'npz_unpacked', True),
    'BDMAP_00000004': ((44, 68, 72), 'npy_packed', False),
    'BDMAP_00000005': ((50, 64, 80), 'npy_unpacked', True),
    'BDMAP_00000006': ((40, 72, 60), 'npz_unpacked', False),
}
ATLAS_WITHOUT_GT = 'BDMAP_00000007'
# id -> (shape, stored form, sides of the kidneys present)
UFO = {
    'BDMAP_00001001': ((40, 60, 60), 'npy_packed', ('left', 'right')),
    'BDMAP_00001002': ((52, 66, 70), 'npy_unpacked', ('left', 'right')),
    'BDMAP_00001003': ((46, 80, 64), 'npz_unpacked', ('left', 'right')),
    'BDMAP_00001004': ((42, 62, 90), 'npy_packed', ('right',)),          # the report names the left kidney: an empty segment mask
    'BDMAP_00000003': ((48, 64, 64), 'npy_unpacked', ('left', 'right')),  # also an annotated case
    'BDMAP_00001006': ((40, 60, 60), 'npy_packed', ('left', 'right')),   # 'multiple': dropped by the report cleaning
}
COLUMNS = ['BDMAP_ID', 'Standardized Organ', 'Standardized Location', 'Tumor Size (mm)', 'Unknow Tumor Size', 'no lesion']
REPORT_ROWS = [
    ['BDMAP_00001001', 'kidney', 'left', '12', 'no', 0],
    ['BDMAP_00001002', 'kidney', 'right', '10 x 8', 'no', 0],
    ['BDMAP_00001003', None, None, None, None, 1],
    ['BDMAP_00001004', 'kidney', 'left', '9', 'no', 0],
    ['BDMAP_00000003', 'kidney', 'right', '15 x 10 x 8', 'no', 0],
    ['BDMAP_00001006', 'kidney', 'left', 'multiple', 'no', 0],
    ['BDMAP_00009999', 'kidney', 'left', '7', 'no', 0],                  # no volume of this id
]
ELIGIBLE_UFO = sorted(['BDMAP_00001001', 'BDMAP_00001002', 'BDMAP_00001003', 'BDMAP_00001004', 'BDMAP_00000003'])


def image(shape):
    return ((1 + np.arange(int(np.prod(shape)), dtype=np.float64)) * IMG_SCALE).astype(np.float32).reshape(shape)


def corner_of(crop, full, size):
    """The corner (in coordinates of the volume padded to `full`) of an un-resampled crop of `image(size)`; crop (..., d, h, w)."""
    c = np.asarray(crop, np.float64).reshape(crop.shape[-3:])
    lo = [(f - s) // 2 for f, s in zip(full, size)]
    idx = np.argwhere(c != 0)
    assert len(idx), 'the crop lies in the padding'
    z, y, x = idx[0]
    lin = int(round(c[z, y, x] / IMG_SCALE)) - 1
    vz, r = divmod(lin, size[1] * size[2])
    vy, vx = divmod(r, size[2])
    return [int(vz + lo[0] - z), int(vy + lo[1] - y), int(vx + lo[2] - x)]


def padded(a, full):
    """pad_volume_pair: zeros on both sides, pad // 2 on the low side; a (..., D, H, W)."""
    size = a.shape[-3:]
    full = [max(f, s) for f, s in zip(full, size)]
    out = np.zeros(a.shape[:-3] + tuple(full), a.dtype)
    lo = [(f - s) // 2 for f, s in zip(full, size)]
    out[..., lo[0]:lo[0] + size[0], lo[1]:lo[1] + size[1], lo[2]:lo[2] + size[2]] = a
    return out


def _ell(shape, c, r):
    z, y, x = np.meshgrid(*(np.arange(s) for s in shape), indexing='ij')
    return ((z - c[0]) / r[0]) ** 2 + ((y - c[1]) / r[1]) ** 2 + ((x - c[2]) / r[2]) ** 2 < 1.0


def organs(shape, k, sides=('left', 'right')):
    """name -> bool mask; k shifts the organs a little from case to case."""
    D, H, W = shape
    o = {}
    if 'left' in sides:
        o['kidney_left'] = _ell(shape, (D // 2 + k % 3, H // 3, W // 4 + k % 5), (6, 7, 6))
    if 'right' in sides:
        o['kidney_right'] = _ell(shape, (D // 2 - k % 4, H // 3 + 2, 3 * W // 4 - k % 3), (6, 6, 7))
    o['spleen'] = _ell(shape, (D // 3, 2 * H // 3, W // 4), (5, 6, 6))
    o['pancreas_head'] = _ell(shape, (D // 2, H // 2, W // 2 - 5), (3, 4, 4))
    o['pancreas_body'] = _ell(shape, (D // 2, H // 2 + 3, W // 2 + 3), (3, 3, 5))
    o['liver_segment_1'] = _ell(shape, (2 * D // 3, 2 * H // 3, 2 * W // 3), (5, 7, 7))
    o['aorta'] = _ell(shape, (D // 2, H // 2 - 8, W // 2), (D // 2 - 2, 2, 2))
    return o


def atlas_label(name):
    shape, _, lesion = ATLAS[name]
    k = int(name[-2:])
    lab = np.zeros((len(CLASSES),) + shape, np.int8)
    o = organs(shape, k)
    o['liver'] = o['liver_segment_1']
    o['pancreas'] = o['pancreas_head'] | o['pancreas_body']
    if lesion:
        D, H, W = shape
        o['kidney_lesion'] = _ell(shape, (D // 2 + k % 3, H // 3, W // 4 + k % 5), (2, 3, 2))
    for n, m in o.items():
        lab[CLASSES.index(n)] = m
    return lab


def ufo_label(name):
    shape, _, sides = UFO[name]
    lab = np.zeros((len(CLASSES_UFO),) + shape, np.int8)
    for n, m in organs(shape, int(name[-2:]) + 1, sides).items():
        lab[CLASSES_UFO.index(n)] = m
    return lab


def _store(root, name, shape, form, lab):
    img = image(shape)
    if form.startswith('npz'):
        np.savez_compressed(os.path.join(root, name + '.npz'), img)
        np.savez_compressed(os.path.join(root, name + '_gt.npz'), lab)
    else:
        np.save(os.path.join(root, name + '.npy'), img)
        np.save(os.path.join(root, name + '_gt.npy'), np.packbits(lab.astype(bool), axis=0) if form == 'npy_packed' else lab)


def _names_yaml(root, names):
    os.makedirs(os.path.join(root, 'list'), exist_ok=True)
    with open(os.path.join(root, 'list', 'label_names.yaml'), 'w') as f:
        f.write(''.join('- %s\n' % n for n in reversed(names)))          # the dataset sorts them


def build(base):
    """Write the tree under `base` -> {'data_root', 'UFO_root', 'reports'}."""
    import pandas as pd
    data_root, ufo_root = os.path.join(base, 'atlas'), os.path.join(base, 'ufo')
    os.makedirs(data_root), os.makedirs(ufo_root)
    for name, (shape, form, _) in ATLAS.items():
        _store(data_root, name, shape, form, atlas_label(name))
    np.save(os.path.join(data_root, ATLAS_WITHOUT_GT + '.npy'), image((40, 60, 60)))
    for name, (shape, form, _) in UFO.items():
        _store(ufo_root, name, shape, form, ufo_label(name))
    _names_yaml(data_root, CLASSES)
    _names_yaml(ufo_root, CLASSES_UFO)
    reports = os.path.join(base, 'reports.csv')
    pd.DataFrame(REPORT_ROWS, columns=COLUMNS).to_csv(reports, index=False)
    return {'data_root': data_root, 'UFO_root': ufo_root, 'reports': reports}


def args_for(tree, **kw):
    import argparse
    a = argparse.Namespace(data_root=tree['data_root'], UFO_root=tree['UFO_root'], reports=tree['reports'], ucsf_ids=None,
                           training_size=list(TRAINING_SIZE), scale=0.3, rotate=45, translate=0.1, aug_device='cpu', proc_idx=0,
                           model_genesis_pretrain=False, no_pancreas_subseg=False, pancreas_only=False, num_workers=0)
    for k, v in kw.items():
        setattr(a, k, v)
    return a


# The report table of the clean_ufo / normalize_no_lesion parity test: every rule of the cleaning is hit (see the comments).
def clean_table():
    import pandas as pd
    nan = float('nan')
    rows = []

    def add(i, organ, loc, size, unk='no', nl=0):
        rows.append(['BDMAP_%08d' % i, organ, loc, size, unk, nl])
    add(1, 'kidney', 'left', '12')
    add(2, 'kidney', 'right upper', '10 x 8')
    add(3, 'kidney', 'u', '9')                           # a sided organ without a side: the case goes
    add(4, 'kidney', 'Left', '9')                        # passes the case-blind rule, fails the case-sensitive one: no row of interest
    add(5, 'pancreas', 'head', '0.0 x 3')                # an extraction artefact: the case goes
    add(5, 'pancreas', 'tail', '14')
    add(6, 'pancreas', 'body', '0')
    add(7, 'pancreas', 'head', 'u')                      # no digit
    add(8, 'pancreas', 'head', 'multiple')
    add(9, 'pancreas', 'head / body', '20', unk='yes')   # size marked unknown
    add(10, 'pancreas', 'tail', '11 x 7 x 5')
    add(10, 'liver', 'segment 4', 'u')                   # an organ outside annotated_tumors: the row goes, the case stays
    add(11, 'liver', 'segment 2', '30')                  # only rows of other organs: nothing left
    add(12, 'adrenal_gland', 'gland', '8')               # sided organ outside annotated_tumors: dropped with rule 2 before the side rule
    add(13, 'adrenal_gland', 'left', '8')
    add(14, 'pancreas', 'head', '13', unk=' No ')        # passes the case rule ('no' after strip / lower), fails `== 'no'`
    add(15, 'pancreas', nan, '16')
    add(16, 'kidney', 'right', '0.0')
    add(17, 'pancreas', 'body', '18 x 12')
    add(17, 'kidney', 'left', '6')
    for j, nl in enumerate([1, 1.0, '1', '1.0', 'True', 'yes', ' Y ', True, 1, 1, 1, 1, 1, 1]):     # healthy, spelled in many ways
        add(20 + j, nan, nan, nan, nan, nl)
    for j, nl in enumerate([nan, 0, 'no', 'maybe', '2']):                                     # not healthy and no organ of interest: dropped
        add(40 + j, nan, nan, nan, nan, nl)
    return pd.DataFrame(rows, columns=COLUMNS)


CLEAN_TUMORS = [['kidney', 'pancreas'], ['kidney'], ['pancreas', 'adrenal_gland']]
