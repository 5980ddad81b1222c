"""numpy restatement of the test flow's measurement (rsuper_train/test_with_reports.py detection :56-94 and the rows of _process_single_file), the
yardstick of tests/test_test_flow_cpu.py and tests/test_gpu_test_flow.py.  No scipy: ndimage.zoom(order=0), binary_erosion and binary_dilation with
a 3x3x3 box are written out; tests/golden/gen_golden_test_flow.py checks this file against scipy and the reference on every fixture case."""
import numpy as np

SUFFIXES = (('_lesion', 'tumor'), ('_pdac', 'pdac'), ('_pnet', 'pnet'), ('_cyst', 'cyst'))


def zoom_shape(shape, factors):
    return tuple(int(round(float(n) * float(f))) for n, f in zip(shape, factors))


def nearest_axis(n_in, n_out, clamp=False):
    """(source index per output index, valid): floor(c + 0.5) of c = o * (n_in - 1) / (n_out - 1) in f64; invalid (the constant 0) where
    c > n_in - 1.  clamp=True is the rule scipy does NOT follow (last voxel instead of the constant), kept to show that a case tells them apart."""
    s = (n_in - 1) / (n_out - 1) if n_out > 1 else 0.0
    c = np.arange(n_out, dtype=np.float64) * np.float64(s)
    over = c > n_in - 1
    idx = np.minimum(np.floor(c + 0.5).astype(np.int64), n_in - 1)
    return idx, (np.ones(n_out, bool) if clamp else ~over)


def zoom0(m, out_shape, clamp=False):
    """ndimage.zoom(m, f, order=0) of a bool volume onto out_shape."""
    ax = [nearest_axis(n, o, clamp) for n, o in zip(m.shape, out_shape)]
    out = m[np.ix_(ax[0][0], ax[1][0], ax[2][0])]
    valid = ax[0][1][:, None, None] & ax[1][1][None, :, None] & ax[2][1][None, None, :]
    return out & valid


def _box3(m, op):
    """op = np.logical_and: erosion (border value 0); np.logical_or: dilation."""
    out = m
    for axis in range(3):
        p = np.pad(out, [(1, 1) if a == axis else (0, 0) for a in range(3)], constant_values=False)
        n = out.shape[axis]
        sl = [np.take(p, np.arange(k, k + n), axis=axis) for k in range(3)]
        out = op(op(sl[0], sl[1]), sl[2])
    return out


def detection_binary(array, spacing=(1, 1, 1), th=0.5, erode=True, clamp=False):
    m = np.asarray(array).astype(np.float64) > th
    z = zoom0(m, zoom_shape(m.shape, spacing), clamp)
    if erode:
        a = _box3(z, np.logical_and)
        a = _box3(_box3(a, np.logical_or), np.logical_or)
        z = a & z
    return int(z.sum())


def column_name(cls):
    for suffix, word in SUFFIXES:
        if cls.endswith(suffix):
            return f'{cls[:-len(suffix)]} {word} volume predicted'
    return None


def normalize_id(name):
    return name.replace('_0000.', '.').replace('.nii.gz', '')


def row(case, planes, spacing=(1, 1, 1), th=0.5):
    """The CSV row of a case from {class: host array}."""
    out = {'BDMAP_ID': normalize_id(case)}
    for cls, a in planes.items():
        if column_name(cls) is not None:
            out[column_name(cls)] = detection_binary(a, spacing, th, True)
    return out
