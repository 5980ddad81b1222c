"""The host half of the NIfTI front end (inference/nifti.py) against the tests' own header writer / parser (tests/nifti_ref.py) and hand-worked
table values; the command-line flag and the C ABI of the three device entry points.  No device is needed."""
import ctypes
import inspect
import math
import os
import re
import struct

import numpy as np
import pytest

import nifti_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NP_OF = {2: np.uint8, 256: np.int8, 4: np.int16, 512: np.uint16, 8: np.int32, 16: np.float32, 64: np.float64}


def _ramp(shape=(5, 7, 9)):
    """Every voxel its own value: i + 10 j + 100 k."""
    i, j, k = np.meshgrid(*[np.arange(n) for n in shape], indexing='ij')
    return i + 10 * j + 100 * k


@pytest.mark.parametrize('datatype', sorted(NP_OF))
@pytest.mark.parametrize('bo', ['<', '>'])
@pytest.mark.parametrize('ext', ['.nii', '.nii.gz'])
def test_header_round_trip_every_dtype_byte_order_and_container(tmp_path, datatype, bo, ext):
    from rsuper_amd.inference import nifti as N
    arr = (_ramp() % 120).astype(NP_OF[datatype])
    A = R.affine_for((1, 0, 2), (True, False, True), (0.75, 0.5, 2.5), origin=(10.0, -20.0, 30.0))
    path = tmp_path / ('x' + ext)
    R.write_nifti(path, arr, datatype, (0.75, 0.5, 2.5), bo=bo, slope=2.5, inter=-1024.0, sform=A)
    v = N.read_nifti(path)
    assert v.shape == (5, 7, 9) and v.datatype == datatype and v.vox_offset == 352
    assert v.data.dtype == (np.float32 if datatype == 64 else NP_OF[datatype]) and v.data.dtype.isnative and v.data.flags['C_CONTIGUOUS']
    assert np.array_equal(v.data, R.file_order(arr).astype(v.data.dtype))             # file order, nothing permuted
    assert v.pixdim == (0.75, 0.5, 2.5) and (v.scl_slope, v.scl_inter) == (2.5, -1024.0)
    assert (v.qform_code, v.sform_code) == (0, 1)
    assert np.array_equal(N.affine(v), A.astype(np.float32).astype(np.float64))


def test_sform_qform_and_neither(tmp_path):
    from rsuper_amd.inference import nifti as N
    arr = _ramp().astype(np.int16)
    pix = (0.8, 0.8, 2.5)
    # qform only, left-handed (qfac = -1): the LAS scan of the device tests
    A = R.affine_for((0, 1, 2), (False, True, False), pix, origin=(3.0, 4.0, 5.0))
    b, c, d, qfac, qpix = R.qform_of(A)
    assert qfac == -1.0 and np.allclose(qpix, pix)
    R.write_nifti(tmp_path / 'q.nii', arr, 4, pix, qform=(b, c, d, qfac), qoffset=(3.0, 4.0, 5.0))
    v = N.read_nifti(tmp_path / 'q.nii')
    assert (v.qform_code, v.sform_code, v.qfac) == (1, 0, -1.0)
    assert np.allclose(N.affine(v), A, atol=1e-6)
    assert N.orientation_plan(N.affine(v)) == ((0, 1, 2), (False, True, False))
    # both: the sform wins
    S = R.affine_for((2, 0, 1), (False, False, True), pix)
    R.write_nifti(tmp_path / 'b.nii', arr, 4, pix, qform=(b, c, d, qfac), sform=S)
    assert np.allclose(N.affine(N.read_nifti(tmp_path / 'b.nii')), S, atol=1e-6)
    # neither: diag(pixdim); slope 0 is kept as the header has it ("no scaling" is the caller's reading)
    R.write_nifti(tmp_path / 'n.nii', arr, 4, pix)
    v = N.read_nifti(tmp_path / 'n.nii')
    assert np.allclose(N.affine(v), np.diag(pix + (1.0,)), atol=1e-7) and v.scl_slope == 0.0
    # a 4-D file with one volume reads as 3-D
    R.write_nifti(tmp_path / 'd4.nii', arr, 4, pix, dim0=4, dim4=1)
    assert N.read_nifti(tmp_path / 'd4.nii').shape == (5, 7, 9)


def test_error_cases_name_the_file(tmp_path):
    from rsuper_amd.inference import nifti as N
    arr = _ramp().astype(np.int16)
    pix = (1.0, 1.0, 1.0)
    (tmp_path / 'two.nii').write_bytes(struct.pack('<i', 540) + b'n+2\x00\r\n\x1a\n' + bytes(540 - 12))
    R.write_nifti(tmp_path / 'four.nii', arr, 4, pix, dim0=4, dim4=2)
    R.write_nifti(tmp_path / 'short.nii.gz', arr, 4, pix, truncate=7)
    R.write_nifti(tmp_path / 'analyze.nii', arr, 4, pix, magic=b'\x00\x00\x00\x00')
    R.write_nifti(tmp_path / 'pair.nii', arr, 4, pix, magic=b'ni1\x00')
    R.write_nifti(tmp_path / 'cplx.nii', arr.astype(np.float32), 16, pix)
    raw = bytearray((tmp_path / 'cplx.nii').read_bytes())
    struct.pack_into('<h', raw, 70, 32)                              # complex64
    (tmp_path / 'cplx.nii').write_bytes(bytes(raw))
    R.write_nifti(tmp_path / 'cut.nii.gz', arr, 4, pix)
    gz = (tmp_path / 'cut.nii.gz').read_bytes()
    (tmp_path / 'cut.nii.gz').write_bytes(gz[:len(gz) // 2])       # a gzip stream that ends early
    for name, word in (('two.nii', 'NIfTI-2'), ('four.nii', 'dim'), ('short.nii.gz', 'truncated'), ('analyze.nii', 'Analyze'), ('pair.nii', 'two-file'),
                       ('cplx.nii', 'datatype'), ('cut.nii.gz', 'cut.nii.gz')):
        with pytest.raises(ValueError, match=word) as e:
            N.read_nifti(tmp_path / name)
        assert name in str(e.value)


def test_orientation_plan_all_48_orientations_give_the_canonical_array():
    from rsuper_amd.inference import nifti as N
    canon = np.arange(5 * 7 * 9).reshape(9, 7, 5)                    # canonical (Z, Y, X) ramp: X = 5, Y = 7, Z = 9
    assert len(R.ORIENTATIONS) == 48
    for perm, flip in R.ORIENTATIONS:
        arr = R.inverse_reorient(canon, perm, flip)                 # the same anatomy stored in this orientation
        pix = tuple((0.7, 0.8, 2.5)[perm[a]] for a in range(3))
        A = R.affine_for(perm, flip, pix)
        assert N.orientation_plan(A) == (perm, flip)
        assert np.array_equal(R.reorient(arr, perm, flip), canon)
        # the strided view of the flat file buffer that the device kernel reads
        size, stride, offset, inv = N.canonical_layout(arr.shape, perm, flip)
        assert size == (5, 7, 9) and tuple(pix[a] for a in inv) == (0.7, 0.8, 2.5)
        flat = R.file_order(arr)
        z, y, x = np.meshgrid(np.arange(9), np.arange(7), np.arange(5), indexing='ij')
        assert np.array_equal(flat[offset + z * stride[2] + y * stride[1] + x * stride[0]], canon)


def test_orientation_plan_names_the_axes_as_the_reference_does():
    """RAS+ identity (nibabel 'RAS') is ITK 'LPI': both in-plane axes are flipped to reach 'RAI'; an 'LPS' file is canonical as it is."""
    from rsuper_amd.inference import nifti as N
    assert N.orientation_plan(np.eye(4)) == ((0, 1, 2), (True, True, False))
    assert N.orientation_plan(np.diag([-1.0, -1.0, 1.0, 1.0])) == ((0, 1, 2), (False, False, False))
    assert N.orientation_plan(np.diag([-0.8, 0.8, 2.5, 1.0])) == ((0, 1, 2), (False, True, False))          # 'LAS'
    assert 'LEFT' in N.orientation_plan.__doc__.upper() + N.__doc__.upper() and "('L', 'P', 'S')" in N.orientation_plan.__doc__


def test_orientation_plan_oblique_and_tie():
    from rsuper_amd.inference import nifti as N

    def rot_z(deg):
        c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        return np.array([[c, -s, 0, 0], [s, c, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1.0]])

    base = R.affine_for((1, 0, 2), (False, True, False), (0.7, 0.7, 3.0))
    assert N.orientation_plan(rot_z(10.0) @ base) == ((1, 0, 2), (False, True, False))
    assert N.orientation_plan(rot_z(-10.0) @ base) == ((1, 0, 2), (False, True, False))
    with pytest.raises(ValueError, match='equally'):
        N.orientation_plan(rot_z(45.0) @ base)
    shear = np.eye(4)
    shear[:3, :3] = [[1.0, 0.9, 0.0], [0.2, 0.3, 0.0], [0.0, 0.0, 1.0]]      # i and j both lie mostly along world x
    with pytest.raises(ValueError, match='permutation'):
        N.orientation_plan(shear)


def test_resample_axis_table_hand_worked_values():
    from rsuper_amd.inference import nifti as N
    # n_in = 10, 1.5 -> 1.0 mm: 15 outputs at pos = o / 1.5.  The last, o = 14, sits at 9.333 < 9.5: inside, so this axis has no outside index
    # (the first one would be o = 15 = n_out).  Its taps are floor(9.333) - 1 ... + 2 = 8, 9, 10, 11 -> mirrored 8, 9, 8, 7.
    idx, w = N.resample_axis_table(10, 1.5, 1.0, 'bspline')
    assert idx.shape == w.shape == (15, 4) and idx.dtype == np.int32 and w.dtype == np.float32
    assert (idx[:, 0] >= 0).all() and idx[14].tolist() == [8, 9, 8, 7] and idx[0].tolist() == [1, 0, 1, 2]
    t = 14 / 1.5 - 9
    assert np.allclose(w[14], [(1 - t) ** 3 / 6, (3 * t ** 3 - 6 * t ** 2 + 4) / 6, (-3 * t ** 3 + 3 * t ** 2 + 3 * t + 1) / 6, t ** 3 / 6], atol=1e-7)
    assert w[0].tolist() == [np.float32(1 / 6), np.float32(4 / 6), np.float32(1 / 6), 0.0]
    # n_in = 9 at 1.5 -> 1.0: 13.5 rounds (half to even) to 14 outputs, and o = 13 sits at 8.667 >= 8.5: the far-edge stripe
    idx, w = N.resample_axis_table(9, 1.5, 1.0, 'bspline')
    assert idx.shape == (14, 4) and idx[13].tolist() == [N.OUTSIDE] * 4 and w[13].tolist() == [0.0] * 4 and (idx[:13] >= 0).all()
    # n_in = 10 at 2.5 -> 1.0: 25 outputs, o = 24 sits at 9.6 >= 9.5: outside; o = 23 at 9.2 -> nearest 9
    nz = N.resample_axis_table(10, 2.5, 1.0, 'nearest')
    assert nz.dtype == np.int32 and nz.shape == (25,) and nz[24] == N.OUTSIDE and nz[23] == 9 and nz[:3].tolist() == [0, 0, 1]
    # a position of exactly k + 0.5 rounds up: 2.0 -> 1.0 puts o = 1, 3, 5 at 0.5, 1.5, 2.5
    assert N.resample_axis_table(4, 2.0, 1.0, 'nearest').tolist() == [0, 1, 1, 2, 2, 3, 3, N.OUTSIDE]
    # down-sampling 0.625 -> 1.0: pos = 1.6 o
    assert N.resample_axis_table(8, 0.625, 1.0, 'nearest').tolist() == [0, 2, 3, 5, 6]
    # n_in = 1, 2, 3
    idx, w = N.resample_axis_table(1, 1.5, 1.0, 'bspline')
    assert idx.tolist() == [[0, 0, 0, 0], [N.OUTSIDE] * 4]           # o = 1 sits at 0.667 >= 0.5
    idx, w = N.resample_axis_table(2, 1.5, 1.0, 'bspline')
    assert idx.tolist() == [[1, 0, 1, 0], [1, 0, 1, 0], [0, 1, 0, 1]]
    idx, w = N.resample_axis_table(3, 1.0, 1.0, 'bspline')
    assert idx.tolist() == [[1, 0, 1, 2], [0, 1, 2, 1], [1, 2, 1, 0]]
    assert np.array_equal(w, np.tile(np.array([1 / 6, 4 / 6, 1 / 6, 0], dtype=np.float32), (3, 1)))
    # the four weights sum to 1, and the tables agree with the reference's positions on every axis the device tests use
    for n_in, sp in ((29, 0.8203), (37, 1.5), (200, 0.8203), (130, 1.5), (67, 1.0), (2, 0.8203), (5, 2.5), (14, 0.625)):
        idx, w = N.resample_axis_table(n_in, sp, 1.0, 'bspline')
        pos, inside = R.positions(n_in, sp, 1.0)
        assert len(idx) == R.out_size(n_in, sp, 1.0) and np.array_equal(idx[:, 0] >= 0, inside)
        assert np.abs(w[inside].astype(np.float64).sum(1) - 1.0).max() < 2e-7
        assert idx[inside].min() >= 0 and idx[inside].max() < n_in
        assert np.array_equal(N.resample_axis_table(n_in, sp, 1.0, 'nearest'), R.nearest_table(n_in, sp, 1.0))
    with pytest.raises(ValueError):
        N.resample_axis_table(10, 1.0, 1.0, 'linear')


def test_prefilter_recursion_reproduces_scipy():
    """The recursion the kernels run (tests/nifti_ref.prefilter_line, float64) is scipy's spline_filter(order=3, mode='mirror')."""
    from scipy import ndimage
    rng = np.random.default_rng(5)
    for n in (1, 2, 3, 4, 17, 200):
        s = rng.uniform(-1024, 3071, size=n)
        assert np.abs(R.prefilter_line(s) - ndimage.spline_filter1d(s, order=3, mode='mirror')).max() < 1e-9
    from rsuper_amd.inference import nifti as N
    assert N.Z1 == math.sqrt(3.0) - 2.0 and abs(N.Z1) ** 16 < 2.0 ** -30 < abs(N.Z1) ** 15


def test_product_header_parsed_by_the_tests_parser():
    from rsuper_amd.inference import nifti as N
    for perm, flip in (((0, 1, 2), (False, True, False)), ((2, 0, 1), (True, False, True)), ((1, 2, 0), (False, False, False))):
        A = R.affine_for(perm, flip, (0.8, 0.75, 2.5), origin=(-100.5, 20.25, 7.0))
        raw = N.nifti1_header((40, 36, 14), (0.8, 0.75, 2.5), A, 2)
        assert len(raw) == 352
        h = R.parse_header(raw)
        assert h['dim'] == (3, 40, 36, 14, 1, 1, 1, 1) and (h['datatype'], h['bitpix']) == (2, 8) and h['vox_offset'] == 352.0
        assert h['pixdim'][1:4] == (np.float32(0.8), 0.75, 2.5) and h['extension'] == b'\x00\x00\x00\x00'
        assert h['qform_code'] > 0 and h['sform_code'] > 0 and (h['slope'], h['inter']) == (1.0, 0.0)
        assert np.array_equal(h['srow'], A[:3].astype(np.float32).astype(np.float64))
        assert np.allclose(R.quaternion_affine(h), A, atol=1e-5)             # the qform says the same as the sform
    with pytest.raises(ValueError):
        N.nifti1_header((2, 2, 2), (1, 1, 1), np.eye(4), 32)


def test_cli_flag_parses_and_is_off_by_default(tmp_path):
    from rsuper_amd import predict_abdomenatlas as P
    cl = tmp_path / 'classes.yaml'
    cl.write_text('[liver]\n')
    argv = ['--load', str(tmp_path / 'run' / 'a.pth'), '--img_path', str(tmp_path / 'img'), '--class_list', str(cl), '--save_path', str(tmp_path / 'res')]
    assert P.get_parser(argv).nifti is False and P.get_parser(argv + ['--nifti']).nifti is True
    os.makedirs(tmp_path / 'img' / 'BDMAP_2')
    (tmp_path / 'img' / 'BDMAP_1.nii.gz').write_bytes(b'')
    (tmp_path / 'img' / 'BDMAP_2' / 'ct.nii.gz').write_bytes(b'')
    (tmp_path / 'img' / 'BDMAP_3.npy').write_bytes(b'')
    args = P.get_parser(argv + ['--nifti'])
    assert P.list_ids(args) == ['BDMAP_1.nii.gz', 'BDMAP_2/ct.nii.gz', 'BDMAP_3.npy']
    with pytest.raises(ValueError, match='INTEGRATION section 3b'):           # without the flag nothing changes
        P.list_ids(P.get_parser(argv))
    args.predict_pancreas_only = True
    with pytest.raises(ValueError, match='You cannot predict only pancreas with nii.gz files'):
        P.load_case(args, 'BDMAP_1.nii.gz', ['liver'])
    args.predict_pancreas_only = False
    with pytest.raises(ValueError, match='BDMAP_1.nii.gz'):                   # the empty file is no NIfTI: the reader names it
        P.load_case(args, 'BDMAP_1.nii.gz', ['liver'])
    # the already-predicted filter looks for .nii.gz masks of a NIfTI case
    os.makedirs(tmp_path / 'save' / 'BDMAP_1' / 'predictions')
    (tmp_path / 'save' / 'BDMAP_1' / 'predictions' / 'liver.nii.gz').write_bytes(b'')
    assert P.filter_already_predicted(['BDMAP_1.nii.gz', 'BDMAP_2/ct.nii.gz'], str(tmp_path / 'save'), ['liver'], False) == ['BDMAP_2/ct.nii.gz']


def test_symbols_declared_bound_exported_with_matching_arity():
    from rsuper_amd.hip import lib, library
    hdr = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'rsuper_hip.h')).read(), flags=re.S)
    for name, arity in (('rsuper_nifti_load_prefilter', 15), ('rsuper_bspline_resample', 15), ('rsuper_reorient_store', 17)):
        m = re.search(r'int %s\(([^)]*)\)' % name, hdr)
        assert m, f'{name} is not declared in include/rsuper_hip.h'
        res, argtypes = lib._SIGS[name]
        assert res is ctypes.c_int and len(argtypes) == len(m.group(1).split(',')) == arity
        assert name in lib.exported_symbols() and hasattr(lib.lib(), name)
    assert lib._SIGS['rsuper_nifti_load_prefilter'][1][10] is ctypes.c_float and lib._SIGS['rsuper_bspline_resample'][1][13] is ctypes.c_float
    for code, name in enumerate(('U8', 'I8', 'I16', 'U16', 'I32', 'F32')):
        assert re.search(r'#define RSUPER_NII_%s %d\b' % (name, code), hdr)
    assert list(inspect.signature(library.install_nifti_ops).parameters) == ['load_prefilter', 'bspline_resample', 'reorient_store']


def test_entry_points_refuse_bad_arguments_before_any_launch():
    """Every call below is refused on the host side of the C ABI: the pointers are never dereferenced and no device is needed."""
    from rsuper_amd.hip import lib
    L = lib.lib()
    p, q = ctypes.c_void_p(4096), ctypes.c_void_p(1 << 20)
    ok = dict(n=5 * 7 * 9, Z=9, Y=7, X=5)
    assert L.rsuper_nifti_load_prefilter(p, 2, ok['n'], 9, 7, 4097, 35, 5, 1, 0, 1.0, 0.0, 1, q, None) == 3            # a side above 4096: UNSUPPORTED
    assert L.rsuper_nifti_load_prefilter(p, 2, ok['n'], 9, 7, 5, 35, 5, 1, 1, 1.0, 0.0, 1, q, None) == 1               # the last voxel leaves the buffer
    assert L.rsuper_nifti_load_prefilter(p, 2, ok['n'], 9, 7, 5, 35, 5, -1, 0, 1.0, 0.0, 1, q, None) == 1              # a flip without its offset
    assert L.rsuper_nifti_load_prefilter(p, 6, ok['n'], 9, 7, 5, 35, 5, 1, 0, 1.0, 0.0, 1, q, None) == 1               # unknown dtype
    assert L.rsuper_nifti_load_prefilter(p, 2, ok['n'], 9, 7, 5, 35, 5, 1, 0, 1.0, 0.0, 1, p, None) == 1               # in place
    assert L.rsuper_nifti_load_prefilter(None, 2, ok['n'], 9, 7, 5, 35, 5, 1, 0, 1.0, 0.0, 1, q, None) == 1
    assert L.rsuper_bspline_resample(p, 9, 7, 5, p, p, p, p, p, q, 70000, 7, 5, 0.0, None) == 3                       # more output slices than a grid holds
    assert L.rsuper_bspline_resample(p, 9, 7, 5, p, p, p, p, None, q, 9, 7, 5, 0.0, None) == 1
    assert L.rsuper_bspline_resample(p, 9, 7, 5, p, p, p, p, p, p, 9, 7, 5, 0.0, None) == 1
    n = ok['n']
    assert L.rsuper_reorient_store(p, 3, 9, 7, 5, q, 3 * (352 + n) - 1, 352, 352 + n, 5, 7, 9, 1, 5, 35, 0, None) == 1   # the last plane leaves dst
    assert L.rsuper_reorient_store(p, 3, 9, 7, 5, q, 3 * (352 + n), 352, 352 + n, 5, 7, 8, 1, 5, 35, 0, None) == 1       # another voxel count
    assert L.rsuper_reorient_store(p, 3, 9, 7, 5, q, 3 * (352 + n), 352, 352 + n, 5, 7, 9, -1, 5, 35, 0, None) == 1      # a flip without its offset
    assert L.rsuper_reorient_store(p, 3, 9, 7, 5, p, 3 * (352 + n), 352, 352 + n, 5, 7, 9, 1, 5, 35, 0, None) == 1       # overlapping buffers
    assert L.rsuper_reorient_store(p, 0, 9, 7, 5, q, 3 * (352 + n), 352, 352 + n, 5, 7, 9, 1, 5, 35, 0, None) == 1


def test_device_entry_points_refuse_host_tensors():
    import torch
    from rsuper_amd.hip import lib
    from rsuper_amd.inference import nifti_device as D
    with pytest.raises(lib.RSuperHipError):
        D._load_prefilter_impl(torch.zeros(8, dtype=torch.uint8), 0, [2, 2, 2], [4, 2, 1], 0, 1.0, 0.0, False)
    with pytest.raises(lib.RSuperHipError):
        D._bspline_resample_impl(torch.zeros(2, 2, 2), *[torch.zeros(2, 4, dtype=torch.int32)] * 5, 0.0)
    with pytest.raises(lib.RSuperHipError):
        D._reorient_store_impl(torch.zeros(1, 2, 2, 2, dtype=torch.uint8), torch.zeros(400, dtype=torch.uint8), 352, 360, [2, 2, 2], [1, 2, 4], 0)
    # the reference's spacing test compares float32 tensors: 1 + 1e-8 is 1, 1.001 is not
    assert D.same_spacing((1.0, 1.0, np.float32(1.0)), (1., 1., 1.)) and D.same_spacing((1.0, 1.0, 1.00000001), (1., 1., 1.))
    assert not D.same_spacing((1.0, 1.0, 1.001), (1., 1., 1.))
