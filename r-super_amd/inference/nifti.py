"""NIfTI-1 single-file reader and writer, orientation and resampling tables: the host half of the NIfTI front end (the device half is
inference/nifti_device.py, csrc/nifti.hip).  Pure Python: struct, gzip and numpy -- no nibabel, no SimpleITK, no torch.

What the reference does with SimpleITK before the clip of `preprocess` (predict_abdomenatlas.py:333-343, dataset_conversion/utils.py:10-47):
read the image, reorient_image(img, 'RAI'), resample x and y with a cubic B-spline and z with nearest neighbour to the target spacing,
GetArrayFromImage.  Here the file's voxel buffer is returned as it lies in the file; `orientation_plan` says which voxel axis becomes which
canonical axis and `resample_axis_table` gives the per-axis source indices and weights, both consumed by the device kernels.

Orientation.  The canonical array is the reference's `GetArrayFromImage(reorient_image(img, 'RAI'))`: array[z, y, x] with x increasing towards
the patient's LEFT, y towards POSTERIOR, z towards SUPERIOR.  ITK's "RAI" names where an axis comes FROM, and ITK's world is LPS; a NIfTI affine
maps to RAS+.  In nibabel's axis codes (where an axis goes TO, in RAS+) the canonical axes are therefore ('L', 'P', 'S'): canonical x is world
-x, canonical y is world -y, canonical z is world +z.

Checked against scipy (tests/nifti_ref.py), not against ITK: the inside rule, the default pixel, round-half-up of the nearest table and the
mirror boundary are written from ITK's documented behaviour."""
import gzip
import math
import struct
from dataclasses import dataclass, field

import numpy as np

# NIfTI-1 datatype code -> (numpy type character with its size, bitpix)
DATATYPES = {2: ('u1', 8), 256: ('i1', 8), 4: ('i2', 16), 512: ('u2', 16), 8: ('i4', 32), 16: ('f4', 32), 64: ('f8', 64)}
HEADER_BYTES = 348
VOX_OFFSET = 352
OUTSIDE = -1                                   # the "outside" marker of an index table
CANONICAL_SIGN = (-1.0, -1.0, 1.0)             # canonical x, y, z along the RAS+ world axes: L, P, S
Z1 = math.sqrt(3.0) - 2.0                      # the pole of the cubic B-spline prefilter


@dataclass
class NiftiVolume:
    """A NIfTI-1 file: `data` is the flat voxel buffer in file order (i fastest) in the machine's byte order, float64 already converted to
    float32; `shape` is (ni, nj, nk)."""
    path: str
    data: np.ndarray
    shape: tuple
    pixdim: tuple                              # pixdim[1..3]
    qfac: float
    datatype: int
    vox_offset: int
    scl_slope: float
    scl_inter: float
    qform_code: int
    sform_code: int
    quatern: tuple                             # (b, c, d)
    qoffset: tuple
    srow: np.ndarray = field(default=None)     # (3, 4) float64


def _read_bytes(path):
    path = str(path)
    try:
        if path.endswith('.gz'):
            with gzip.open(path, 'rb') as f:
                return f.read()
        with open(path, 'rb') as f:
            return f.read()
    except (EOFError, gzip.BadGzipFile, OSError) as e:
        if isinstance(e, FileNotFoundError):
            raise
        raise ValueError(f'{path}: not a readable NIfTI-1 file ({type(e).__name__}: {e})') from None


def read_nifti(path):
    """Read a `.nii` / `.nii.gz` NIfTI-1 single file of either byte order.  ValueError (naming the file) for NIfTI-2, Analyze and two-file
    NIfTI, for anything but a 3-D volume (dim[0] == 3, or 4 with dim[4] == 1), an unsupported datatype and truncated data."""
    raw = _read_bytes(path)
    if len(raw) < HEADER_BYTES:
        raise ValueError(f'{path}: truncated: {len(raw)} bytes hold no NIfTI-1 header')
    for bo in '<>':
        size = struct.unpack(bo + 'i', raw[:4])[0]
        if size in (HEADER_BYTES, 540):
            break
    else:
        raise ValueError(f'{path}: sizeof_hdr is neither 348 nor 540: not a NIfTI file')
    if size == 540:
        raise ValueError(f'{path}: NIfTI-2 is not supported (NIfTI-1 single file only)')
    magic = raw[344:348]
    if magic != b'n+1\x00':
        kind = 'a two-file NIfTI-1 pair' if magic == b'ni1\x00' else 'Analyze 7.5 (no NIfTI magic)'
        raise ValueError(f'{path}: {kind} is not supported (NIfTI-1 single file only)')
    dim = struct.unpack(bo + '8h', raw[40:56])
    if not (dim[0] == 3 or (dim[0] == 4 and dim[4] == 1)) or min(dim[1:4]) < 1:
        raise ValueError(f'{path}: dim = {list(dim)}: only 3-D volumes (dim[0] == 3, or 4 with dim[4] == 1) are read')
    datatype, bitpix = struct.unpack(bo + '2h', raw[70:74])
    if datatype not in DATATYPES:
        raise ValueError(f'{path}: datatype {datatype} is not supported (uint8, int8, int16, uint16, int32, float32, float64)')
    pixdim = struct.unpack(bo + '8f', raw[76:108])
    vox_offset, slope, inter = struct.unpack(bo + '3f', raw[108:120])
    qform_code, sform_code = struct.unpack(bo + '2h', raw[252:256])
    quat = struct.unpack(bo + '6f', raw[256:280])
    srow = np.array(struct.unpack(bo + '12f', raw[280:328]), dtype=np.float64).reshape(3, 4)
    shape = tuple(int(v) for v in dim[1:4])
    n = shape[0] * shape[1] * shape[2]
    off = int(vox_offset) if vox_offset >= VOX_OFFSET else VOX_OFFSET
    dt = np.dtype(DATATYPES[datatype][0]).newbyteorder(bo)
    if len(raw) < off + n * dt.itemsize:
        raise ValueError(f'{path}: truncated: {n} voxels of {dt.itemsize} bytes at offset {off} need {off + n * dt.itemsize} bytes, the file has {len(raw)}')
    data = np.frombuffer(raw, dtype=dt, count=n, offset=off)
    data = data.astype(np.float32 if datatype == 64 else dt.newbyteorder('='))           # the byte swap and the float64 conversion
    return NiftiVolume(path=str(path), data=np.ascontiguousarray(data), shape=shape, pixdim=tuple(float(v) for v in pixdim[1:4]),
                       qfac=-1.0 if pixdim[0] < 0 else 1.0, datatype=int(datatype), vox_offset=off,
                       scl_slope=float(slope), scl_inter=float(inter), qform_code=int(qform_code), sform_code=int(sform_code),
                       quatern=tuple(float(v) for v in quat[:3]), qoffset=tuple(float(v) for v in quat[3:]), srow=srow)


def quaternion_to_rotation(b, c, d):
    """The rotation matrix of the unit quaternion (a, b, c, d), a >= 0 implied."""
    a = 1.0 - (b * b + c * c + d * d)
    if a < 1e-7:                                   # a half turn: float32 b, c, d leave no digits for a (the rule of the NIfTI-1 C library)
        n = 1.0 / math.sqrt(b * b + c * c + d * d)
        a, b, c, d = 0.0, b * n, c * n, d * n
    else:
        a = math.sqrt(a)
    return np.array([[a * a + b * b - c * c - d * d, 2 * (b * c - a * d), 2 * (b * d + a * c)],
                     [2 * (b * c + a * d), a * a + c * c - b * b - d * d, 2 * (c * d - a * b)],
                     [2 * (b * d - a * c), 2 * (c * d + a * b), a * a + d * d - b * b - c * c]])


def affine(vol):
    """The 4 x 4 voxel (i, j, k) -> RAS+ millimetre matrix: the sform if sform_code > 0, else the qform, else diag(pixdim) (nibabel's order)."""
    A = np.eye(4)
    if vol.sform_code > 0:
        A[:3, :] = vol.srow
    elif vol.qform_code > 0:
        R = quaternion_to_rotation(*vol.quatern)
        A[:3, :3] = R * np.array([vol.pixdim[0], vol.pixdim[1], vol.pixdim[2] * vol.qfac])[None, :]
        A[:3, 3] = vol.qoffset
    else:
        A[:3, :3] = np.diag(vol.pixdim)
    return A


def orientation_plan(aff):
    """(perm, flip) of a voxel -> RAS+ affine.  perm[a] is the world axis (0, 1, 2 = the canonical x, y, z) on which voxel axis a (i, j, k) has its
    largest absolute direction cosine; flip[a] says that the voxel axis runs against the canonical direction and has to be reversed.

    Canonical means the reference's array: x towards the patient's left, y towards posterior, z towards superior -- ITK's 'RAI' (named by where an
    axis comes from, in ITK's LPS world), which in RAS+ axis codes is ('L', 'P', 'S').  So a voxel axis whose cosine on world x or y is positive
    is flipped, and one whose cosine on world z is negative.  An oblique scan resolves to its nearest axis permutation, as DICOMOrientImageFilter
    does; ValueError if two cosines of an axis tie or two voxel axes claim the same world axis."""
    R = np.asarray(aff, dtype=np.float64)[:3, :3]
    perm, flip = [], []
    for a in range(3):
        col = R[:, a]
        norm = float(np.linalg.norm(col))
        if not norm > 0:
            raise ValueError(f'orientation_plan: voxel axis {a} has no direction in {R.tolist()}')
        cos = np.abs(col) / norm
        order = np.argsort(-cos)
        if cos[order[0]] - cos[order[1]] < 1e-6:
            raise ValueError(f'orientation_plan: voxel axis {a} lies equally along two world axes ({(col / norm).tolist()})')
        w = int(order[0])
        perm.append(w)
        flip.append(bool(np.sign(col[w]) != CANONICAL_SIGN[w]))
    if sorted(perm) != [0, 1, 2]:
        raise ValueError(f'orientation_plan: the voxel axes map to world axes {perm}, which is no permutation')
    return tuple(perm), tuple(flip)


def canonical_layout(shape_ijk, perm, flip):
    """How the canonical (Z, Y, X) array lies in the file's flat buffer: ((X, Y, Z), (sx, sy, sz) element strides, start offset, voxel axis of each
    canonical axis).  A flipped axis has a negative stride and starts at its far end."""
    file_stride = (1, shape_ijk[0], shape_ijk[0] * shape_ijk[1])
    inv = [perm.index(w) for w in range(3)]
    size = tuple(int(shape_ijk[a]) for a in inv)
    stride = tuple(-file_stride[a] if flip[a] else file_stride[a] for a in inv)
    offset = sum((shape_ijk[a] - 1) * file_stride[a] for a in range(3) if flip[a])
    return size, stride, offset, tuple(inv)


def _rotation_to_quaternion(R):
    a = R[0, 0] + R[1, 1] + R[2, 2] + 1.0
    if a > 0.5:
        a = 0.5 * math.sqrt(a)
        b, c, d = 0.25 * (R[2, 1] - R[1, 2]) / a, 0.25 * (R[0, 2] - R[2, 0]) / a, 0.25 * (R[1, 0] - R[0, 1]) / a
    else:
        xd, yd, zd = 1.0 + R[0, 0] - (R[1, 1] + R[2, 2]), 1.0 + R[1, 1] - (R[0, 0] + R[2, 2]), 1.0 + R[2, 2] - (R[0, 0] + R[1, 1])
        if xd > 1.0:
            b = 0.5 * math.sqrt(xd)
            c, d, a = 0.25 * (R[0, 1] + R[1, 0]) / b, 0.25 * (R[0, 2] + R[2, 0]) / b, 0.25 * (R[2, 1] - R[1, 2]) / b
        elif yd > 1.0:
            c = 0.5 * math.sqrt(yd)
            b, d, a = 0.25 * (R[0, 1] + R[1, 0]) / c, 0.25 * (R[1, 2] + R[2, 1]) / c, 0.25 * (R[0, 2] - R[2, 0]) / c
        else:
            d = 0.5 * math.sqrt(zd)
            b, c, a = 0.25 * (R[0, 2] + R[2, 0]) / d, 0.25 * (R[1, 2] + R[2, 1]) / d, 0.25 * (R[1, 0] - R[0, 1]) / d
        if a < 0:
            b, c, d = -b, -c, -d
    return b, c, d


def nifti1_header(shape_ijk, pixdim, aff, datatype):
    """The 352 bytes in front of the voxels of a little-endian NIfTI-1 single file: the 348-byte header (magic n+1, vox_offset 352, no scaling,
    sform_code = qform_code = 2 (aligned), millimetres) and the 4-byte extension flag.  srow_* are the affine's rows; the quaternion is the
    rotation nearest to its direction cosines, qfac (pixdim[0]) its handedness."""
    if datatype not in DATATYPES:
        raise ValueError(f'nifti1_header: datatype {datatype} is not supported')
    A = np.asarray(aff, dtype=np.float64)
    M = A[:3, :3] / np.maximum(np.linalg.norm(A[:3, :3], axis=0), 1e-30)[None, :]
    qfac = 1.0
    if np.linalg.det(M) < 0:
        qfac = -1.0
        M = M * np.array([1.0, 1.0, -1.0])[None, :]
    U, _, Vt = np.linalg.svd(M)
    b, c, d = _rotation_to_quaternion(U @ Vt)
    h = bytearray(HEADER_BYTES + 4)
    struct.pack_into('<i', h, 0, HEADER_BYTES)
    struct.pack_into('<8h', h, 40, 3, int(shape_ijk[0]), int(shape_ijk[1]), int(shape_ijk[2]), 1, 1, 1, 1)
    struct.pack_into('<2h', h, 70, datatype, DATATYPES[datatype][1])
    struct.pack_into('<8f', h, 76, qfac, float(pixdim[0]), float(pixdim[1]), float(pixdim[2]), 1.0, 1.0, 1.0, 1.0)
    struct.pack_into('<3f', h, 108, float(VOX_OFFSET), 1.0, 0.0)
    h[123] = 2                                                     # xyzt_units: millimetres
    struct.pack_into('<2h', h, 252, 2, 2)
    struct.pack_into('<6f', h, 256, b, c, d, A[0, 3], A[1, 3], A[2, 3])
    struct.pack_into('<12f', h, 280, *A[:3, :].reshape(-1).tolist())
    h[344:348] = b'n+1\x00'
    return bytes(h)


def bspline_weights(t):
    """The four cubic B-spline weights of the taps floor(pos) - 1 ... floor(pos) + 2 at t = pos - floor(pos)."""
    return ((1.0 - t) ** 3 / 6.0, (3.0 * t ** 3 - 6.0 * t ** 2 + 4.0) / 6.0, (-3.0 * t ** 3 + 3.0 * t ** 2 + 3.0 * t + 1.0) / 6.0, t ** 3 / 6.0)


def mirror_index(i, n):
    """Whole-sample mirror about 0 and n - 1 (period 2 (n - 1)); n == 1: always 0."""
    if n == 1:
        return 0
    p = 2 * (n - 1)
    m = i % p
    return m if m < n else p - m


def output_size(n_in, sp_in, sp_out):
    """int(round(n_in * sp_in / sp_out)) with Python's round, as ResampleXYZAxis writes it."""
    return int(round(n_in * sp_in * 1.0 / sp_out))


def source_position(o, sp_in, sp_out):
    """Output index -> continuous source index: same origin and direction, identity transform."""
    return o * sp_out / sp_in


def resample_axis_table(n_in, sp_in, sp_out, kind):
    """One axis of the reference's resample, in float64.  Output index o samples source position o * sp_out / sp_in; it is inside while
    -0.5 <= pos < n_in - 0.5, otherwise the output voxel takes the outside value (ITK's default pixel).

    kind 'bspline': (idx (n_out, 4) int32, w (n_out, 4) float32) -- taps floor(pos) - 1 ... + 2 mirrored into the axis and their cubic B-spline
    weights, cast to float32 last; an outside row has idx OUTSIDE and weight 0.
    kind 'nearest': idx (n_out,) int32 = floor(pos + 0.5) (round half up), OUTSIDE where outside."""
    if kind not in ('bspline', 'nearest'):
        raise ValueError(f"resample_axis_table: kind {kind!r} (bspline / nearest)")
    n_in, sp_in, sp_out = int(n_in), float(sp_in), float(sp_out)
    n_out = output_size(n_in, sp_in, sp_out)
    if n_in < 1 or n_out < 1:
        raise ValueError(f'resample_axis_table: {n_in} samples at {sp_in} give {n_out} at {sp_out}')
    if kind == 'nearest':
        idx = np.full((n_out,), OUTSIDE, dtype=np.int32)
    else:
        idx = np.full((n_out, 4), OUTSIDE, dtype=np.int32)
        w = np.zeros((n_out, 4), dtype=np.float64)
    for o in range(n_out):
        pos = source_position(o, sp_in, sp_out)
        if not -0.5 <= pos < n_in - 0.5:
            continue
        if kind == 'nearest':
            idx[o] = min(int(math.floor(pos + 0.5)), n_in - 1)
        else:
            f = math.floor(pos)
            idx[o] = [mirror_index(int(f) - 1 + k, n_in) for k in range(4)]
            w[o] = bspline_weights(pos - f)
    return idx if kind == 'nearest' else (idx, w.astype(np.float32))
