"""CPU restatement of the NIfTI front and back end (inference/nifti.py, inference/nifti_device.py, csrc/nifti.hip) for the tests.  It imports
nothing of the product: its own NIfTI-1 header writer and parser on struct, reorientation as numpy transpose + flips, and the reference's
"cubic B-spline in-plane, nearest along z" resample as scipy.ndimage.map_coordinates(order=3, mode='mirror') per source slice.

Conventions (the same as the product states them, written down independently): a file holds voxels (i, j, k), i fastest; the canonical array is
array[z, y, x] with x towards the patient's left, y towards posterior, z towards superior -- ITK 'RAI', i.e. ('L', 'P', 'S') in RAS+ axis codes.
perm[a] is the canonical axis (0 = x, 1 = y, 2 = z) of voxel axis a, flip[a] says the voxel axis runs against it."""
import gzip
import itertools
import math
import struct

import numpy as np

DTYPES = {2: 'u1', 256: 'i1', 4: 'i2', 512: 'u2', 8: 'i4', 16: 'f4', 64: 'f8'}
CANON_SIGN = (-1.0, -1.0, 1.0)
ORIENTATIONS = [(p, f) for p in itertools.permutations(range(3)) for f in itertools.product((False, True), repeat=3)]      # all 48


def affine_for(perm, flip, pixdim, origin=(0.0, 0.0, 0.0)):
    """The voxel -> RAS+ affine of a scan whose voxel axis a lies along canonical axis perm[a] (against it when flip[a]) with spacing pixdim[a]."""
    A = np.eye(4)
    A[:3, :3] = 0.0
    for a in range(3):
        A[perm[a], a] = CANON_SIGN[perm[a]] * (-1.0 if flip[a] else 1.0) * pixdim[a]
    A[:3, 3] = origin
    return A


def reorient(arr_ijk, perm, flip):
    """(ni, nj, nk) array -> canonical (Z, Y, X) array."""
    a = arr_ijk
    for ax in range(3):
        if flip[ax]:
            a = np.flip(a, axis=ax)
    inv = [perm.index(w) for w in range(3)]
    return np.ascontiguousarray(a.transpose(inv[2], inv[1], inv[0]))


def inverse_reorient(canon_zyx, perm, flip):
    """canonical (Z, Y, X) array -> (ni, nj, nk) array."""
    xyz = canon_zyx.transpose(2, 1, 0)                      # axes: canonical x, y, z
    a = xyz.transpose(perm[0], perm[1], perm[2])            # voxel axis a is canonical axis perm[a]
    for ax in range(3):
        if flip[ax]:
            a = np.flip(a, axis=ax)
    return np.ascontiguousarray(a)


def file_order(arr_ijk):
    """The flat voxel buffer of a file: i fastest."""
    return np.ascontiguousarray(arr_ijk.transpose(2, 1, 0)).reshape(-1)


def rotation_to_quaternion(R):
    """(b, c, d) of a proper rotation matrix (a >= 0), by the largest diagonal term."""
    a2 = (1.0 + R[0, 0] + R[1, 1] + R[2, 2]) / 4.0
    b2 = (1.0 + R[0, 0] - R[1, 1] - R[2, 2]) / 4.0
    c2 = (1.0 - R[0, 0] + R[1, 1] - R[2, 2]) / 4.0
    d2 = (1.0 - R[0, 0] - R[1, 1] + R[2, 2]) / 4.0
    k = int(np.argmax([a2, b2, c2, d2]))
    if k == 0:
        a = math.sqrt(a2)
        q = [a, (R[2, 1] - R[1, 2]) / (4 * a), (R[0, 2] - R[2, 0]) / (4 * a), (R[1, 0] - R[0, 1]) / (4 * a)]
    elif k == 1:
        b = math.sqrt(b2)
        q = [(R[2, 1] - R[1, 2]) / (4 * b), b, (R[0, 1] + R[1, 0]) / (4 * b), (R[0, 2] + R[2, 0]) / (4 * b)]
    elif k == 2:
        c = math.sqrt(c2)
        q = [(R[0, 2] - R[2, 0]) / (4 * c), (R[0, 1] + R[1, 0]) / (4 * c), c, (R[1, 2] + R[2, 1]) / (4 * c)]
    else:
        d = math.sqrt(d2)
        q = [(R[1, 0] - R[0, 1]) / (4 * d), (R[0, 2] + R[2, 0]) / (4 * d), (R[1, 2] + R[2, 1]) / (4 * d), d]
    if q[0] < 0:
        q = [-v for v in q]
    return q[1], q[2], q[3]


def qform_of(affine):
    """(b, c, d, qfac, pixdim) that encode an orthogonal affine as a NIfTI qform."""
    M = np.asarray(affine, dtype=np.float64)[:3, :3]
    pix = np.linalg.norm(M, axis=0)
    R = M / pix[None, :]
    qfac = 1.0
    if np.linalg.det(R) < 0:
        qfac = -1.0
        R = R * np.array([1.0, 1.0, -1.0])[None, :]
    return rotation_to_quaternion(R) + (qfac, tuple(pix))


def header_bytes(shape, datatype, pixdim, *, bo='<', slope=0.0, inter=0.0, sform=None, qform=None, qoffset=(0.0, 0.0, 0.0), dim0=3, dim4=1,
                 sizeof_hdr=348, magic=b'n+1\x00', vox_offset=352.0):
    """348 header bytes + 4 extension bytes.  sform: a 4 x 4 affine or None (sform_code 0); qform: (b, c, d, qfac) or None (qform_code 0)."""
    h = bytearray(352)
    struct.pack_into(bo + 'i', h, 0, sizeof_hdr)
    struct.pack_into(bo + '8h', h, 40, dim0, shape[0], shape[1], shape[2], dim4, 1, 1, 1)
    struct.pack_into(bo + '2h', h, 70, datatype, 8 * np.dtype(DTYPES[datatype]).itemsize)
    qfac = 1.0 if qform is None else qform[3]
    struct.pack_into(bo + '8f', h, 76, qfac, pixdim[0], pixdim[1], pixdim[2], 0.0, 0.0, 0.0, 0.0)
    struct.pack_into(bo + '3f', h, 108, vox_offset, slope, inter)
    struct.pack_into(bo + '2h', h, 252, 0 if qform is None else 1, 0 if sform is None else 1)
    if qform is not None:
        struct.pack_into(bo + '6f', h, 256, qform[0], qform[1], qform[2], *qoffset)
    if sform is not None:
        struct.pack_into(bo + '12f', h, 280, *np.asarray(sform, dtype=np.float64)[:3, :].reshape(-1).tolist())
    h[344:348] = magic
    return bytes(h)


def write_nifti(path, arr_ijk, datatype, pixdim, *, bo='<', truncate=0, **kw):
    """Write arr_ijk (ni, nj, nk) as a NIfTI-1 single file of `datatype` in byte order `bo`; gzip by the file name; `truncate` drops that many
    payload bytes from the end."""
    payload = file_order(arr_ijk).astype(np.dtype(DTYPES[datatype]).newbyteorder(bo)).tobytes()
    if truncate:
        payload = payload[:-truncate]
    data = header_bytes(arr_ijk.shape, datatype, pixdim, bo=bo, **kw) + payload
    with (gzip.open(path, 'wb') if str(path).endswith('.gz') else open(path, 'wb')) as f:
        f.write(data)


def parse_header(raw):
    """The fields of a little-endian NIfTI-1 header the tests look at."""
    assert struct.unpack('<i', raw[:4])[0] == 348 and raw[344:348] == b'n+1\x00', 'not a little-endian NIfTI-1 single-file header'
    dim = struct.unpack('<8h', raw[40:56])
    datatype, bitpix = struct.unpack('<2h', raw[70:74])
    pixdim = struct.unpack('<8f', raw[76:108])
    vox_offset, slope, inter = struct.unpack('<3f', raw[108:120])
    qcode, scode = struct.unpack('<2h', raw[252:256])
    quat = struct.unpack('<6f', raw[256:280])
    srow = np.array(struct.unpack('<12f', raw[280:328]), dtype=np.float64).reshape(3, 4)
    return dict(dim=dim, datatype=datatype, bitpix=bitpix, pixdim=pixdim, vox_offset=vox_offset, slope=slope, inter=inter, qform_code=qcode,
                sform_code=scode, quatern=quat[:3], qoffset=quat[3:], srow=srow, extension=bytes(raw[348:352]))


def quaternion_affine(h):
    """The affine a parsed header's qform encodes."""
    b, c, d = h['quatern']
    a = 1.0 - b * b - c * c - d * d
    if a < 1e-7:                                            # a half turn: renormalise, as the NIfTI-1 C library reads it
        n = math.sqrt(b * b + c * c + d * d)
        a, b, c, d = 0.0, b / n, c / n, d / n
    else:
        a = math.sqrt(a)
    R = np.array([[a * a + b * b - c * c - d * d, 2 * b * c - 2 * a * d, 2 * b * d + 2 * a * c],
                  [2 * b * c + 2 * a * d, a * a + c * c - b * b - d * d, 2 * c * d - 2 * a * b],
                  [2 * b * d - 2 * a * c, 2 * c * d + 2 * a * b, a * a + d * d - c * c - b * b]])
    qfac = -1.0 if h['pixdim'][0] < 0 else 1.0
    A = np.eye(4)
    A[:3, :3] = R * np.array([h['pixdim'][1], h['pixdim'][2], h['pixdim'][3] * qfac])[None, :]
    A[:3, 3] = h['qoffset']
    return A


def read_nifti_gz(path):
    """(parsed header, (ni, nj, nk) array) of a little-endian .nii.gz: gzip plus the plain header parse."""
    with gzip.open(path, 'rb') as f:
        raw = f.read()
    h = parse_header(raw)
    ni, nj, nk = h['dim'][1:4]
    flat = np.frombuffer(raw, dtype=np.dtype(DTYPES[h['datatype']]).newbyteorder('<'), count=ni * nj * nk, offset=int(h['vox_offset']))
    return h, flat.reshape(nk, nj, ni).transpose(2, 1, 0)


# ---- the resample
def out_size(n_in, sp_in, sp_out):
    return int(round(n_in * sp_in / sp_out))


def positions(n_in, sp_in, sp_out):
    """(source positions of every output index in float64, inside mask): -0.5 <= pos < n_in - 0.5."""
    pos = np.array([o * sp_out / sp_in for o in range(out_size(n_in, sp_in, sp_out))], dtype=np.float64)
    return pos, (pos >= -0.5) & (pos < n_in - 0.5)


def nearest_table(n_in, sp_in, sp_out):
    """floor(pos + 0.5) (round half up), -1 outside."""
    pos, inside = positions(n_in, sp_in, sp_out)
    return np.where(inside, np.minimum(np.floor(pos + 0.5), n_in - 1), -1).astype(np.int64)


def resample(canon_zyx, spacing_xyz, target_xyz, outside_value=0.0):
    """The reference's two passes on a canonical (Z, Y, X) volume: cubic B-spline over x and y of each source slice (scipy, float64,
    mode='mirror'), nearest along z.  Returns (float64 (Zo, Yo, Xo) volume, boolean mask of the voxels inside the scan)."""
    from scipy import ndimage
    Z, Y, X = canon_zyx.shape
    px, inx = positions(X, spacing_xyz[0], target_xyz[0])
    py, iny = positions(Y, spacing_xyz[1], target_xyz[1])
    zt = nearest_table(Z, spacing_xyz[2], target_xyz[2])
    out = np.full((len(zt), len(py), len(px)), float(outside_value), dtype=np.float64)
    inside = np.zeros(out.shape, dtype=bool)
    plane_in = iny[:, None] & inx[None, :]
    coords = np.stack(np.meshgrid(py, px, indexing='ij'))
    done = {}
    for zo, zs in enumerate(zt):
        if zs < 0:
            continue
        if zs not in done:
            done[zs] = ndimage.map_coordinates(canon_zyx[zs].astype(np.float64), coords, order=3, mode='mirror')
        out[zo][plane_in] = done[zs][plane_in]
        inside[zo] = plane_in
    return out, inside


def prefilter_line(s):
    """The cubic B-spline coefficients of one line in float64 by the recursion the kernels use: pole z1 = sqrt(3) - 2, gain (1 - z1)(1 - 1/z1),
    the exact whole-sample mirror start sums; a line of one sample is the sample."""
    s = np.asarray(s, dtype=np.float64)
    N = len(s)
    if N == 1:
        return s.copy()
    z1 = math.sqrt(3.0) - 2.0
    g = (1.0 - z1) * (1.0 - 1.0 / z1)
    P = 2 * N - 2
    mir = [k if k < N else P - k for k in range(P)]
    cp = np.empty(N)
    cp[0] = sum(z1 ** k * g * s[mir[k]] for k in range(P)) / (1.0 - z1 ** P)
    for k in range(1, N):
        cp[k] = g * s[k] + z1 * cp[k - 1]
    c = np.empty(N)
    c[N - 1] = z1 / (z1 * z1 - 1.0) * (cp[N - 1] + z1 * cp[N - 2])
    for k in range(N - 2, -1, -1):
        c[k] = z1 * (c[k + 1] - cp[k])
    return c


def phantom(shape_zyx, seed):
    """int16 HU in [-1024, 3071] with sharp edges: a random walk along x plus a step phantom (blocks of air, soft tissue and bone)."""
    rng = np.random.default_rng(seed)
    Z, Y, X = shape_zyx
    walk = np.cumsum(rng.integers(-60, 61, size=(Z, Y, X)), axis=2) + rng.integers(-200, 200, size=(Z, Y, 1))
    zz, yy, xx = np.meshgrid(np.arange(Z), np.arange(Y), np.arange(X), indexing='ij')
    steps = np.where(((xx // 5 + yy // 3 + zz) % 3) == 0, -1024, np.where(((xx // 5 + yy // 3 + zz) % 3) == 1, 40, 1800))
    return np.clip(walk + steps, -1024, 3071).astype(np.int16)
