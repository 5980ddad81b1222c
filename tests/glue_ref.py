"""float64 references and derived error bounds for the bandwidth-bound kernels between the convolutions (csrc/unet_misc.hip: in_bwd_finalize{,2},
maxpool_fwd{,2} / maxpool_bwd, subsample_fwd / bwd, upsample_fwd{,2,3} / upsample_bwd{,2,4}; csrc/loss.hip: plane_partials_fwd).  CPU only, numpy / torch.

Written from the DEFINITIONS of the operations, not from the kernels:
    max pool      nn.MaxPool3d(2)                                       model/dim3/unet_utils.py:35-37  (ATen keeps the FIRST maximum in (d, h, w) scan order)
    subsample     the stride-2 convolution evaluated at the even voxels  unet_utils.py:38-39            y = x[::2, ::2, ::2], output size ceil(D / 2)
    trilinear     F.interpolate(mode='trilinear', align_corners=True)    unet_utils.py:69               src = o (I - 1) / (O - 1), an exact rational here
    norm tail     the backward of nn.InstanceNorm3d(eps=1e-4, affine=False)  conv_layers.py:40-42       dx = rstd (g - m1 - x_n m2) [+ adds], x_n = (x - mean) rstd
    plane sums    the six sums per label plane of training/losses_foundation.py:945-956, :541-607 (spelt out by gpu_checks.check_plane_partials)
and the comment blocks of unet_misc.hip, which say the same.  tests/test_glue_ref_cpu.py proves each reference against torch float64 autograd, proves that a
correct f32 evaluation stays inside the trilinear bounds, and shows that each bound rejects a subtly wrong kernel.

Every reference takes channels-last tensors (N, D, H, W, C) AS STORED: the bf16 / f32 device values converted to float64.  Each returns the reference and the
per-element magnitude(s) its bound needs.  Every bound is reported as a RATIO |got - ref| / bound; <= 1 passes, NaN (an unwritten element) counts as inf.

The bounds, with u = 2^-24 (unit round-off of f32, round to nearest) and r the storage rounding (2^-8 bf16: half an ulp; 2^-24 f32):

    selection results (pool / subsample y, pool dx without add, subsample dx)
        the result IS one of the stored inputs (or 0): bit-exact equality.
    pool backward with add        |got - ref| <= r |ref| + u mag,  mag = |dy| + |add|
        one f32 addition of two stored values (u of the sum <= u mag), then the storage rounding.  (In f32 the two coincide; the sum of both terms stands.)
    norm tail                     |got - ref| <= r |ref| + 8 u mag,  mag = rstd (|g| + |m1| + |x_n m2|) + |adds|
        tests/test_gpu_block_stages.py's bound: the six to seven f32 operations of the tail and the additions, each at most u of a partial result that mag bounds.
    trilinear forward             |got - ref| <= r |ref| + c u mag,  c = 4 sum_axes (I_a - 1) + 16,  mag = the largest |corner|
        the kernels' coordinate (csrc/up_coord.hpp lin_coord) is src = fl(fl((I-1) / (O-1)) * o): two f32 roundings, each at most u relative of a value <= I - 1,
        so |d src| <= 2 (I - 1) u per axis.  The interpolant is continuous and piecewise linear in src with slope |x1 - x0| <= 2 mag, ALSO across a knot
        (where the f32 floor may pick the neighbouring cell with l = 1 - tiny): each axis moves the result by at most 4 (I - 1) u mag.  On top: 1 - l (one
        rounding), the two weight products, the eight multiply-adds: 11 roundings of partial results bounded by mag; 16 leaves room for an evaluation without
        fused multiply-add (tests/test_glue_ref_cpu.py runs one).  Because the f32 floor may pick the neighbouring cell at a knot, `mag` takes the corners
        of every cell within 4 (I - 1) u of src: two indices per axis, three at a knot.
    trilinear backward            |got - ref| <= r |ref| + u ((K + 4) mag_w + c_s mag_s),  c_s = 2 sum_axes (I_a - 1) + 4
        mag_w = sum |w| |dy| over the taps with the exact weights; K = the largest tap count of one input voxel (product of the per-axis counts): a sum of K
        products in f32, in any association, errs by at most K u mag_w (K enters as it does in the GEMM-stage bound), + 4 for the weight products and 1 - l.
        The f32 weights differ from the exact ones by |d src| <= 2 (I_a - 1) u per axis ABSOLUTELY (the hat function has slope 1), so a tap whose exact
        weight is 0 or tiny may carry up to that much: this part is bounded with mag_s = sum |dy| over the taps of the closed support widened by the
        coordinate error (|src - i| < 1 + 4 (I_a - 1) u on every axis; the other two axes' weights are <= 1).
    statistics rows, integer-valued inputs     sum over the rows of `part` in float64 EQUALS the integer sums
        inputs are integers in [-8, 8] (exact in bf16); while sum y^2 over a sample's channel stays below 2^24 every f32 partial sum is an exactly
        representable integer whatever the order (stat_sums_exact checks the cap per case), so a voxel counted twice or not at all shows as an inequality.
    statistics rows, general inputs            (mean, rstd) finalised by ops.stats_finalize against stat_sums of the STORED output: 1e-4 of the column's rms
        for the mean, 1e-4 relative for rstd (the block-stage criterion, check_conv_exact's).
    plane sums                    |got - ref| <= u (E + (m + 10) T) per (plane, column), + u |ref| for the reduced f32 sums; column 3 (the count t k) is exact
        T = sum of the |terms| of the column; m = the longest chain of f32 additions a thread makes (voxels per thread: ceil(V / (256 blocks)) + 16 for the
        16-voxel trips), + 8 levels of the block's tree reduction, + 2.  E = sum over voxels of the error of the f32 evaluation of the term:
        bce = max(x, 0) - x t + log(1 + e), e = exp(-|x|): x t is exact (t in {0, 1}); the subtraction and the addition round once each (u of <= |x| + 1);
        1 + e rounds by u absolutely and log has slope <= 1 there; the hardware exp2 / log2 are good to an ulp of their results (<= 1) and their argument
        scalings round once: at most 8 u (|x| + 1) per voxel.  sigmoid = (1 or e) / (1 + e): the exponent's scaling by log2(e) rounds (u |x| relative, twice
        for the constant), exp2 1 ulp, 1 + e, the reciprocal, the product: at most (2 |x| + 8) u relative.  Measured against gpu_checks.check_plane_partials'
        2e-5 of the global maximum this is a per-entry bound of about 1e-6 relative at the shapes used.
"""
import math
from fractions import Fraction

import numpy as np
import torch

U = 2.0 ** -24
R_STORE = {'bf16': 2.0 ** -8, 'f32': 2.0 ** -24}
EPS = 1e-4


# ================================================================================================ ratios
def ratio(got, ref, bound):
    """max |got - ref| / bound; a NaN or inf anywhere (an unwritten element) gives inf."""
    q = (got.double() - ref).abs() / (bound + 1e-300)
    q = torch.where(torch.isfinite(q), q, torch.full_like(q, float('inf')))
    return q.max().item() if q.numel() else 0.0


def rounded_sum_ratio(got, ref, mag, mode):
    """pool backward with add"""
    return ratio(got, ref, R_STORE[mode] * ref.abs() + U * mag)


def tail_ratio(got, ref, mag, mode):
    return ratio(got, ref, R_STORE[mode] * ref.abs() + 8 * U * mag)


def up_fwd_c(I):
    return 4 * sum(i - 1 for i in I) + 16


def up_fwd_ratio(got, ref, mag, I, mode):
    return ratio(got, ref, R_STORE[mode] * ref.abs() + up_fwd_c(I) * U * mag)


def up_bwd_ratio(got, ref, mag_w, mag_s, K, I, mode):
    return ratio(got, ref, R_STORE[mode] * ref.abs() + U * ((K + 4) * mag_w + (2 * sum(i - 1 for i in I) + 4) * mag_s))


def stats_ratio(fin, y):
    """(mean, rstd) (N, C, 2) against float64 sums over the stored channels-last tensor y: 1e-4 of the column's rms / of rstd.  Returns (mean, rstd) ratios."""
    fin = fin.double()
    cnt = y[0, ..., 0].numel()
    s = stat_sums(y)
    mean = s[..., 0] / cnt
    var = (s[..., 1] / cnt - mean * mean).clamp_min(0)
    rstd = 1.0 / torch.sqrt(var + EPS)
    rms = torch.sqrt(s[..., 1] / cnt).clamp_min(1e-30)
    em = ((fin[..., 0] - mean).abs() / rms).max().item()
    er = (fin[..., 1] / rstd - 1.0).abs().max().item()
    return tuple((e if e == e else float('inf')) / 1e-4 for e in (em, er))


# ================================================================================================ statistics
def stat_sums(y):
    """float64 (sum y, sum y^2) per (n, c) of a stored channels-last tensor: (N, C, 2)."""
    y = y.double().reshape(y.shape[0], -1, y.shape[-1])
    return torch.stack([y.sum(1), (y * y).sum(1)], -1)


def stat_sums_exact(y):
    """stat_sums of an integer-valued tensor, after checking the cap under which every f32 partial sum of any summation order is exact."""
    y = y.double()
    assert bool((y == y.round()).all()), 'integer-valued inputs only'
    s = stat_sums(y)
    assert s[..., 1].max().item() < 2 ** 24, 'sum y^2 of a channel reaches 2^24: f32 partial sums need not be exact'
    return s


def part_sums(part):
    """The rows of `part` (N, rows, C, 2) f32 added in float64: (N, C, 2)."""
    return part.double().sum(1)


# ================================================================================================ max pool
def _windows(x):
    """(N, D, H, W, C) -> (N, OD, OH, OW, C, 8): the 2x2x2 windows, last axis in (d, h, w) scan order; trailing odd planes dropped."""
    N, D, H, W, C = x.shape
    OD, OH, OW = D // 2, H // 2, W // 2
    w = x[:, :2 * OD, :2 * OH, :2 * OW].reshape(N, OD, 2, OH, 2, OW, 2, C)
    return w.permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(N, OD, OH, OW, C, 8)


def maxpool_fwd(x):
    return _windows(x.double()).max(-1).values


def maxpool_bwd(x, dy, add=None, last=False):
    """dx: dy at the FIRST maximum of each window in scan order (last=True: the mutant that keeps the last), 0 elsewhere and on the trailing planes of odd
    sizes; `add` is added everywhere.  Returns (dx, |dy| + |add| routed the same way)."""
    x, dy = x.double(), dy.double()
    N, D, H, W, C = x.shape
    OD, OH, OW = D // 2, H // 2, W // 2
    w = _windows(x)
    eq = w == w.max(-1, keepdim=True).values
    if last:
        pick = eq & (eq.flip(-1).cumsum(-1).flip(-1) == 1)
    else:
        pick = eq & (eq.cumsum(-1) == 1)
    assert bool((pick.sum(-1) == 1).all())

    def scatter(v):
        t = (pick * v[..., None]).reshape(N, OD, OH, OW, C, 2, 2, 2).permute(0, 1, 5, 2, 6, 3, 7, 4).reshape(N, 2 * OD, 2 * OH, 2 * OW, C)
        out = torch.zeros((N, D, H, W, C), dtype=torch.float64)
        out[:, :2 * OD, :2 * OH, :2 * OW] = t
        return out
    dx, mag = scatter(dy), scatter(dy.abs())
    if add is not None:
        dx, mag = dx + add.double(), mag + add.double().abs()
    return dx, mag


# ================================================================================================ subsample
def subsample_fwd(x):
    return x.double()[:, ::2, ::2, ::2].contiguous()


def subsample_bwd(dy, dims):
    """dims = (D, H, W) of the full grid: dy at the even voxels, 0 elsewhere."""
    N, C = dy.shape[0], dy.shape[-1]
    dx = torch.zeros((N,) + tuple(dims) + (C,), dtype=torch.float64)
    dx[:, ::2, ::2, ::2] = dy.double()
    return dx


# ================================================================================================ trilinear, align_corners=True
def src_coord(o, I, O):
    """The source coordinate of output o as an exact rational (ATen area_pixel_compute_source_index, align_corners=True: scale 0 for O = 1)."""
    return Fraction(o * (I - 1), O - 1) if O > 1 else Fraction(0)


def axis_tables(I, O):
    """One axis I -> O from the exact coordinates.  Returns float64 (Wm (O, I) interpolation weights, S (O, I) 0 / 1 widened closed support, lo (O,), hi (O,):
    the index range of the cells within the coordinate error of src)."""
    Wm, S = np.zeros((O, I)), np.zeros((O, I))
    lo, hi = np.zeros(O, dtype=np.int64), np.zeros(O, dtype=np.int64)
    tol = Fraction(4 * (I - 1), 2 ** 24)
    for o in range(O):
        src = src_coord(o, I, O)
        i0 = min(math.floor(src), I - 1)
        i1 = min(i0 + 1, I - 1)
        l1 = src - i0
        Wm[o, i0] += float(1 - l1)
        Wm[o, i1] += float(l1)
        lo[o], hi[o] = max(0, math.floor(src - tol)), min(I - 1, math.ceil(src + tol))
        a, b = max(0, math.ceil(src - 1 - tol)), min(I - 1, math.floor(src + 1 + tol))
        for i in range(a, b + 1):
            if abs(src - i) < 1 + tol:
                S[o, i] = 1.0
    return Wm, S, lo, hi


def _apply(t, M, axis):
    """contract `axis` of t (size M.shape[1]) with M (rows, size): the axis gets M.shape[0] entries"""
    return torch.movedim(torch.tensordot(t, torch.from_numpy(M), dims=([axis], [1])), -1, axis)


def trilinear_fwd(x, size):
    """x (N, ID, IH, IW, C) -> (y (N, OD, OH, OW, C), mag: the largest |corner| of the cells within the coordinate error)."""
    x = x.double()
    y, m = x, x.abs()
    for a in range(3):
        Wm, _, lo, hi = axis_tables(x.shape[1 + a], size[a])
        y = _apply(y, Wm, 1 + a)
        lo_t, hi_t = torch.from_numpy(lo), torch.from_numpy(hi)
        m = torch.stack([m.index_select(1 + a, torch.minimum(lo_t + k, hi_t)) for k in range(3)]).max(0).values
    return y, m


def trilinear_bwd(dy, in_size):
    """dy (N, OD, OH, OW, C) -> (dx (N, ID, IH, IW, C), mag_w, mag_s, K): the transpose of trilinear_fwd."""
    dy = dy.double()
    dx, mw, ms, K = dy, dy.abs(), dy.abs(), 1
    for a in range(3):
        Wm, S, _, _ = axis_tables(in_size[a], dy.shape[1 + a])
        dx, mw, ms = _apply(dx, Wm.T.copy(), 1 + a), _apply(mw, Wm.T.copy(), 1 + a), _apply(ms, S.T.copy(), 1 + a)
        K *= int(S.sum(0).max())
    return dx, mw, ms, K


# ---- the f32 restatement: a correct f32 evaluation (csrc/up_coord.hpp lin_coord, no fused multiply-add) that the bounds above must admit
def lin_coord_f32(I, O):
    """(i0, i1, l1) of every output of one axis, in float32 with one rounding per operation."""
    f = np.float32
    scale = f(f(I - 1) / f(O - 1)) if O > 1 else f(0)
    src = (scale * np.arange(O, dtype=np.float32)).astype(np.float32)
    i0 = np.minimum(src.astype(np.int64), I - 1)
    i1 = i0 + (i0 < I - 1)
    return i0, i1, (src - i0.astype(np.float32)).astype(np.float32)


def trilinear_fwd_f32(x, size):
    """x: float32 numpy (N, ID, IH, IW, C).  Weight products ((wd wh) ww), eight multiplies and adds, each rounded to f32."""
    f = np.float32
    x = x.astype(f)
    (d0, d1, ld), (h0, h1, lh), (w0, w1, lw) = (lin_coord_f32(x.shape[1 + a], size[a]) for a in range(3))
    acc = np.zeros((x.shape[0],) + tuple(size) + (x.shape[-1],), dtype=f)
    for dd, wd in ((d0, (f(1) - ld).astype(f)), (d1, ld)):
        for hh, wh in ((h0, (f(1) - lh).astype(f)), (h1, lh)):
            for ww_, ww in ((w0, (f(1) - lw).astype(f)), (w1, lw)):
                wt = ((wd[:, None, None] * wh[None, :, None]).astype(f) * ww[None, None, :]).astype(f)
                v = x[:, dd][:, :, hh][:, :, :, ww_]
                acc = (acc + (wt[None, ..., None] * v).astype(f)).astype(f)
    return acc


def trilinear_bwd_f32(dy, in_size):
    """dy: float32 numpy (N, OD, OH, OW, C) -> dx, accumulated tap by tap in f32 with the f32 weights of lin_coord_f32 (scatter form of the transpose)."""
    f = np.float32
    dy = dy.astype(f)
    O = dy.shape[1:4]
    (d0, d1, ld), (h0, h1, lh), (w0, w1, lw) = (lin_coord_f32(in_size[a], O[a]) for a in range(3))
    dx = np.zeros((dy.shape[0],) + tuple(in_size) + (dy.shape[-1],), dtype=f)
    for dd, wd in ((d0, (f(1) - ld).astype(f)), (d1, ld)):
        for hh, wh in ((h0, (f(1) - lh).astype(f)), (h1, lh)):
            for ww_, ww in ((w0, (f(1) - lw).astype(f)), (w1, lw)):
                wt = ((wd[:, None, None] * wh[None, :, None]).astype(f) * ww[None, None, :]).astype(f)
                contrib = (wt[None, ..., None] * dy).astype(f)
                for od in range(O[0]):              # one output plane after the other: np.add.at rounds every addition to f32
                    np.add.at(dx[:, dd[od]], (slice(None), hh[:, None], ww_[None, :]), contrib[:, od])
    return dx


# ================================================================================================ InstanceNorm backward tail
def in_bwd_tail(g, x, mr, gm, adds=()):
    """g, x (N, vox, C) as stored; mr = (mean, rstd), gm = (m1, m2): (N, C, 2) f32 tables.  dx = rstd (g - m1 - x_n m2) + adds, and its magnitude."""
    g, x = g.double(), x.double()
    mu, rs, m1, m2 = (t.double()[:, None, :] for t in (mr[..., 0], mr[..., 1], gm[..., 0], gm[..., 1]))
    t = (x - mu) * rs * m2
    ref, mag = rs * (g - m1 - t), rs.abs() * (g.abs() + m1.abs() + t.abs())
    for a in adds:
        ref, mag = ref + a.double(), mag + a.double().abs()
    return ref, mag


# ================================================================================================ loss plane sums
def unpack_labels(tpk, tC):
    """np.packbits(label, axis=class) bytes (B, tP, V) -> (B * tC, V) 0 / 1: class c is bit 7 - (c & 7) of byte plane c >> 3."""
    tpk = np.asarray(tpk)
    B, tP, V = tpk.shape
    out = np.empty((B, tC, V), dtype=np.uint8)
    for c in range(tC):
        out[:, c] = (tpk[:, c >> 3] >> (7 - (c & 7))) & 1
    return out.reshape(B * tC, V)


def plane_sums(x, t, k=None, w2=None, w1=None, chain=0):
    """x (planes, V) logits as stored (f32); t (planes, V) 0 / 1 labels (bytes: non-zero counts as 1); k known-voxel mask, w2 background mask, w1 weights:
    optional.  Returns (ref (planes, 6), bound (planes, 6)) in float64:
        S = sum bce k, A = sum sig k, B = sum sig t k, Cn = sum t k, F1 = sum bce k w1, F2 = sum bce k (1 - w2)       (0 for F1 without w1)
    chain: the longest chain of f32 additions (see the module docstring); bound[:, 3] = 0: the count is exact."""
    x = torch.as_tensor(np.asarray(x), dtype=torch.float64)
    one = torch.ones_like(x)
    t = (torch.as_tensor(np.asarray(t)) != 0).double()
    k = one if k is None else (torch.as_tensor(np.asarray(k)) != 0).double()
    bg = one if w2 is None else (torch.as_tensor(np.asarray(w2)) == 0).double()
    w1 = torch.zeros_like(x) if w1 is None else torch.as_tensor(np.asarray(w1), dtype=torch.float64)
    bce = torch.clamp(x, min=0) - x * t + torch.log1p(torch.exp(-x.abs()))
    sg = torch.sigmoid(x)
    e_bce, e_sg = 8 * (x.abs() + 1), sg * (2 * x.abs() + 8)
    terms = [bce * k, sg * k, sg * t * k, t * k, bce * k * w1, bce * k * bg]
    errs = [e_bce * k, e_sg * k, e_sg * t * k, 0 * k, e_bce * k * w1.abs(), e_bce * k * bg]
    ref = torch.stack([v.sum(1) for v in terms], -1)
    bound = U * torch.stack([e.sum(1) + (chain + 10) * v.abs().sum(1) for e, v in zip(errs, terms)], -1)
    bound[:, 3] = 0
    return ref, bound


def plane_ratio(got, ref, bound, reduced=False):
    """per-entry |got - ref| / bound; the exact count column (bound 0) must be equal"""
    got = got.double()
    if reduced:
        bound = bound + U * ref.abs()
    exact = bound == 0
    bad = (exact & (got != ref)) | ~torch.isfinite(got)
    q = torch.where(exact, torch.zeros_like(ref), (got - ref).abs() / (bound + 1e-300))
    q = torch.where(bad, torch.full_like(q, float('inf')), q)
    return q.max().item()


def plane_chain(V, blocks):
    return -(-V // (256 * blocks)) + 16


# ================================================================================================ the GPU cases (tests/test_gpu_glue_ref.py), shared with the CPU test
# kernel names are rsuper_amd.hip.lib.GLUE_KERNELS'; sel: U of in_bwd_finalize2 / NT of upsample_bwd4; z: blocks in z (the channel split)
TAIL_CASES = [  # (id, mode, N, vox, C, adds, kernel, sel)
    ('bf16-255', 'bf16', 1, 8160, 64, 0, 'in_bwd_finalize_kernel', 0), ('bf16-256', 'bf16', 1, 8161, 64, 1, 'in_bwd_finalize2_kernel', 2),
    ('bf16-1023', 'bf16', 1, 32736, 64, 2, 'in_bwd_finalize2_kernel', 2), ('bf16-1024', 'bf16', 1, 32737, 64, 0, 'in_bwd_finalize2_kernel', 4),
    ('bf16-8192', 'bf16', 1, 262144, 64, 1, 'in_bwd_finalize2_kernel', 4), ('bf16-8193', 'bf16', 1, 262145, 64, 2, 'in_bwd_finalize_kernel', 0),
    ('bf16-C24', 'bf16', 2, 30000, 24, 1, 'in_bwd_finalize_kernel', 0),        # 352 blocks' worth: only the vector count (3) keeps it off finalize2
    ('bf16-small', 'bf16', 2, 7 * 9 * 11, 8, 2, 'in_bwd_finalize_kernel', 0),
    ('f32-C8', 'f32', 2, 7 * 9 * 11, 8, 1, 'in_bwd_finalize_kernel', 0), ('f32-C8-U2', 'f32', 1, 40000, 8, 2, 'in_bwd_finalize2_kernel', 2),
    ('f32-C64', 'f32', 1, 8161, 64, 0, 'in_bwd_finalize2_kernel', 2),
]
POOL_CASES = [  # (id, mode, N, (D, H, W), C, forward kernel, z, backward threads per block)
    ('odd', 'bf16', 1, (7, 9, 11), 8, 'maxpool_fwd2_kernel', 1, 64), ('even', 'bf16', 1, (6, 10, 14), 8, 'maxpool_fwd2_kernel', 1, 64),
    ('C128', 'bf16', 2, (12, 12, 12), 128, 'maxpool_fwd2_kernel', 2, 64), ('C256', 'bf16', 2, (12, 12, 12), 256, 'maxpool_fwd2_kernel', 4, 64),
    ('C320', 'bf16', 2, (12, 12, 12), 320, 'maxpool_fwd2_kernel', 2, 64),
    ('rows1008', 'bf16', 1, (126, 64, 64), 8, 'maxpool_fwd2_kernel', 1, 64), ('rows1024', 'bf16', 1, (128, 64, 64), 8, 'maxpool_fwd_kernel', 1, 64),
    ('bwd496', 'bf16', 1, (128, 128, 62), 8, 'maxpool_fwd_kernel', 1, 64), ('bwd512', 'bf16', 1, (128, 128, 64), 8, 'maxpool_fwd_kernel', 1, 256),
    ('f32-odd', 'f32', 1, (7, 9, 11), 8, 'maxpool_fwd2_kernel', 1, 64), ('f32-C256', 'f32', 2, (12, 12, 12), 256, 'maxpool_fwd2_kernel', 4, 64),
]
SUB_CASES = [  # (id, mode, N, (D, H, W), C, z)
    ('odd', 'bf16', 1, (7, 9, 11), 8, 1), ('C256', 'bf16', 2, (12, 12, 12), 256, 4), ('C320', 'bf16', 2, (24, 24, 24), 320, 2), ('f32-odd', 'f32', 1, (7, 9, 11), 8, 1),
]
UP_FWD_CASES = [  # (id, mode, N, I, O, C, kernel, z)
    ('ragged', 'bf16', 1, (3, 5, 4), (7, 9, 11), 8, 'upsample_fwd3_kernel', 1), ('axis1', 'bf16', 1, (5, 1, 7), (5, 4, 7), 8, 'upsample_fwd3_kernel', 1),
    ('C320', 'bf16', 2, (6, 6, 6), (12, 12, 12), 320, 'upsample_fwd3_kernel', 2), ('C256', 'bf16', 2, (12, 12, 12), (24, 24, 24), 256, 'upsample_fwd3_kernel', 4),
    ('w3070', 'bf16', 1, (1, 1, 1536), (1, 1, 3070), 8, 'upsample_fwd3_kernel', 1), ('w3071', 'bf16', 1, (1, 1, 1536), (1, 1, 3071), 8, 'upsample_fwd2_kernel', 1),
    ('f32-ragged', 'f32', 1, (3, 5, 4), (7, 9, 11), 8, 'upsample_fwd3_kernel', 1),
]
UP_FWD_STRIDED = ('strided', 'bf16', 2, (12, 12, 12), (24, 24, 24), 64, 'upsample_fwd3_kernel')      # input ld 96 at channel 32, output ld 128 at channel 64
UP_BWD_CASES = [  # (id, mode, N, I, O, C, kernel, NT)
    ('2x', 'bf16', 2, (6, 6, 6), (12, 12, 12), 64, 'upsample_bwd4_kernel', 4), ('ragged', 'bf16', 1, (3, 5, 7), (6, 9, 13), 8, 'upsample_bwd4_kernel', 4),
    ('scale1', 'bf16', 1, (5, 4, 3), (5, 4, 3), 8, 'upsample_bwd4_kernel', 4),
    ('3x', 'bf16', 1, (3, 3, 4), (8, 9, 10), 24, 'upsample_bwd4_kernel', 6),       # 3 -> 9 along w: five or six outputs per input index
    # 3 -> 10 along w: more than six outputs per input index, the row-sharing kernel's tables do not hold it: the gather kernel, which is also what
    # RSUPER_UPSAMPLE_BWD4=0 selects
    ('gather', 'bf16', 1, (3, 3, 3), (8, 9, 10), 24, 'upsample_bwd2_kernel', 0),
    ('f32-ragged', 'f32', 1, (3, 5, 4), (7, 9, 11), 8, 'upsample_bwd2_kernel', 0),
]
PLANE_CASES = [  # (id, planes, V, label form, known-voxel mask, background mask)
    ('bits', 26, 40 * 36 * 28, 'bits', True, False), ('bytes-odd', 3, 7 * 9 * 11, 'bytes', False, False), ('bytes-masks', 6, 12 ** 3, 'bytes', True, True),
    ('V4096', 2, 4096, 'bytes', True, False), ('V4097', 2, 4097, 'bytes', True, False),      # rsuper_plane_partials_blocks: 1 | 2
]


def glue_plan(op, mode, N, shape, C, ld=None):
    """rsuper_glue_plan's answer (host code, no GPU) as a dict: kernel NAME, sel, bx, by, bz, threads, lds, rows."""
    import ctypes
    from rsuper_amd.hip import lib
    ops_ = ('in_bwd', 'pool_fwd', 'pool_bwd', 'sub_fwd', 'sub_bwd', 'up_fwd', 'up_bwd')
    out = (ctypes.c_int * 8)(*([-7] * 8))
    rc = lib.lib().rsuper_glue_plan(ops_.index(op), {'f32': lib.F32, 'bf16': lib.BF16}[mode], (ctypes.c_int * 7)(N, *shape), C, C if ld is None else ld, out)
    assert rc == 0, (op, mode, N, shape, C, rc)
    p = dict(zip(('kernel', 'sel', 'bx', 'by', 'bz', 'threads', 'lds', 'rows'), out))
    p['kernel'] = lib.GLUE_KERNELS[p['kernel']]
    return p


DTYPES = {'f32': torch.float32, 'bf16': torch.bfloat16}


def stored(seed, shape, mode, kind='gauss'):
    """A seeded CPU tensor in the storage type of `mode`, the same for the CPU and the GPU test.  gauss: N(0, 1) rounded to the storage type; ints: integers
    in [-8, 8] (exact in bf16, for the exact statistics rows; full of ties); levels: five values (max-pool ties)."""
    g = torch.Generator().manual_seed(seed)
    if kind == 'gauss':
        t = torch.randn(shape, generator=g, dtype=torch.float32)
    elif kind == 'ints':
        t = torch.randint(-8, 9, shape, generator=g).float()
    else:
        t = torch.randint(0, 5, shape, generator=g).float() * 0.5 - 1.0
    return t.to(DTYPES[mode])
