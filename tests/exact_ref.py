"""Integer-operand references for the MFMA reduction kernels (stride-1 / stride-2 3x3x3 weight gradient, csrc/pointwise.hip), host only: no import of
rsuper_amd.hip.  The companion of glue_ref.py and block_stage_ref.py; tests/gpu_checks.py (check_wgrad_int, check_wgrad_s2_int, check_pointwise_int) runs
the kernels on these operands and tests/test_exact_ref_cpu.py checks the instrument itself without a GPU.

The idea (tests/test_gpu_glue_ref.py uses it for max-pool and subsample as kind='ints'): small integers and multiples of 1/2 with a few significant bits
are exact in bf16, their products are multiples of 1/2, and while 2 * sum|a||b| stays below 2^24 every partial sum of the reduction is an integer count of
halves that f32 holds exactly -- in ANY order: any MFMA step order, any slab split, any reduction tree.  The kernel must then equal the float64 result at
every element with no tolerance, so one lost, doubled or misplaced term fails at any reduction length (a tolerance relative to the tensor's max hides a
single voxel from R ~ 10^3 on: the sum grows like sqrt(R), a term stays O(1)).

The InstanceNorm + ReLU prologue is pinned the same way: the (mean, rstd) rows are an INPUT of the kernels, so integer means and power-of-two rstd make
fma(x, rstd, -mean * rstd) exact, and they are drawn per sample and per channel so that a kernel reading the wrong row of the table fails.

Integers cannot see a wrong rounding mode: gpu_checks.check_pointwise_exact / check_wgrad_exact pin that on real-valued operands with derived bounds."""
import functools

import numpy as np
import torch
import torch.nn.functional as F

X_RANGE, Y_RANGE, B_RANGE, MEANS, RSTDS = 3, 2, 4, (-2, -1, 0, 1, 2), (0.5, 1.0, 2.0)
X_NARROW, MEANS_NARROW = 2, (-1, 0, 1)          # the one large case (2 x 32 x 48 x 48): same rstd, |x_hat| <= 6


# ================================================================================================ cases (the GPU file and the CPU file import these)
# (kernel, cfg, mt, mode, N, S, Ca, Cb, Ya, Yb, norm, thr, tr[, sliced[, narrow]]) of gpu_checks.check_wgrad_int.  kernel / cfg / mt: what
# rsuper_conv3_wgrad_plan answers for the launch under threshold thr (rsuper_conv3_wgrad2_min_tiles; None: the default) -- the check asserts it before it
# launches, and test_exact_ref_cpu.py asserts it on the host.  norm: 'raw' | 'both' (every x source carries statistics) | 'mixed' (a normalised, b raw).
# sliced: the two dY sources are channel slices of one tensor (ld = Ya + Yb).  Shapes: the smallest at which each path exists.
NEVER = 1 << 20
WGRAD_INT = [
    # ---- tile-streaming kernel (threshold "never"): each configuration with the transposed LDS reads and without, cfg 0 / 1 in f32 too
    ('tile', 0, 1, 'bf16', 1, (8, 8, 16), 32, 0, 32, 0, 'both', NEVER, 1), ('tile', 0, 1, 'bf16', 1, (8, 8, 16), 32, 0, 32, 0, 'both', NEVER, 0),
    ('tile', 1, 2, 'bf16', 1, (8, 8, 16), 32, 0, 64, 0, 'both', NEVER, 1), ('tile', 1, 2, 'bf16', 1, (8, 8, 16), 32, 0, 64, 0, 'both', NEVER, 0),
    ('tile', 2, 2, 'bf16', 1, (16, 32, 64), 32, 0, 64, 0, 'both', NEVER, 1), ('tile', 2, 2, 'bf16', 1, (16, 32, 64), 32, 0, 64, 0, 'both', NEVER, 0),
    ('tile', 0, 1, 'f32', 1, (8, 8, 16), 32, 0, 32, 0, 'both', NEVER, 1), ('tile', 1, 2, 'f32', 1, (8, 8, 16), 32, 0, 64, 0, 'both', NEVER, 1),
    ('tile', 0, 1, 'bf16', 1, (5, 6, 7), 8, 16, 8, 8, 'both', NEVER, 1),                  # ragged on every face, channel tails, two x / two dY sources
    ('tile', 0, 1, 'bf16', 1, (7, 9, 35), 40, 0, 24, 0, 'raw', NEVER, 1),
    ('tile', 0, 1, 'bf16', 9, (3, 2, 7), 16, 0, 16, 0, 'both', NEVER, 1),                 # more samples than tiles
    ('tile', 1, 2, 'bf16', 2, (8, 12, 20), 64, 32, 64, 64, 'mixed', NEVER, 1),            # src_flags bit 0
    # ---- second-generation kernel (threshold 0): 32-row form, 64-row form, two 32-row blocks per chunk (wgrad2_mt1: 576 tiles >= 512)
    ('wgrad2', 0, 1, 'bf16', 1, (8, 8, 16), 32, 0, 32, 0, 'both', 0, 1),
    ('wgrad2', 2, 2, 'bf16', 1, (16, 32, 64), 32, 0, 64, 0, 'both', 0, 1),
    ('wgrad2', 2, 1, 'bf16', 2, (32, 48, 48), 32, 0, 64, 0, 'both', 0, 1, False, True),
    # W mod 16 >= 8 (validity bits of the upper half of a tile row), sliced dY, two x sources.  Fewer than 128 tiles at more than 32 rows is the 9-tap
    # configuration, which the second-generation kernel never takes (csrc/wgrad_plan.hpp): under threshold 0 these three run the tile kernel, cfg 1 ...
    ('tile', 1, 2, 'bf16', 1, (9, 9, 31), 64, 0, 128, 128, 'both', 0, 1, True),
    ('tile', 1, 2, 'bf16', 2, (6, 7, 25), 32, 0, 32, 32, 'both', 0, 1, True),
    ('tile', 1, 2, 'bf16', 2, (11, 9, 29), 64, 64, 64, 64, 'raw', 0, 1),
    # ... so the same three properties on the second-generation kernel itself: 32 rows (any tile count), and 64 / 128 rows at 128 tiles
    ('wgrad2', 0, 1, 'bf16', 1, (9, 9, 31), 64, 0, 32, 0, 'both', 0, 1),
    ('wgrad2', 2, 2, 'bf16', 2, (16, 13, 63), 32, 0, 32, 32, 'both', 0, 1, True),
    ('wgrad2', 2, 2, 'bf16', 2, (13, 16, 61), 32, 32, 32, 32, 'raw', 0, 1),
    # ---- small-volume kernel (default threshold): 6^3 whole, 12^3 in two depth parts, two x / dY sources, ragged
    ('sv', 1, 1, 'bf16', 2, (6, 6, 6), 64, 0, 64, 0, 'both', None, 1),
    ('sv', 1, 1, 'bf16', 2, (12, 12, 12), 64, 0, 64, 0, 'both', None, 1),
    ('sv', 1, 1, 'bf16', 2, (12, 12, 12), 96, 32, 64, 32, 'both', None, 1),
    # a first dY source of 24 rows (not a multiple of 32) keeps a fused [conv1 | shortcut] off the small-volume kernel: tile kernel, cfg 1 ...
    ('tile', 1, 2, 'bf16', 1, (11, 9, 13), 40, 0, 24, 24, 'both', None, 1),
    # ... and the same ragged volume with 32 + 24 rows on the small-volume kernel
    ('sv', 1, 1, 'bf16', 1, (11, 9, 13), 40, 0, 32, 24, 'both', None, 1),
]

# (mode, N, S, Ca, Ya, Yb) of gpu_checks.check_wgrad_s2_int: even / ragged / odd sizes, one and two dY sources, channel tails
WGRAD_S2_INT = [(m, *c) for m in ('bf16', 'f32') for c in
                [(1, (8, 8, 32), 32, 32, 0), (2, (12, 10, 20), 16, 32, 32), (1, (7, 9, 35), 8, 16, 16), (2, (5, 17, 66), 40, 24, 24), (1, (2, 3, 5), 8, 8, 8),
                 (1, (13, 13, 13), 16, 32, 32)]]

# (mode, R, K, N) of gpu_checks.check_pointwise_int(..., sliced=True): operands as column slices [:, 4:4+width] of matrices 8 columns wider
POINTWISE_SLICED = [('bf16', 200, 116, 64), ('f32', 200, 60, 64), ('bf16', 65, 64, 64), ('bf16', 4096, 68, 68)]

# real-valued rounding checks (gpu_checks.check_wgrad_exact): (stride, N, S, Ca, Cb, Ya, Yb, thr, sliced), R <= 4096 voxels
WGRAD_EXACT = [(1, 1, (8, 8, 16), 32, 0, 32, 0, NEVER, False), (1, 1, (8, 8, 16), 32, 0, 32, 0, 0, False), (1, 1, (8, 8, 16), 32, 0, 64, 0, NEVER, False),
               (1, 1, (5, 6, 7), 8, 16, 8, 8, NEVER, False), (1, 1, (7, 9, 35), 40, 0, 24, 0, NEVER, False), (1, 2, (6, 6, 6), 64, 0, 64, 0, None, False),
               (1, 2, (12, 12, 12), 64, 0, 64, 0, None, False), (1, 1, (11, 9, 13), 40, 0, 24, 24, None, False), (1, 1, (11, 9, 13), 40, 0, 32, 24, None, False),
               (1, 1, (9, 9, 31), 64, 0, 128, 128, 0, True), (1, 1, (9, 9, 31), 64, 0, 32, 0, 0, False),
               (2, 1, (8, 8, 32), 32, 0, 32, 0, None, False), (2, 2, (12, 10, 20), 16, 0, 32, 32, None, False), (2, 1, (7, 9, 35), 8, 0, 16, 16, None, False),
               (2, 1, (2, 3, 5), 8, 0, 8, 8, None, False)]


# ================================================================================================ operands
def _ints(g, shape, hi):
    return torch.from_numpy(g.integers(-hi, hi + 1, size=shape).astype(np.float32))


def stats_int(g, N, C, narrow=False):
    """(N, C, 2) rows (mean, rstd): integer means, power-of-two rstd, drawn per sample and per channel."""
    means = MEANS_NARROW if narrow else MEANS
    m = torch.from_numpy(g.choice(np.asarray(means, dtype=np.float32), size=(N, C)))
    r = torch.from_numpy(g.choice(np.asarray(RSTDS, dtype=np.float32), size=(N, C)))
    return torch.stack([m, r], dim=-1)


def xhat_int(x, mr):
    """relu(x * rstd - mean * rstd) on (N, C, D, H, W) integers and (N, C, 2) integer-mean / power-of-two-rstd rows, in float64: a multiple of 1/2 of
    at most 5 significant bits (|x - mean| <= 5, times 1/2, 1 or 2), exact in f32 and bf16.  mr None: the raw source, x itself."""
    if mr is None:
        return x.double()
    sc = mr[:, :, 1].double()[:, :, None, None, None]
    return torch.relu(x.double() * sc - mr[:, :, 0].double()[:, :, None, None, None] * sc)


@functools.lru_cache(maxsize=None)
def wgrad_operands(N, S, Ca, Cb, Ya, Yb, norm, stride=1, narrow=False, seed=0):
    """Seeded integer operands of one weight-gradient case, f32 on the host: dict(xa, xb, mra, mrb, dy (N, Ya + Yb, ...), xh = [x_hat a | x_hat b] float64).
    Cached and shared: callers must not modify them."""
    g = np.random.default_rng(1000 + seed)
    D, H, W = S
    So = S if stride == 1 else tuple((s + 1) // 2 for s in S)
    hi = X_NARROW if narrow else X_RANGE
    xa = _ints(g, (N, Ca, D, H, W), hi)
    xb = _ints(g, (N, Cb, D, H, W), hi) if Cb else None
    mra = stats_int(g, N, Ca, narrow) if norm in ('both', 'mixed') else None
    mrb = stats_int(g, N, Cb, narrow) if (Cb and norm == 'both') else None
    dy = _ints(g, (N, Ya + Yb) + So, Y_RANGE)
    xh = xhat_int(xa, mra) if xb is None else torch.cat([xhat_int(xa, mra), xhat_int(xb, mrb)], 1)
    return dict(xa=xa, xb=xb, mra=mra, mrb=mrb, dy=dy, xh=xh)


def wgrad_f64(xh, dy, stride=1):
    """dW (Y, C, 3, 3, 3) of F.conv3d(xh, w, stride, padding=1) for the output gradient dy, by autograd in float64 (as gpu_checks.check_wgrad_xhat)."""
    w = torch.zeros((dy.shape[1], xh.shape[1], 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(xh.double(), w, stride=stride, padding=1).backward(dy.double())
    return w.grad


@functools.lru_cache(maxsize=None)
def wgrad_mag(N, S, Ca, Cb, Ya, Yb, norm, stride=1, narrow=False, seed=0):
    """sum|x_hat||dy| per element of dW: the same reduction over absolute values."""
    o = wgrad_operands(N, S, Ca, Cb, Ya, Yb, norm, stride, narrow, seed)
    return wgrad_f64(o['xh'].abs(), o['dy'].abs(), stride)


@functools.lru_cache(maxsize=None)
def wgrad_ref(N, S, Ca, Cb, Ya, Yb, norm, stride=1, narrow=False, seed=0):
    """(dW float64 of all Ya + Yb rows, its magnitude) of the case's operands.  Computed once and shared: do not modify."""
    o = wgrad_operands(N, S, Ca, Cb, Ya, Yb, norm, stride, narrow, seed)
    return wgrad_f64(o['xh'], o['dy'], stride), wgrad_mag(N, S, Ca, Cb, Ya, Yb, norm, stride, narrow, seed)


def wgrad_int_key(case):
    """The operand key (arguments of wgrad_operands / wgrad_ref) of an entry of WGRAD_INT."""
    N, S, Ca, Cb, Ya, Yb, norm = case[4:11]
    return (N, S, Ca, Cb, Ya, Yb, norm, 1, len(case) > 14 and bool(case[14]))


@functools.lru_cache(maxsize=None)
def pointwise_operands(R, K, N, seed=0):
    """x (R, K) in [-3, 3], w (N, K) and dy (R, N) in [-2, 2], bias (N,) and res (R, N) in [-4, 4]: integers as f32.  Cached: do not modify."""
    g = np.random.default_rng(2000 + seed)
    return dict(x=_ints(g, (R, K), X_RANGE), w=_ints(g, (N, K), Y_RANGE), dy=_ints(g, (R, N), Y_RANGE), b=_ints(g, (N,), B_RANGE), res=_ints(g, (R, N), B_RANGE))


def pointwise_ref(o):
    """float64 matmul references of everything gpu_checks.check_pointwise computes, and their magnitudes (the same reductions over absolute values; the
    forward's includes |bias| + |res|): dict name -> (ref, mag) for y (bias), yr (bias + residual), dx, dw, db."""
    x, w, dy, b, res = (o[k].double() for k in ('x', 'w', 'dy', 'b', 'res'))
    y, ym = x @ w.t() + b, x.abs() @ w.abs().t() + b.abs()
    return dict(y=(y, ym), yr=(y + res, ym + res.abs()), dx=(dy @ w, dy.abs() @ w.abs()), dw=(dy.t() @ x, dy.abs().t() @ x.abs()), db=(dy.sum(0), dy.abs().sum(0)))


# ================================================================================================ the two judgements
def exact_ok(mag):
    """f32 accumulation of the terms behind `mag` (= sum|a||b| per element) is exact in any order: every term is a multiple of 1/2, so every partial sum
    is a count of halves of at most 2 * mag, which must stay below 2^24."""
    return bool(2.0 * float(mag.max()) < 2.0 ** 24)


def mismatch(got, ref):
    """Compare by value (-0 equals +0; a non-finite `got` never equals): (count, None) when equal, else (count, (index, got, ref)) of the first
    differing element in row-major order."""
    got, ref = got.detach().cpu().double(), ref.detach().cpu().double()
    assert got.shape == ref.shape, (tuple(got.shape), tuple(ref.shape))
    bad = ~(torch.isfinite(got) & (got == ref))
    n = int(bad.sum())
    if not n:
        return 0, None
    i = int(torch.nonzero(bad.reshape(-1))[0])
    idx = tuple(int(v) for v in np.unravel_index(i, tuple(got.shape)))
    return n, (idx, float(got.reshape(-1)[i]), float(ref.reshape(-1)[i]))


def mismatch_note(what, got, ref):
    """'' when equal, else 'what: n of m differ, first at index: got g, ref r'."""
    n, first = mismatch(got, ref)
    return '' if not n else f'{what}: {n} of {ref.numel()} differ, first at {first[0]}: got {first[1]!r}, ref {first[2]!r}'
