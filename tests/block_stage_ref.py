"""Float64 reference of every stage of BasicBlockFn (rsuper_amd/hip/ops.py: _BB.forward, _forward_s2, _backward_s1, _backward_s2), one plain torch function
per stage, CPU only.

Each function takes the tensors the previous stage STORED (teacher forcing) as (N, C, D, H, W) tensors and returns (ref, mag): the float64 value of the stage
and the sum of the absolute values of its terms, the magnitude the f32 rounding slack of the kernels scales with (as in gpu_checks.check_conv_exact).
The operation order is restated from the kernels:
    prologue   x_hat = bf16(max(fma(x, rstd, -mean * rstd), 0))                      csrc/common.hpp norm_relu16       (gpu_checks._xhat_bf16)
    mask       x > mean, i.e. the sign of the f32 value (x - mean) * rstd            epilogue of the data-gradient kernels
    tail       x_n = (x - mean) * rstd;  dx = rstd * (g - m1 - x_n * m2) [+ add1]    csrc/unet_misc.hip in_bwd_tail, one rounding when stored
`exact=True` leaves out every bf16 rounding (tests/test_block_stage_ref_cpu.py chains the stages on their own outputs and compares with autograd).
A source without statistics (mr None) is raw: no normalisation, no ReLU, no mask, no tail.
"""
import torch
import torch.nn.functional as F

EPS = 1e-4


def _bc(v):
    return v[:, :, None, None, None]


def stats(y):
    """(mean, rstd) of a stored tensor, (N, C, 2) float64: biased variance, eps = 1e-4 (what stats_finalize derives from the partial sums)."""
    y = y.double()
    m = y.mean(dim=(2, 3, 4))
    v = (y * y).mean(dim=(2, 3, 4)) - m * m
    return torch.stack([m, 1.0 / torch.sqrt(v.clamp_min(0) + EPS)], -1)


def x_hat(x, mr, exact=False):
    """The prologue of every conv input.  mr None: a raw source passes through."""
    if mr is None:
        return x.double()
    if exact:
        return torch.relu((x.double() - _bc(mr[..., 0].double())) * _bc(mr[..., 1].double()))
    from gpu_checks import _xhat_bf16
    return _xhat_bf16(x.float(), mr.float())


def x_hat_cat(srcs, exact=False):
    """srcs: list of (x, mr or None) -> x_hat of the concatenated sources."""
    return torch.cat([x_hat(x, mr, exact) for x, mr in srcs], 1)


def _w(w, exact):
    return w.double() if exact else w.float().bfloat16().double()


def _mag32(fn, a, w, **kw):
    # the magnitude only scales a bound: f32 is plenty and several times cheaper on the CPU
    return fn(a.abs().float(), w.abs().float(), **kw).double()


def conv_fwd(xh, weights, stride=1, res=None, exact=False):
    """[conv(xh, w) for w in weights] concatenated over the output channels (+ res): ys = [y1 | sc] and out = conv2 + residual."""
    ws = [_w(w, exact) for w in weights]
    ref = torch.cat([F.conv3d(xh, w, stride=stride, padding=1) for w in ws], 1)
    mag = torch.cat([_mag32(F.conv3d, xh, w, stride=stride, padding=1) for w in ws], 1)
    if res is not None:
        ref, mag = ref + res.double(), mag + res.double().abs()
    return ref, mag


def relu_mask(srcs):
    """(mask, ties) of the concatenated sources: x > mean with the f32 mean the kernel holds; a tie is a voxel whose f32 (x - mean) * rstd is exactly 0."""
    ms, ts = [], []
    for x, mr in srcs:
        if mr is None:
            ms.append(torch.ones_like(x, dtype=torch.float64)); ts.append(torch.zeros_like(x, dtype=torch.bool))
        else:
            xn = (x.double() - _bc(mr[..., 0].double())) * _bc(mr[..., 1].double())
            ms.append((xn > 0).double())
            ts.append(xn.float() == 0)          # x == mean (or a product that underflows in f32): the kernel's value carries no sign here
    return torch.cat(ms, 1), torch.cat(ts, 1)


def dgrad(dys, weights, srcs, stride=1, exact=False):
    """g = sum_i convT(dy_i, w_i) * mask(x): g1 = convT(dout, w2) [y1 > mean], g0 = convT([dy1 | dout], [w1 | ws]) mask(x).  Returns (ref, mag, ties)."""
    mask, ties = relu_mask(srcs)
    kw = dict(stride=stride, padding=1)
    if stride == 2:
        kw['output_padding'] = tuple(1 - s % 2 for s in mask.shape[2:])
    ref = sum(F.conv_transpose3d(dy.double(), _w(w, exact), **kw) for dy, w in zip(dys, weights))
    mag = sum(_mag32(F.conv_transpose3d, dy.double(), _w(w, exact), **kw) for dy, w in zip(dys, weights))
    return ref * mask, mag * mask, ties


def x_norm(x, mr):
    return (x.double() - _bc(mr[..., 0].double())) * _bc(mr[..., 1].double())


def bwd_means(g, x, mr):
    """(mean g, mean g x_n) over the stored g, (N, C, 2) float64: the InstanceNorm-backward rows a data-gradient launch emits."""
    g = g.double()
    return torch.stack([g.mean(dim=(2, 3, 4)), (g * x_norm(x, mr)).mean(dim=(2, 3, 4))], -1)


def tail(g, x, mr, gm, add=None):
    """dx = rstd * (g - m1 - x_n m2) [+ add], and rstd * (|g| + |m1| + |x_n m2|) [+ |add|]."""
    g, rs, m1, m2 = g.double(), _bc(mr[..., 1].double()), _bc(gm[..., 0].double()), _bc(gm[..., 1].double())
    t = x_norm(x, mr) * m2
    ref, mag = rs * (g - m1 - t), rs.abs() * (g.abs() + m1.abs() + t.abs())
    if add is not None:
        ref, mag = ref + add.double(), mag + add.double().abs()
    return ref, mag


def wgrad(xh, dy, stride=1):
    """dW of conv(xh, W) for the output gradient dy, float64."""
    w = torch.zeros((dy.shape[1], xh.shape[1], 3, 3, 3), dtype=torch.float64, requires_grad=True)
    F.conv3d(xh, w, stride=stride, padding=1).backward(dy.double())
    return w.grad


# The seeded cases of tests/test_gpu_block_stages.py: name -> (N, (D, H, W), Ca, Cb, Cout, shortcut, second source raw, stride, seed).  The smallest shapes
# that still take each path (see the GPU test); nothing above ~10^4 voxels per sample except A2.
CASES = {
    'A': (2, (9, 17, 33), 32, 64, 32, True, False, 1, 100),       # decoder head scaled down: 32 n + 64 n -> 32 + shortcut
    # A with 512 tiles of 4x4x16 voxels, the smallest volume whose joint 96-column data gradient takes 32-column blocks (below, the launch is under-filled and
    # the plan answers with wider blocks): the one condition of ops.split_dgrad_sources besides its tile threshold that depends on the size
    'A2': (2, (5, 29, 241), 32, 64, 32, True, False, 1, 210),
    'B': (1, (8, 16, 32), 64, 0, 32, True, False, 1, 110),        # 64 n -> 32 + shortcut
    'C32a': (2, (5, 9, 19), 32, 0, 32, False, False, 1, 120),     # identity shortcut: the tail adds dOut
    'C32b': (1, (12, 12, 12), 32, 0, 32, False, False, 1, 130),
    'C64a': (2, (5, 9, 19), 64, 0, 64, False, False, 1, 140),
    'C64b': (1, (12, 12, 12), 64, 0, 64, False, False, 1, 150),   # 12^3: the small-volume weight gradient by default
    'D128': (2, (6, 6, 6), 128, 0, 128, False, False, 1, 160),    # 6^3: the volume-fitted kernel, split reduction through the registered workspace
    'D64': (2, (6, 6, 6), 64, 64, 64, True, False, 1, 170),
    'E': (1, (8, 12, 20), 32, 32, 32, True, True, 1, 180),        # one normalised and one raw source
    'G16': (1, (13, 13, 13), 16, 0, 32, True, False, 2, 190),     # stride 2, odd sizes
    'G32': (2, (12, 10, 20), 32, 0, 64, True, False, 2, 200),     # stride 2, even / ragged sizes
}


def make_inputs(name):
    """The seeded operands of a case, CPU f32 tensors holding bf16-representable activations (the values the device tensors hold) and f32 weights:
    dict(srcs=[(x, mr or None)], w1, w2, ws, dout, stride).  mr = statistics of the bf16 values, f32, as the producer of x would hand them on."""
    import math
    import os
    import sys
    import numpy as np
    g = os.path.join(os.path.dirname(os.path.abspath(__file__)), 'golden')
    if g not in sys.path:
        sys.path.insert(0, g)
    import synth
    N, (D, H, W), Ca, Cb, Cout, has_sc, b_raw, stride, seed = CASES[name]

    def rt(k, shape, scale=1.0):
        return torch.from_numpy(synth.rng(seed + k).standard_normal(shape).astype(np.float32) * np.float32(scale))
    xa = (rt(1, (N, Ca, D, H, W)) + 0.3).bfloat16().float()
    srcs = [(xa, stats(xa).float())]
    if Cb:
        xb = rt(2, (N, Cb, D, H, W)) * 1.5 - 0.2
        xb = (torch.relu(xb) if b_raw else xb).bfloat16().float()
        srcs.append((xb, None if b_raw else stats(xb).float()))
    Cin = Ca + Cb
    O = [(s + 1) // 2 if stride == 2 else s for s in (D, H, W)]
    return dict(srcs=srcs, stride=stride,
                w1=rt(3, (Cout, Cin, 3, 3, 3), 1.0 / math.sqrt(27 * Cin)),
                ws=rt(4, (Cout, Cin, 3, 3, 3), 1.0 / math.sqrt(27 * Cin)) if has_sc else None,
                w2=rt(5, (Cout, Cout, 3, 3, 3), 1.0 / math.sqrt(27 * Cout)),
                dout=rt(6, (N, Cout, *O)).bfloat16().float())


def count_ties(name):
    """[(ties, elements)] of the two masks a case evaluates: its sources against their statistics, and y1 -- emulated here as bf16(float64 conv1) with
    the statistics of those values; the GPU test counts again on the tensors the device stored."""
    inp = make_inputs(name)
    srcs, Cout = inp['srcs'], inp['w1'].shape[0]
    y1 = conv_fwd(x_hat_cat(srcs), [inp['w1']], inp['stride'])[0].float().bfloat16().float()
    t0, t1 = relu_mask(srcs)[1], relu_mask([(y1, stats(y1).float())])[1]
    return [(int(t0.sum()), t0.numel()), (int(t1.sum()), t1.numel())]


def chain(srcs, w1, w2, ws, dout, stride=1, exact=True, store=lambda t: t):
    """The whole block by chaining the stage functions on their own outputs (`store` is what a stage's result goes through before the next one reads it:
    the identity here, a bf16 rounding in an emulation).  srcs: [(xa, mra), (xb, mrb)?].  Returns a dict of every stage's value."""
    has_sc = ws is not None
    Cout = w1.shape[0]
    x = torch.cat([s[0] for s in srcs], 1)
    r = {}
    xh = x_hat_cat(srcs, exact)
    ys = store(conv_fwd(xh, [w1, ws] if has_sc else [w1], stride, exact=exact)[0])
    y1, sc = ys[:, :Cout], (ys[:, Cout:] if has_sc else x.double())
    mr_y1 = stats(y1)
    y1h = x_hat(y1, mr_y1, exact)
    r['ys'], r['mr_y1'] = ys, mr_y1
    r['out'] = store(conv_fwd(y1h, [w2], 1, res=sc, exact=exact)[0])
    r['mr_out'] = stats(r['out'])
    g1 = store(dgrad([dout], [w2], [(y1, mr_y1)], 1, exact)[0])
    gm1 = bwd_means(g1, y1, mr_y1)
    dy1 = store(tail(g1, y1, mr_y1, gm1)[0])
    r['g1'], r['gm1'], r['dy1'] = g1, gm1, dy1
    g0 = store(dgrad([dy1, dout] if has_sc else [dy1], [w1, ws] if has_sc else [w1], srcs, stride, exact)[0])
    r['g0'] = g0
    dxs, c0 = [], 0
    for k, (xs, mr) in enumerate(srcs):
        g = g0[:, c0:c0 + xs.shape[1]]
        c0 += xs.shape[1]
        if mr is None:
            dxs.append(g)
            continue
        gm = bwd_means(g, xs, mr)
        r['gm0' + 'ab'[k]] = gm
        dxs.append(store(tail(g, xs, mr, gm, add=None if has_sc else dout)[0]))
    r['dx'] = dxs
    r['dw2'] = wgrad(y1h, dout)
    r['dw1'] = wgrad(xh, dy1, stride)
    if has_sc:
        r['dws'] = wgrad(xh, dout, stride)
    return r


def autograd_block(srcs, w1, w2, ws, dout, stride=1):
    """The block as the model writes it (model/dim3/conv_layers.py BasicBlock, pre-activation: F.instance_norm(eps=1e-4), F.relu, F.conv3d), in the dtype
    of its inputs, and torch.autograd through it: the independent statement the chained stages are proven against."""
    xs = [x.clone().requires_grad_(True) for x, _ in srcs]
    xh = torch.cat([x if mr is None else F.relu(F.instance_norm(x, eps=1e-4)) for x, (_, mr) in zip(xs, srcs)], 1)
    w1, w2 = w1.clone().requires_grad_(True), w2.clone().requires_grad_(True)
    ws = ws.clone().requires_grad_(True) if ws is not None else None
    y1 = F.conv3d(xh, w1, stride=stride, padding=1)
    y1.retain_grad()
    sc = F.conv3d(xh, ws, stride=stride, padding=1) if ws is not None else torch.cat(xs, 1)
    out = F.conv3d(F.relu(F.instance_norm(y1, eps=1e-4)), w2, padding=1) + sc
    out.backward(dout)
    r = dict(ys=torch.cat([y1, sc], 1).detach() if ws is not None else y1.detach(), out=out.detach(), dy1=y1.grad, dx=[x.grad for x in xs],
             dw1=w1.grad, dw2=w2.grad)
    if ws is not None:
        r['dws'] = ws.grad
    return r
