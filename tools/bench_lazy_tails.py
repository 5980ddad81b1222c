#!/usr/bin/env python3
"""Lazy InstanceNorm backward tails at the UNet step's shapes (B = 2, 96^3, base 32): rsuper_in_bwd_finalize + the consuming backward kernel against
the fused launch (rsuper_maxpool2_bwd_lazy with both gradients lazy, rsuper_upsample_bwd_lazy), each timed alone over back-to-back launches.
rsuper_lazy_tails(2) admits the fused kernels at every shape they can take, whatever the rule in csrc/lazy_tail_plan.hpp says.  The kernels' times
inside the step (other cache contents) come from a kernel trace of bench.py; this is the quick A/B."""
import os, sys, torch
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from rsuper_amd.hip import ops
L = ops._L()
assert L.rsuper_lazy_tails(2) == 2
BF, N = 1, 2


def timeit(fn, it=20):
    fn(); torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(it):
        fn()
    e.record(); torch.cuda.synchronize()
    return s.elapsed_time(e) / it * 1e3


def rnd(*shape):
    return torch.randn(*shape, device='cuda').bfloat16()


def tables(C):
    return torch.rand(N, C, 2, device='cuda') + 0.5, torch.randn(N, C, 2, device='cuda') * 0.1


print('max-pool backward, both gradients lazy')
for S, C in ((96, 32), (48, 64), (24, 128), (12, 256)):
    O = S // 2
    x, ga, gy = rnd(N, S, S, S, C), rnd(N, S, S, S, C), rnd(N, O, O, O, C)
    y, mry = ops._maxpool_fwd(x)
    (mrx, gmx), (_, gmy) = tables(C), tables(C)
    dx = torch.empty_like(x)
    fin = [None, None]

    def tail_a():
        fin[0] = ops.in_bwd_finalize(ops.Src(ga), ops.Src(x, mr=mrx), gmx, C)

    def tail_y():
        fin[1] = ops.in_bwd_finalize(ops.Src(gy), ops.Src(y, mr=mry), gmy, C)

    def pool():
        L.rsuper_maxpool2_bwd_add(BF, x.data_ptr(), C, fin[1].data_ptr(), C, fin[0].data_ptr(), C, dx.data_ptr(), C, N, S, S, S, C, None)

    def fused():
        assert L.rsuper_maxpool2_bwd_lazy(BF, x.data_ptr(), C, gy.data_ptr(), C, mry.data_ptr(), gmy.data_ptr(), ga.data_ptr(), C, mrx.data_ptr(),
                                          gmx.data_ptr(), dx.data_ptr(), C, N, S, S, S, C, None) == 0
    ta, ty, tp, tf = timeit(tail_a), timeit(tail_y), timeit(pool), timeit(fused)
    print(f'{S}^3 x {C:3d}: tails {ta:6.1f} + {ty:5.1f} us, maxpool_bwd_add {tp:6.1f} us = {ta + ty + tp:6.1f} us | fused {tf:6.1f} us')

print('trilinear backward, lazy gradient')
for S, C in ((96, 64), (48, 128), (24, 256), (12, 320)):
    I = S // 2
    g, u = rnd(N, S, S, S, C), rnd(N, S, S, S, C)
    mr, gm = tables(C)
    dx = torch.empty(N, I, I, I, C, device='cuda', dtype=torch.bfloat16)
    fin = [None]

    def tail():
        fin[0] = ops.in_bwd_finalize(ops.Src(g), ops.Src(u, mr=mr), gm, C)

    def plain():
        L.rsuper_upsample_bwd(BF, fin[0].data_ptr(), C, dx.data_ptr(), C, N, I, I, I, S, S, S, C, None)

    def fused():
        assert L.rsuper_upsample_bwd_lazy(BF, g.data_ptr(), C, u.data_ptr(), C, mr.data_ptr(), gm.data_ptr(), dx.data_ptr(), C, N, I, I, I, S, S, S, C, None) == 0
    t0, t1, tf = timeit(tail), timeit(plain), timeit(fused)
    print(f'{I}^3 -> {S}^3 x {C:3d}: tail {t0:6.1f} us + upsample_bwd {t1:6.1f} us = {t0 + t1:6.1f} us | fused {tf:6.1f} us')
