"""BasicBlockFn's bf16 chain (hip/ops.py: _BB.forward, _forward_s2, _backward_s1, _backward_s2), stage by stage against float64 -- TEACHER FORCED: every stage
is compared with tests/block_stage_ref.py evaluated on the tensors the previous stage actually STORED on the device, so a flipped ReLU mask or a rounding
difference cannot travel down the chain and each stage keeps the derivable bound the single kernels are held to (gpu_checks.check_conv_exact):

    GEMM stages (ys, out, g1, g0)        |got - ref| <= 2^-8 |ref| + (K / 8 + 4) 2^-24 mag            K = reduction length of the launch
    statistics (mr_y1, mr_out, gm1, gm0) 1e-4 of the column's rms (of rstd), against float64 sums over the stored tensor
    tails (dy1, dxa, dxb)                |got - ref| <= 2^-8 |ref| + 8 x 2^-24 mag,  mag = rstd (|g| + |m1| + |x_n m2|) [+ |dout|]
    weight gradients                     max-norm 3e-3 of the tensor's max (check_wgrad_sliced_dy's number, on the stored operands)

Every figure is reported as a ratio to its bound (<= 1).  The stored tensors are captured by spies on the module attributes of rsuper_amd.hip.ops that _BB's
methods look up at call time; the spies change nothing (asserted bit for bit once).  Each case asserts from the spy record and from ops.igemm_plan WHICH path
it took, so that a later dispatch change cannot quietly turn it into a copy of another case.  A voxel whose f32 (x - mean) rstd is exactly 0 (a tie of the
ReLU mask) is left out of the g1 / g0 comparison; the reference alone decides that, and the share is capped at 1e-4 (0 for every seeded case:
tests/test_block_stage_ref_cpu.py).  Lazy tails are covered bit for bit by tests/test_gpu_lazy_tails.py: the cases here hand over plain statistics tensors.
"""
import ctypes
import inspect
import os
import sys

import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_stage_ref as R  # noqa: E402
import gpu_checks as gc  # noqa: E402

pytestmark = pytest.mark.gpu

SPIED = ('igemm', 'igemm_s2', 'stats_finalize', 'flush_wgrad_reduces', 'in_bwd_finalize', 'wgrad', 'wgrad_s2')
BF16 = torch.bfloat16


class Spies:
    """Wrappers around the launch helpers of hip/ops.py: call the original, keep its arguments (by name) and its result.  Host-side queries only besides."""

    def __init__(self, ops, setattr_):
        self.ops, self.calls = ops, []
        for name in SPIED:
            setattr_(ops, name, self._wrap(name, getattr(ops, name)))

    def _wrap(self, name, orig):
        sig = inspect.signature(orig)

        def spy(*a, **kw):
            args = sig.bind(*a, **kw)
            args.apply_defaults()
            rec = dict(args.arguments, fn=name)
            if name == 'flush_wgrad_reduces':
                rec['deferred'] = len(self.ops._DEFERRED)
            if name == 'wgrad':                      # the plans, while the variant / threshold the case forces is in effect (host-only queries)
                rec['plan'] = _wgrad_plan(self.ops, rec)
            if name == 'igemm':
                rec['plan'] = _igemm_plan(self.ops, rec)
            self.calls.append(rec)
            rec['ret'] = orig(*a, **kw)
            return rec['ret']
        return spy

    def of(self, name, **match):
        return [c for c in self.calls if c['fn'] == name and all(c[k] == v for k, v in match.items())]


def _wgrad_plan(ops, c):
    xa, xb, ya, yb = c['xa'], c['xb'], c['ya'], c['yb']
    plan = (ctypes.c_int * 4)()
    mixed = xb is not None and (xa.mr is None) != (xb.mr is None)
    rc = ops._L().rsuper_conv3_wgrad_plan(ops._DT[xa.t.dtype], ops.use_tr(), xa.C, 0 if xb is None else xb.C, ya.C, 0 if yb is None else yb.C, *c['dims'],
                                          1 if mixed else 0, 0, plan)
    assert rc == 0
    return tuple(plan)


def _igemm_plan(ops, c):
    a, b = c['a'], c['b']
    mixed = b is not None and (a.mr is None) != (b.mr is None)
    return ops.igemm_plan(a.t.dtype, c['epi'], c['dims'], c['n_cols'], c['bn'], mixed, a.C, 0 if b is None else b.C)


def _run_block(name, dt, setattr_=None):
    """One forward + backward of the case on the device.  Returns (device results, spies or None, the CPU operands)."""
    from rsuper_amd.hip import ops
    inp = R.make_inputs(name)
    ops._BLOCK_PACK_CACHE.clear()             # a forced variant must not meet another variant's plan
    spies = Spies(ops, setattr_) if setattr_ is not None else None
    xs = [gc.to_cl(x, dt).requires_grad_(True) for x, _ in inp['srcs']]
    mrs = [None if mr is None else mr.to(gc.DEV) for _, mr in inp['srcs']]
    w1, w2 = inp['w1'].to(gc.DEV).requires_grad_(True), inp['w2'].to(gc.DEV).requires_grad_(True)
    ws = inp['ws'].to(gc.DEV).requires_grad_(True) if inp['ws'] is not None else None
    dout = gc.to_cl(inp['dout'], dt)
    try:
        out, mr_out = ops.BasicBlockFn.apply(xs[0], mrs[0], xs[1] if len(xs) > 1 else None, mrs[1] if len(xs) > 1 else None, w1, w2, ws, None, inp['stride'])
        out.backward(dout)
        torch.cuda.synchronize()
    finally:
        ops._BLOCK_PACK_CACHE.clear()
    got = dict(out=out.detach(), mr_out=mr_out, dx=[x.grad for x in xs], dw1=w1.grad, dw2=w2.grad, dws=None if ws is None else ws.grad, dout=dout)
    return got, spies, inp


def _nc(t):
    return gc.from_cl(t).double()


def _src(s):
    """The channels a Src names, as a CPU (N, C, D, H, W) float64 tensor."""
    return _nc(s.t[..., s.off:s.off + s.C])


def _same(a, b):
    return a.t.data_ptr() == b.t.data_ptr() and (a.off, a.C, a.ld) == (b.off, b.C, b.ld) and (a.mr is None) == (b.mr is None) and \
        (a.mr is None or a.mr.data_ptr() == b.mr.data_ptr())


def _gemm_ratio(got, ref, mag, K, skip=None):
    bound = 2.0 ** -8 * ref.abs() + (K / 8 + 4) * 2.0 ** -24 * mag + 1e-30
    ratio = (got - ref).abs() / bound
    ratio = torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf')))
    if skip is not None:
        ratio = torch.where(skip, torch.zeros_like(ratio), ratio)
    return ratio.max().item()


def _tail_ratio(got, ref, mag):
    # one bf16 rounding of the result + 8 f32 roundings: the six to seven f32 operations of in_bwd_tail (x - mu, * rs, g - m1, x_n * m2, the second
    # subtraction, * rs) and the add of dOut, each at most 2^-24 of a partial result that mag bounds
    ratio = (got - ref).abs() / (2.0 ** -8 * ref.abs() + 8 * 2.0 ** -24 * mag + 1e-30)
    return torch.where(torch.isfinite(ratio), ratio, torch.full_like(ratio, float('inf'))).max().item()


def _stats_ratio(fin, y):
    """(mean, rstd) a launch emitted against float64 sums over the tensor it wrote: 1e-4 of the column's rms / of rstd (check_conv_exact)."""
    fin, ref = fin.detach().cpu().double(), R.stats(y)
    rms = (y * y).mean(dim=(2, 3, 4)).sqrt().clamp_min(1e-30)
    e = max(((fin[..., 0] - ref[..., 0]).abs() / rms).max().item(), (fin[..., 1] / ref[..., 1] - 1.0).abs().max().item())
    return (e if e == e else float('inf')) / 1e-4


def _means_ratio(gm, g, x, mr):
    gm, ref = gm.detach().cpu().double(), R.bwd_means(g, x, mr)
    rms = (g * g).mean(dim=(2, 3, 4)).sqrt().clamp_min(1e-30)
    e = ((gm - ref).abs() / rms[..., None]).max().item()
    return (e if e == e else float('inf')) / 1e-4


def _wgrad_ratio(got, ref):
    e = gc.relerr(got.detach().cpu(), ref)
    return (e if e == e else float('inf')) / 3e-3


def _judge(name, got, sp, inp):
    """Every stage of the recorded run against float64 on the stored tensors.  Returns (ratios per stage, facts about the path taken)."""
    N, S, Ca, Cb, Cout, has_sc, b_raw, stride, _ = R.CASES[name]
    srcs, w1, w2, ws = inp['srcs'], inp['w1'], inp['w2'], inp['ws']
    Cin = Ca + Cb
    r, facts = {}, {}
    cpu_mr = lambda t: t.detach().cpu()             # noqa: E731
    # ---- forward.  [y1 | shortcut] is what conv1's launch WROTE (one interleaved tensor, or two under the split output); conv2 is the forward launch with a
    # residual.  Where conv2 reads its residual from is judged by the `out` stage, not assumed.
    conv2 = [c for c in sp.of('igemm', epi=0) if c['res'] is not None]
    assert len(conv2) == 1
    conv2 = conv2[0]
    first = sp.calls[0]
    assert first['fn'] in (('igemm', 'igemm_s2') if stride == 2 else ('igemm',))
    facts['split_ys'] = first.get('out2') is not None
    if first['fn'] == 'igemm':
        facts['conv1_plan'] = first['plan']
    y1_src, mr_y1 = conv2['a'], cpu_mr(conv2['a'].mr)
    y1 = _src(y1_src)
    if stride == 2 and first['fn'] == 'igemm':        # the stride-1 evaluation: conv1 wrote the full grid, subsample2 made the tensor conv2 reads
        wrote = _nc(y1_src.t)
    else:
        assert first['out'].data_ptr() == y1_src.t.data_ptr() and (y1_src.off, y1_src.C) == (0, Cout)     # conv2 normalises the y1 conv1 wrote
        wrote = torch.cat([_nc(first['out']), _nc(first['out2'])], 1) if facts['split_ys'] else _nc(first['out'])
    if facts['split_ys']:
        assert first['out_split'] == Cout and first['out'].shape[-1] == first['out2'].shape[-1] == Cout
    assert wrote.shape[1] == Cout * (2 if has_sc else 1) and torch.equal(wrote[:, :Cout], y1)
    ys = wrote
    dout = _nc(got['dout'])
    xh = R.x_hat_cat(srcs)
    ref, mag = R.conv_fwd(xh, [w1, ws] if has_sc else [w1], stride)
    r['ys'] = _gemm_ratio(ys, ref, mag, 27 * Cin)
    r['mr_y1'] = _stats_ratio(mr_y1, y1)
    y1h = R.x_hat(y1, mr_y1)
    ref, mag = R.conv_fwd(y1h, [w2], 1, res=ys[:, Cout:] if has_sc else srcs[0][0])
    out = _nc(got['out'])
    assert conv2['out'].data_ptr() == got['out'].data_ptr()
    r['out'] = _gemm_ratio(out, ref, mag, 27 * Cout)
    r['mr_out'] = _stats_ratio(got['mr_out'], out)
    # ---- backward, conv2: g1, its means, the tail
    dg = sp.of('igemm', epi=1)
    tails = sp.of('in_bwd_finalize')
    g1c = dg[0]
    assert _same(g1c['ea'], y1_src) and g1c['a'].t.data_ptr() == got['dout'].data_ptr() and g1c['eb'] is None
    g1 = _nc(g1c['out'])
    ref, mag, ties = R.dgrad([dout], [w2], [(y1, mr_y1)])
    facts['ties'] = [int(ties.sum())]
    assert ties.sum().item() <= 1e-4 * ties.numel()
    r['g1'] = _gemm_ratio(g1, ref, mag, 27 * Cout, skip=ties)
    t1 = tails[0]
    assert t1['g'].t.data_ptr() == g1c['out'].data_ptr() and _same(t1['x'], y1_src) and t1['add1'] is None
    gm1 = cpu_mr(t1['gm'])
    r['gm1'] = _means_ratio(gm1, g1, y1, mr_y1)
    dy1 = _nc(t1['ret'])
    r['dy1'] = _tail_ratio(dy1, *R.tail(g1, y1, mr_y1, gm1))
    # ---- backward, conv1 (+ shortcut): g0 in one or two launches (igemm epi 1 / the strided kernel; a raw source's launch is a plain epi 0 GEMM)
    g0c = dg[1:] + sp.of('igemm_s2', mode=2) + [c for c in sp.of('igemm', epi=0) if c['res'] is None and c is not first]
    for c in g0c:
        if stride == 1:
            assert c['a'].t.data_ptr() == t1['ret'].data_ptr() and (c['b'] is None) == (not has_sc)
            assert c['b'] is None or c['b'].t.data_ptr() == got['dout'].data_ptr()
    facts['g0_launches'] = [(c['fn'], c.get('epi', c.get('mode')), c['n_cols'], 0 if c['ea'] is None else 1, 0 if c.get('eb') is None else 1) for c in g0c]
    g0 = torch.cat([_nc(c['out']) for c in g0c], 1)
    assert g0.shape[1] == Cin
    ref, mag, ties = R.dgrad([dy1, dout] if has_sc else [dy1], [w1, ws] if has_sc else [w1], srcs, stride)
    facts['ties'].append(int(ties.sum()))
    assert ties.sum().item() <= 1e-4 * ties.numel()
    r['g0'] = _gemm_ratio(g0, ref, mag, 27 * Cout * (2 if has_sc else 1), skip=ties)
    # ---- the tails of the sources (the identity block adds dOut before the single rounding)
    fl = sp.of('flush_wgrad_reduces')
    facts['stats_rode'] = bool(fl) and fl[0]['stats'] is not None and fl[0]['deferred'] >= 2
    c0, k = 0, 1
    for i, (x, mr) in enumerate(srcs):
        C = x.shape[1]
        g = g0[:, c0:c0 + C]
        c0 += C
        tag = 'ab'[i]
        if mr is None:
            assert torch.equal(_nc(got['dx'][i]), g)                      # a raw source: the data gradient IS its gradient
            continue
        t = tails[k]
        k += 1
        assert torch.equal(_src(t['g']), g) and torch.equal(_src(t['x']), x.double()) and torch.equal(cpu_mr(t['x'].mr), mr)
        assert t['add1'] is None or t['add1'].data_ptr() == got['dout'].data_ptr()
        gm = cpu_mr(t['gm'])
        assert tuple(gm.shape) == (N, C, 2), f'gm0{tag}: the table of the InstanceNorm-backward means has shape {tuple(gm.shape)}, not {(N, C, 2)}'
        r['gm0' + tag] = _means_ratio(gm, g, x.double(), mr)
        assert torch.equal(t['ret'], got['dx'][i])                        # what the tail stored is the gradient autograd hands on
        r['dx' + tag] = _tail_ratio(_nc(t['ret']), *R.tail(g, x.double(), mr, gm, add=None if has_sc else dout))
    assert k == len(tails)
    # ---- weight gradients on the stored operands
    r['dw2'] = _wgrad_ratio(got['dw2'], R.wgrad(y1h, dout))
    r['dw1'] = _wgrad_ratio(got['dw1'], R.wgrad(xh, dy1, stride))
    if has_sc:
        r['dws'] = _wgrad_ratio(got['dws'], R.wgrad(xh, dout, stride))
    facts['wgrad_kernels'] = [c['plan'][0] for c in sp.of('wgrad')]
    return r, facts


def _report(label, r, facts):
    line = f'{label}: ' + ' '.join(f'{k} {v:.3f}' if v >= 1e-3 else f'{k} {v:.0e}' for k, v in r.items()) + f' | {facts}'
    print(line)
    table = os.environ.get('RSUPER_BLOCK_STAGES_TABLE')       # a file to collect the lines of a run in (profiles/block_stages.txt was measured this way)
    if table:
        with open(table, 'a') as f:
            f.write(line + '\n')
    return line


def _variant(v):
    from rsuper_amd.hip import ops
    return ops._L().rsuper_conv3_variant(v)


def _stages(name, monkeypatch, variant=3, wgrad_tiles=None, env=None, label=None):
    """Run case `name` in bf16 under a forced igemm variant / weight-gradient threshold / environment, judge every stage.  Returns (ratios, facts, line)."""
    from rsuper_amd.hip import ops
    L = ops._L()
    old_env = {k: os.environ.get(k) for k in (env or {})}
    old_thr = L.rsuper_conv3_wgrad2_min_tiles(-1)
    try:
        os.environ.update(env or {})
        L.rsuper_conv3_variant(variant)
        if wgrad_tiles is not None:
            L.rsuper_conv3_wgrad2_min_tiles(wgrad_tiles)
        with monkeypatch.context() as m:
            got, sp, inp = _run_block(name, BF16, m.setattr)
    finally:
        L.rsuper_conv3_variant(3)
        L.rsuper_conv3_wgrad2_min_tiles(old_thr)
        for k, v in old_env.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    r, facts = _judge(name, got, sp, inp)
    line = _report(label or f'{name} v{variant}', r, facts)
    return r, facts, line, sp


def _assert_ratios(r, line):
    bad = {k: v for k, v in r.items() if not v <= 1.0}
    assert not bad, f'first stage over its bound: {next(iter(bad))} -- {line}'


def _forced_kernel(variant):
    from rsuper_amd.hip import lib
    return {0: lib.IGEMM_CLASSIC, 1: lib.IGEMM_PC, 4: lib.IGEMM_WS, 6: lib.IGEMM_BOX, 7: lib.IGEMM_BOX, 8: lib.IGEMM_KD}.get(variant)


def _assert_s1_path(name, variant, facts, sp):
    """What every stride-1 case proves about its path: conv1's kernel under a forced variant, the split output exactly where expected, the joint data
    gradient (or one launch per source), and the InstanceNorm-backward rows riding in the batched slab reduction with both weight gradients deferred."""
    from rsuper_amd.hip import lib
    N, S, Ca, Cb, Cout, has_sc, b_raw, stride, _ = R.CASES[name]
    want, nc1 = _forced_kernel(variant), Cout * (2 if has_sc else 1)
    kd = variant == 8 and nc1 > 32 and not b_raw       # the depth-reuse kernel takes more than 32 columns and two sources of one kind only
    if variant == 8:
        assert (facts['conv1_plan'][0] == lib.IGEMM_KD) == kd, (variant, facts)
    elif want is not None:
        assert facts['conv1_plan'][0] == want, (variant, facts)
    # the split output: bf16, a shortcut, 32 output channels, and the plan hands conv1 to the depth-reuse kernel (forced by variant 8 at these sizes)
    assert facts['split_ys'] == (kd and has_sc and Cout == 32), facts
    assert facts['stats_rode'], facts
    assert len(sp.of('stats_finalize', mode=1)) == 1                    # gm1 alone has a launch of its own; gm0 came back from the slab reduction
    fl = sp.of('flush_wgrad_reduces')[0]
    assert len(fl['stats']) == len(fl['ret']) and all(s[2] == 1 for s in fl['stats'])
    if Cb and not b_raw and len(facts['g0_launches']) == 1:
        assert fl['stats'][0][3] == Ca and len(fl['ret'][0]) == 2       # the joint table split at the first source's channels
    if b_raw:
        assert facts['g0_launches'] == [('igemm', 1, Ca, 1, 0), ('igemm', 0, Cb, 0, 0)], facts


# ================================================================================================ the spies change nothing
def test_spies_change_no_bit(monkeypatch):
    a, _, _ = _run_block('A', BF16)
    with monkeypatch.context() as m:
        b, sp, _ = _run_block('A', BF16, m.setattr)
    assert sp.calls and {c['fn'] for c in sp.calls} == {'igemm', 'stats_finalize', 'flush_wgrad_reduces', 'in_bwd_finalize', 'wgrad'}
    for k in ('out', 'mr_out', 'dw1', 'dw2', 'dws'):
        assert torch.equal(a[k], b[k]), k
    for x, y in zip(a['dx'], b['dx']):
        assert torch.equal(x, y)
    from rsuper_amd.hip import ops
    assert all(getattr(ops, n).__name__ != 'spy' for n in SPIED)          # and they are gone again


# ================================================================================================ A: two normalised sources + shortcut
@pytest.mark.parametrize('variant', [3, 0, 1, 4, 6, 7, 8])
def test_case_a_decoder_head_every_variant(monkeypatch, variant):
    r, facts, line, sp = _stages('A', monkeypatch, variant)
    _assert_s1_path('A', variant, facts, sp)
    assert facts['g0_launches'] == [('igemm', 1, 96, 1, 1)], facts        # the joint data gradient: both sources' masks in one launch
    _assert_ratios(r, line)


@pytest.mark.parametrize('kind', ['wgrad2', 'classic'])
def test_case_a_weight_gradient_kernels(monkeypatch, kind):
    from rsuper_amd.hip import lib
    r, facts, line, sp = _stages('A', monkeypatch, 3, wgrad_tiles=0 if kind == 'wgrad2' else 1 << 20, label=f'A {kind}')
    # conv2's weight gradient (32 -> 32) is one the second-generation kernel supports; the two-source one of conv1 + shortcut stays on the tile-streaming kernel
    assert facts['wgrad_kernels'] == ([lib.WGRAD_2, lib.WGRAD_TILE] if kind == 'wgrad2' else [lib.WGRAD_TILE, lib.WGRAD_TILE]), facts
    _assert_s1_path('A', 3, facts, sp)
    _assert_ratios(r, line)


def test_case_a_data_gradient_per_source(monkeypatch):
    """A': ops.split_dgrad_sources with its tile threshold at 0, every other condition kept (bf16, two sources, 32 | 64 channels, a joint width of 32).
    At A's own size the joint launch is under-filled and takes 64-column blocks, so this runs at A2, the nearest size where the plan answers 32."""
    from rsuper_amd.hip import ops
    N, S, Ca, Cb = R.CASES['A2'][:4]
    tiles = ops._L().rsuper_conv3_tiles(*S) * N
    joint = ops.pick_bn(Ca + Cb, BF16, tiles, (N, *S), epi=1)
    if joint != 32:
        pytest.skip(f'the joint data gradient of {Ca}+{Cb} columns at {S} takes {joint}-column blocks, not 32: split_dgrad_sources keeps one launch there')

    def split0(Ca_, Cb_, dtype, tiles_total, bn_joint):
        if os.environ.get('RSUPER_SPLIT_DGRAD', '1') == '0' or dtype == torch.float32 or not Cb_:
            return False
        return bn_joint == 32 and Ca_ % 32 == 0 and Cb_ % 64 == 0 and tiles_total is not None and tiles_total >= 0
    monkeypatch.setattr(ops, 'split_dgrad_sources', split0)
    r, facts, line, sp = _stages('A2', monkeypatch, 3, label="A' per-source dgrad (A2)")
    assert facts['g0_launches'] == [('igemm', 1, Ca, 1, 0), ('igemm', 1, Cb, 1, 0)], facts       # two epi 1 launches with one `ea` each
    fl = sp.of('flush_wgrad_reduces')[0]
    assert len(fl['stats']) == 2 and [s[3] for s in fl['stats']] == [0, 0] and fl['deferred'] >= 2
    _assert_s1_path('A2', 3, facts, sp)
    _assert_ratios(r, line)


# ================================================================================================ B: one source + shortcut, split output under variant 8
@pytest.mark.parametrize('variant', [3, 8])
def test_case_b_shortcut_and_split_output(monkeypatch, variant):
    r, facts, line, sp = _stages('B', monkeypatch, variant)
    _assert_s1_path('B', variant, facts, sp)
    _assert_ratios(r, line)


# ================================================================================================ C: identity shortcut (the tail adds dOut)
@pytest.mark.parametrize('variant', [3, 0, 1, 4, 8])
@pytest.mark.parametrize('name', ['C32a', 'C32b', 'C64a', 'C64b'])
def test_case_c_identity_tail(monkeypatch, name, variant):
    from rsuper_amd.hip import lib
    r, facts, line, sp = _stages(name, monkeypatch, variant)
    _assert_s1_path(name, variant, facts, sp)
    if name == 'C64b' and variant == 3:
        assert set(facts['wgrad_kernels']) == {lib.WGRAD_SV}, facts       # 12^3: the small-volume weight gradient by default
    _assert_ratios(r, line)
    assert [c['add1'] is not None for c in sp.of('in_bwd_finalize')] == [False, True]


# ================================================================================================ D: 6^3, the volume-fitted kernel
@pytest.mark.parametrize('variant', [3, 6, 7])
@pytest.mark.parametrize('name', ['D128', 'D64'])
def test_case_d_box_kernel_at_6_cubed(monkeypatch, name, variant):
    from rsuper_amd.hip import ops, lib
    r, facts, line, sp = _stages(name, monkeypatch, variant)
    plans = [c['plan'] for c in sp.of('igemm')]
    assert len(plans) == 4 and all(p[0] == lib.IGEMM_BOX for p in plans), plans
    # the split-reduction shape (one box per sample, the reduction split over blocks through the workspace the module registered) unless the 4x4x4 box is forced
    assert all((p[2] == 3 and p[3] >= 1) if variant != 7 else p[2] == 2 for p in plans), plans
    assert ops._WS is not None and facts['stats_rode'] and not facts['split_ys']
    _assert_ratios(r, line)


# ================================================================================================ E: one normalised and one raw source
@pytest.mark.parametrize('variant', [3, 8])
def test_case_e_mixed_sources_forward_and_backward(monkeypatch, variant):
    from rsuper_amd.hip import ops, lib
    N, S, Ca, Cb, Cout = R.CASES['E'][:5]
    r, facts, line, sp = _stages('E', monkeypatch, variant)
    if variant == 8:        # the plan refuses the depth-reuse kernel BECAUSE of the raw source: with two sources of one kind it takes this launch
        ops._L().rsuper_conv3_variant(8)
        try:
            assert ops.igemm_plan(BF16, 0, (N, *S), 2 * Cout, 0, False, Ca, Cb)[0] == lib.IGEMM_KD
            assert ops.igemm_plan(BF16, 0, (N, *S), 2 * Cout, 0, True, Ca, Cb)[0] != lib.IGEMM_KD
        finally:
            ops._L().rsuper_conv3_variant(3)
    assert facts['conv1_plan'][0] != lib.IGEMM_KD and not facts['split_ys']
    _assert_s1_path('E', variant, facts, sp)
    assert len(sp.of('in_bwd_finalize')) == 2                            # dy1 and the normalised source: the raw one has no tail
    _assert_ratios(r, line)


# ================================================================================================ G: stride 2
S2_ENVS = {'default': {}, 'stride-1 evaluation': {'RSUPER_S2_KERNEL': '0'}, 'parity-class kernels': {'RSUPER_S2K': '0', 'RSUPER_S2D': '0'}}


@pytest.mark.parametrize('env', sorted(S2_ENVS))
@pytest.mark.parametrize('name', ['G16', 'G32'])
def test_case_g_strided_block(monkeypatch, name, env):
    r, facts, line, sp = _stages(name, monkeypatch, 3, env=S2_ENVS[env], label=f'{name} {env}')
    strided = [c['mode'] for c in sp.of('igemm_s2')]
    assert strided == ([] if env == 'stride-1 evaluation' else [1, 2]), strided
    assert bool(sp.of('wgrad_s2')) == (env != 'stride-1 evaluation') and not sp.of('flush_wgrad_reduces')
    assert all(os.environ.get(k) is None for k in ('RSUPER_S2_KERNEL', 'RSUPER_S2K', 'RSUPER_S2D'))
    _assert_ratios(r, line)


# ================================================================================================ f32 mode: the whole block against float64 autograd
@pytest.mark.parametrize('name', ['A', 'C32a', 'C32b', 'C64a', 'C64b', 'E'])
def test_f32_block_matches_float64_autograd(name):
    """No teacher forcing, no spies: max-norm 2e-4 of each tensor's scale (check_basic_block's f32 tolerance)."""
    got, _, inp = _run_block(name, torch.float32)
    ref = R.autograd_block([(x.double(), mr) for x, mr in inp['srcs']], inp['w1'].double(), inp['w2'].double(),
                           None if inp['ws'] is None else inp['ws'].double(), inp['dout'].double(), inp['stride'])
    e = {'out': gc.relerr(gc.from_cl(got['out']), ref['out']), 'dw1': gc.relerr(got['dw1'].cpu(), ref['dw1']), 'dw2': gc.relerr(got['dw2'].cpu(), ref['dw2'])}
    for i, (g, rf) in enumerate(zip(got['dx'], ref['dx'])):
        e[f'dx{i}'] = gc.relerr(gc.from_cl(g), rf)
    if inp['ws'] is not None:
        e['dws'] = gc.relerr(got['dws'].cpu(), ref['dws'])
    _report(f'{name} f32 vs float64 autograd (max-norm / 2e-4)', {k: v / 2e-4 for k, v in e.items()}, {})
    assert all(v <= 2e-4 for v in e.values()), e


# ================================================================================================ F: the split output under the DEFAULT dispatch
def test_case_f_split_output_equals_interleaved_output_bit_for_bit():
    """rsuper_conv3_igemm_split_out against rsuper_conv3_igemm on the same 64 n + 32 n -> [32 | 32] operands at 2 x (32, 40, 80): 400 depth-reuse tiles, the
    smallest volume the default dispatch hands to that kernel.  Outputs and `part` start as NaN; both halves and every `part` row must be bit-equal, nothing
    may stay NaN, and the zeros behind each tensor must still be zeros."""
    from rsuper_amd.hip import ops, lib
    N, D, H, W, Ca, Cb, Cout, G = 2, 32, 40, 80, 64, 32, 32, 4096
    dims, nc, vox = (N, D, H, W), 2 * Cout, N * D * H * W
    plan = ops.igemm_plan(BF16, 0, dims, nc)
    assert plan[0] == lib.IGEMM_KD and plan[1] == 64, plan
    xa = (gc._rng_t(301, (N, Ca, D, H, W)) + 0.3).bfloat16().float()
    xb = (gc._rng_t(302, (N, Cb, D, H, W)) * 1.5 - 0.2).bfloat16().float()
    w1, ws = (gc._rng_t(s, (Cout, Ca + Cb, 3, 3, 3), (27 * (Ca + Cb)) ** -0.5).to(gc.DEV) for s in (303, 304))
    a = ops.Src(gc.to_cl(xa, BF16), mr=gc.stats_ref(xa).to(gc.DEV))
    b = ops.Src(gc.to_cl(xb, BF16), mr=gc.stats_ref(xb).to(gc.DEV))
    wp = ops.pack_weights(BF16, 0, w1, ws, Ca, Cb, Cout, Cout, plan[1])
    rows = plan[4]

    def buffers(sizes):
        """Tensors of `sizes` elements from ONE buffer, NaN-filled, each followed by a guard band of G zeros."""
        buf = torch.full((sum(sizes) + G * len(sizes),), float('nan'), device=gc.DEV, dtype=BF16)
        views, guards, o = [], [], 0
        for n in sizes:
            views.append(buf[o:o + n]); guards.append(buf[o + n:o + n + G]); o += n + G
        for g in guards:
            g.zero_()
        return views, guards

    def part_buffer():
        p = torch.full((N * rows * nc * 2 + G,), float('nan'), device=gc.DEV, dtype=torch.float32)
        p[-G:].zero_()
        return p[:-G].view(N, rows, nc, 2), p[-G:]
    (o1, o2), g_split = buffers([vox * Cout, vox * Cout])
    o1, o2 = o1.view(N, D, H, W, Cout), o2.view(N, D, H, W, Cout)
    p_split, pg_split = part_buffer()
    ops.igemm(0, a, b, wp, nc, plan[1], dims, o1, part=p_split, out2=o2, out_split=Cout)
    (oj,), g_joint = buffers([vox * nc])
    oj = oj.view(N, D, H, W, nc)
    p_joint, pg_joint = part_buffer()
    ops.igemm(0, a, b, wp, nc, plan[1], dims, oj, part=p_joint)
    torch.cuda.synchronize()
    for t in (o1, o2, oj, p_split, p_joint):
        assert bool(torch.isfinite(t).all())
    assert torch.equal(o1, oj[..., :Cout]) and torch.equal(o2, oj[..., Cout:])
    assert torch.equal(p_split, p_joint)
    for g in g_split + g_joint + [pg_split, pg_joint]:
        assert int(torch.count_nonzero(g)) == 0
