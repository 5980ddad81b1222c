"""tests/block_stage_ref.py against itself, on the CPU: before any kernel is judged by the stage references, their algebra is proven.  In float64 with NO
bf16 rounding anywhere, the stage functions chained on their own outputs must equal torch.autograd through the block written with F.instance_norm(eps=1e-4),
F.relu and F.conv3d (model/dim3/conv_layers.py BasicBlock, pre-activation) to 1e-10 of each tensor's max.  Also counts the ReLU-mask ties of every seeded
case of tests/test_gpu_block_stages.py (the share that test may exclude is capped at 1e-4; expected 0)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import block_stage_ref as R  # noqa: E402


def _inputs(N, S, Ca, Cb, Cout, has_sc, b_raw, stride, seed):
    g = torch.Generator().manual_seed(seed)

    def rt(*shape, scale=1.0):
        return torch.randn(*shape, generator=g, dtype=torch.float64) * scale
    xa = rt(N, Ca, *S) + 0.3
    srcs = [(xa, R.stats(xa))]
    if Cb:
        xb = rt(N, Cb, *S) * 1.5 - 0.2
        srcs.append((torch.relu(xb), None) if b_raw else (xb, R.stats(xb)))
    Cin = Ca + Cb
    O = [(s + 1) // 2 if stride == 2 else s for s in S]
    return dict(srcs=srcs, stride=stride, w1=rt(Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5), w2=rt(Cout, Cout, 3, 3, 3, scale=(27 * Cout) ** -0.5),
                ws=rt(Cout, Cin, 3, 3, 3, scale=(27 * Cin) ** -0.5) if has_sc else None, dout=rt(N, Cout, *O))


# one and two sources, with and without a shortcut, stride 1 and 2, odd sizes, a raw second source
ALGEBRA = [
    ('one source, identity', (2, (5, 7, 9), 8, 0, 8, False, False, 1, 1)),
    ('one source, shortcut', (1, (4, 6, 5), 8, 0, 16, True, False, 1, 2)),
    ('two sources, shortcut', (2, (5, 3, 7), 8, 16, 8, True, False, 1, 3)),
    ('two sources, second raw', (1, (3, 5, 6), 8, 8, 8, True, True, 1, 4)),
    ('stride 2, odd sizes', (2, (7, 5, 9), 8, 0, 16, True, False, 2, 5)),
    ('stride 2, even and odd sizes', (1, (6, 7, 4), 16, 0, 8, True, False, 2, 6)),
]


@pytest.mark.parametrize('case', ALGEBRA, ids=[c[0] for c in ALGEBRA])
def test_chained_stage_references_equal_autograd_in_float64(case):
    inp = _inputs(*case[1])
    got = R.chain(inp['srcs'], inp['w1'], inp['w2'], inp['ws'], inp['dout'], inp['stride'], exact=True)
    ref = R.autograd_block(inp['srcs'], inp['w1'], inp['w2'], inp['ws'], inp['dout'], inp['stride'])
    worst = {}
    for k, r in ref.items():
        for i, (a, b) in enumerate(zip(got[k], r) if isinstance(r, list) else [(got[k], r)]):
            assert a.shape == b.shape, (k, a.shape, b.shape)
            worst[f'{k}{i}'] = ((a - b).abs().max() / b.abs().max()).item()
    assert max(worst.values()) <= 1e-10, worst


def test_magnitudes_bound_their_references():
    """mag is the sum of the absolute values of the terms: |ref| <= mag elementwise, with equality where every term has one sign."""
    inp = _inputs(1, (4, 5, 6), 8, 8, 8, True, False, 1, 7)
    xh = R.x_hat_cat(inp['srcs'], exact=True)
    ref, mag = R.conv_fwd(xh, [inp['w1'], inp['ws']], exact=True)
    assert bool((ref.abs() <= mag * (1 + 1e-5)).all())
    gref, gmag, ties = R.dgrad([inp['dout'], inp['dout']], [inp['w1'], inp['ws']], inp['srcs'], exact=True)
    assert bool((gref.abs() <= gmag * (1 + 1e-5)).all()) and int(ties.sum()) == 0
    x, mr = inp['srcs'][0]
    g = gref[:, :8]
    tref, tmag = R.tail(g, x, mr, R.bwd_means(g, x, mr), add=x)
    assert bool((tref.abs() <= tmag * (1 + 1e-12)).all())
    ones = torch.ones_like(xh)
    r1, m1 = R.conv_fwd(ones, [inp['w1'].abs()], exact=True)
    assert torch.allclose(r1, m1, rtol=1e-5)


def test_bf16_prologue_and_weights_are_rounded_unless_exact():
    inp = _inputs(1, (3, 4, 5), 8, 0, 8, False, False, 1, 8)
    x, mr = inp['srcs'][0]
    x = x.float().bfloat16().float()
    xh = R.x_hat(x, mr.float())
    assert bool((xh == xh.float().bfloat16().double()).all()) and bool((xh >= 0).all())
    assert float((xh - R.x_hat(x, mr.float(), exact=True)).abs().max()) <= 2.0 ** -8 * float(xh.abs().max()) + 1e-6
    w = inp['w1']
    a = R.conv_fwd(xh, [w])[0]
    b = R.conv_fwd(xh, [w.float().bfloat16().double()], exact=True)[0]
    assert torch.equal(a, b)


@pytest.mark.parametrize('name', sorted(R.CASES))
def test_seeded_cases_have_no_relu_mask_ties(name):
    counts = R.count_ties(name)
    print(f'block stages case {name}: mask ties (sources, y1) = {[c[0] for c in counts]} of {[c[1] for c in counts]} elements')
    for ties, n in counts:
        assert ties <= 1e-4 * n, (name, counts)


def test_seeded_inputs_are_bf16_values_with_f32_statistics():
    inp = R.make_inputs('E')
    (xa, mra), (xb, mrb) = inp['srcs']
    assert mrb is None and bool((xb >= 0).all()) and mra.dtype == torch.float32
    for t in (xa, xb, inp['dout']):
        assert torch.equal(t, t.bfloat16().float())
    assert np.isfinite(mra.numpy()).all()
