#!/usr/bin/env python3
"""Golden vectors for the Models Genesis pretext pairs, produced by the UNMODIFIED reference `baselines/model_genesis/utils.py`
(generate_one_pair :206-266) under seeded `random` / `np.random` generators.  Run in the authoring container only:

    RSUPER_REFERENCE=<checkout of the reference>/rsuper_train python tests/golden/gen_golden_genesis.py

Import shims: `imageio` and `skimage.transform` are only touched by code outside this path, so empty modules are registered for them.
While generate_one_pair runs, random.random / random.randint / random.choice / np.random.shuffle / np.random.rand are wrapped to record what they
return (np.random.shuffle shuffles an index vector with the generator -- the same draws -- and applies it, which gives the permutation as source
positions), and the module's bezier_curve is wrapped to record the knots.  The recorded trace is then read along generate_one_pair's control flow
into the plan of the case.

Writes tests/golden/genesis.npz (data only).  input_A / input_B: the two (D, H, W) f32 inputs.  Per case k: shape_k ('A' / 'B'), seed_k, rates_k (the
five rates passed), flip_k (3 bools: net flip of D, H, W), draws_k (the flip axes as drawn, the reference's axes 0, 1, 2 of the (1, D, H, W) sample),
[blocks_k (nb, 6) u8 (z0, y0, x0, nz, ny, nx), perm_k: the source positions of all blocks, concatenated, u8], [control_k (2, 2) f64, sort_both_k,
knots_sha_k: sha256 of the unsorted xvals and yvals bytes, knots_every_k (2, 100) every 1000th knot], [paint_k 'in' / 'out', boxes_k (n, 6),
noise_k (D, H, W) f32: the recorded rand arrays composed in write order], x_k, y_k: the reference's pair (f32)."""
import hashlib
import importlib
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = {'A': (17, 19, 23), 'B': (20, 24, 30)}
NUM_BLOCK = 10000
# name, shape, (flip, local, nonlinear, paint, inpaint) rates, what the first accepted seed must show
CASES = [
    ('nothing', 'A', (0.0, 0.0, 0.0, 0.0, 0.0), lambda p: True),
    ('flips', 'B', (0.9, 0.0, 0.0, 0.0, 0.0), lambda p: len(p['draws']) == 3 and len(set(p['draws'])) == 2 and 0 not in p['draws'] and any(p['flip'])),
    ('flip_twice', 'A', (0.9, 0.0, 0.0, 0.0, 0.0), lambda p: sorted(p['draws']) in ([1, 1], [2, 2])),
    ('shuffle', 'B', (0.0, 1.0, 0.0, 0.0, 0.0), lambda p: True),
    ('curve_x_sorted', 'A', (0.0, 0.0, 1.0, 0.0, 0.0), lambda p: not p['sort_both']),
    ('curve_both_sorted', 'A', (0.0, 0.0, 1.0, 0.0, 0.0), lambda p: p['sort_both']),
    ('inpaint', 'A', (0.0, 0.0, 0.0, 1.0, 1.0), lambda p: len(p['boxes']) >= 3),
    ('outpaint', 'A', (0.0, 0.0, 0.0, 1.0, 0.0), lambda p: len(p['boxes']) >= 2),
    ('everything', 'A', (0.9, 1.0, 1.0, 1.0, 0.2), lambda p: p['flip'][0] and p['paint'] == 'out'),
]


def case_input(name):
    """(D, H, W) f32: white noise on a ramp, in a CT-like range after the loader's normalisation."""
    D, H, W = SHAPES[name]
    rs = np.random.RandomState(2000 + ord(name))
    z = np.linspace(-1.0, 1.0, D)[:, None, None]
    return (rs.standard_normal((D, H, W)) * 0.6 + 0.8 * z).astype(np.float32)


def import_reference():
    ref = os.environ.get('RSUPER_REFERENCE')
    if not ref or not os.path.isdir(ref):
        raise SystemExit('set RSUPER_REFERENCE to the reference checkout\'s rsuper_train directory')
    for name in ('imageio', 'skimage', 'skimage.transform'):
        sys.modules.setdefault(name, types.ModuleType(name))
    sys.modules['skimage.transform'].resize = None
    sys.path.insert(0, ref)
    return importlib.import_module('baselines.model_genesis.utils')


class Record:
    """Wraps the five generator functions and the module's bezier_curve while active; `trace` holds (kind, value) in call order."""

    def __init__(self, mg):
        self.mg = mg

    def __enter__(self):
        self.trace, self.knots = [], []
        self._orig = (random.random, random.randint, random.choice, np.random.shuffle, np.random.rand, self.mg.bezier_curve)
        o_random, o_randint, o_choice, o_shuffle, o_rand, o_bezier = self._orig

        def w_random():
            v = o_random()
            self.trace.append(('random', v))
            return v

        def w_randint(a, b):
            v = o_randint(a, b)
            self.trace.append(('randint', v))
            return v

        def w_choice(seq):
            v = o_choice(seq)
            self.trace.append(('choice', v))
            return v

        def w_shuffle(a):
            idx = np.arange(len(a))
            o_shuffle(idx)                               # the draws depend on the length alone
            a[:] = a[idx]
            self.trace.append(('shuffle', idx))

        def w_rand(*shape):
            v = o_rand(*shape)
            self.trace.append(('rand', v))
            return v

        def w_bezier(points, nTimes=1000):
            xv, yv = o_bezier(points, nTimes=nTimes)
            self.knots.append((points, xv.copy(), yv.copy()))
            return xv, yv

        random.random, random.randint, random.choice, np.random.shuffle, np.random.rand, self.mg.bezier_curve = (
            w_random, w_randint, w_choice, w_shuffle, w_rand, w_bezier)
        return self

    def __exit__(self, *exc):
        random.random, random.randint, random.choice, np.random.shuffle, np.random.rand, self.mg.bezier_curve = self._orig


def read_plan(trace, knots, shape, rates):
    """The recorded calls of one generate_one_pair on one sample -> its plan, following the function's control flow."""
    flip_rate, local_rate, nonlinear_rate, paint_rate, inpaint_rate = rates
    it = iter(trace)

    def take(kind):
        k, v = next(it)
        assert k == kind, (k, kind)
        return v

    p = dict(draws=[], flip=[False] * 3, blocks=None, perms=None, control=None, sort_both=None, paint=None, boxes=[], noise=None)
    cnt = 3
    while take('random') < flip_rate and cnt > 0:        # data_augmentation
        axis = take('choice')
        p['draws'].append(axis)
        if axis > 0:                                     # axis 0 of the (1, D, H, W) sample is the channel
            p['flip'][axis - 1] = not p['flip'][axis - 1]
        cnt -= 1
    if not take('random') >= local_rate:                 # local_pixel_shuffling
        blocks, perms = [], []
        for _ in range(NUM_BLOCK):
            n = [take('randint') for _ in range(3)]
            c = [take('randint') for _ in range(3)]
            blocks.append(c + n)
            perms.append(take('shuffle'))
            assert len(perms[-1]) == n[0] * n[1] * n[2]
        p['blocks'], p['perms'] = np.array(blocks), perms
    if not take('random') >= nonlinear_rate:             # nonlinear_transformation
        c = [take('random') for _ in range(4)]
        p['control'] = np.array([[c[0], c[1]], [c[2], c[3]]])
        p['sort_both'] = not take('random') < 0.5
        assert len(knots) == 1 and knots[0][0] == [[0, 0], [c[0], c[1]], [c[2], c[3]], [1, 1]]
    if take('random') < paint_rate:
        noise = np.zeros(shape, np.float32)

        def box(sub):
            n = [take('randint') for _ in range(3)]
            if sub:                                      # out-painting draws what it takes off the side
                n = [s - v for s, v in zip(shape, n)]
            c = [take('randint') for _ in range(3)]
            return c + n

        if take('random') < inpaint_rate:                # image_in_painting
            p['paint'], cnt = 'in', 5
            while cnt > 0 and take('random') < 0.95:
                b = box(False)
                r = take('rand')
                assert r.shape == tuple(b[3:])
                noise[b[0]:b[0] + b[3], b[1]:b[1] + b[4], b[2]:b[2] + b[5]] = r
                p['boxes'].append(b)
                cnt -= 1
        else:                                            # image_out_painting
            p['paint'], cnt = 'out', 4
            r = take('rand')
            assert r.shape == (1,) + tuple(shape)
            noise[:] = r[0]
            p['boxes'].append(box(True))
            while cnt > 0 and take('random') < 0.95:
                p['boxes'].append(box(True))
                cnt -= 1
        p['noise'] = noise
    assert next(it, None) is None, 'calls left over: the trace was not read as generate_one_pair made it'
    return p


def run_case(mg, img, rates, seed):
    random.seed(seed)
    np.random.seed(seed)
    with Record(mg) as rec:
        x, y = mg.generate_one_pair(img.copy(), *rates)
    assert x.shape == img.shape and y.shape == img.shape
    return read_plan(rec.trace, rec.knots, img.shape, rates), rec.knots, x.astype(np.float32), y.astype(np.float32), x.dtype


def main():
    mg = import_reference()
    out = {'n_cases': np.array(len(CASES)), 'names': np.array([c[0] for c in CASES])}
    inputs = {k: case_input(k) for k in SHAPES}
    for k, v in inputs.items():
        out['input_' + k] = v
    for k, (name, shape, rates, accept) in enumerate(CASES):
        for seed in range(1000):
            p, knots, x, y, dt = run_case(mg, inputs[shape], rates, seed)
            if accept(p):
                break
        else:
            raise SystemExit('case %s: no seed below 1000 shows it' % name)
        assert dt == np.float32
        out['shape_%d' % k], out['seed_%d' % k], out['rates_%d' % k] = np.array(shape), np.array(seed), np.array(rates)
        out['flip_%d' % k], out['draws_%d' % k] = np.array(p['flip']), np.array(p['draws'], np.int64)
        if p['blocks'] is not None:
            out['blocks_%d' % k] = p['blocks'].astype(np.uint8)
            out['perm_%d' % k] = np.concatenate(p['perms']).astype(np.uint8)
        if p['control'] is not None:
            _, xv, yv = knots[0]
            out['control_%d' % k], out['sort_both_%d' % k] = p['control'], np.array(p['sort_both'])
            out['knots_sha_%d' % k] = np.array(hashlib.sha256(xv.tobytes() + yv.tobytes()).hexdigest())
            out['knots_every_%d' % k] = np.stack([xv[::1000], yv[::1000]])
        if p['paint'] is not None:
            out['paint_%d' % k], out['boxes_%d' % k], out['noise_%d' % k] = np.array(p['paint']), np.array(p['boxes']).reshape(-1, 6), p['noise']
        out['x_%d' % k], out['y_%d' % k] = x, y
        print('case %d %-18s shape %s seed %3d: flips %s draws %s, %s blocks, curve %s, paint %s %d boxes' % (
            k, name, shape, seed, p['flip'], p['draws'], 0 if p['blocks'] is None else len(p['blocks']),
            None if p['control'] is None else ('both sorted' if p['sort_both'] else 'x sorted'), p['paint'], len(p['boxes'])))
    path = os.path.join(HERE, 'genesis.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'kB')
    assert os.path.getsize(path) < 1000 * 1000


if __name__ == '__main__':
    main()
