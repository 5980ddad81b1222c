#!/usr/bin/env python3
"""Times of the Models Genesis pretext pair (baselines/model_genesis/utils.py generate_pair_batch, kernels csrc/genesis.hip) for a batch of 2 volumes
at 96^3, split by which transforms fired in every sample:

    nothing       normalise, map back                                                              2 launches
    flips         D and H flipped                                                                  2 launches
    shuffle       10000 blocks, sides 1 .. 9, permutations drawn on the device                     4 launches
    shuffle_host  the same blocks with permutations drawn on the host and uploaded                 4 launches
    curve         the Bezier curve through 100000 float64 knots                                    2 launches
    inpaint / outpaint    five boxes, noise from the in-kernel generator                           2 launches
    everything    flips, shuffle, curve, out-painting                                              4 launches

Per plan: `device_ms` = the kernels alone (median, min over --reps, device events around the registered operator with the plan's arrays already on
the device), `call_ms` = generate_pair_batch as the training loop calls it (host wall clock to completion: upload of the blocks and knots included),
`cpu_ref_ms_per_sample` = tests/genesis_ref.py for ONE sample of the same plan on the host (numpy, what a loader worker would spend; for the device-drawn
plans it also restates the Philox draws, so read `shuffle_host` / `curve` / `nothing` for the cost of the reference's own arithmetic).
`host_plan_ms` = plan_genesis_pair(2, 96^3) at the reference's rates, median over 20 draws, and with every transform forced to fire.

    python tools/bench_genesis.py [--reps 20] [--batch 2] [--out profiles/genesis_bench.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, 'tests')):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPE = (96, 96, 96)
NUM_BLOCK = 10000


def _device_ms(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        ts.append(a.elapsed_time(b))
    return [float(np.median(ts)), float(min(ts))]


def _wall_ms(fn, reps):
    ts = []
    for _ in range(reps + 1):
        torch.cuda.synchronize()
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t) * 1e3)
    return [float(np.median(ts[1:])), float(min(ts[1:]))]


def plans(mg, B):
    rs = np.random.RandomState(0)
    sz = np.array(SHAPE)
    n = rs.randint(1, sz // 10 + 1, size=(NUM_BLOCK, 3))
    blocks = np.concatenate([rs.randint(0, sz - n + 1), n], axis=1)
    perms = [rs.permutation(int(np.prod(q[3:]))) for q in blocks]
    ctl = ((0.25, 0.8), (0.7, 0.15), False)
    inb, outb = [], []
    for _ in range(5):
        m = rs.randint(sz // 6, sz // 3 + 1)
        inb.append(tuple(int(v) for v in np.concatenate([rs.randint(3, sz - m - 3 + 1), m])))
        m = sz - rs.randint(3 * sz // 7, 4 * sz // 7 + 1)
        outb.append(tuple(int(v) for v in np.concatenate([rs.randint(3, sz - m - 3 + 1), m])))
    every = lambda **kw: mg.make_genesis_plan(B, SHAPE, seed=list(range(1, B + 1)), **{k: [v] * B for k, v in kw.items()})
    return {'nothing': every(), 'flips': every(flip=(True, True, False)), 'shuffle': every(blocks=blocks),
            'shuffle_host': every(blocks=blocks, perms=perms), 'curve': every(control=ctl), 'inpaint': every(paint='in', boxes=inb),
            'outpaint': every(paint='out', boxes=outb),
            'everything': every(flip=(True, True, False), blocks=blocks, control=ctl, paint='out', boxes=outb)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--reps', type=int, default=20)
    ap.add_argument('--batch', type=int, default=2)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'genesis_bench.json'))
    a = ap.parse_args()
    import genesis_ref as GR
    from rsuper_amd.baselines import model_genesis as mg
    from rsuper_amd.baselines.model_genesis import utils
    from rsuper_amd.hip import lib
    lib.require_device()
    B = a.batch
    img = torch.randn((B, 1) + SHAPE, device='cuda', generator=torch.Generator(device='cuda').manual_seed(0))
    host = img[0, 0].cpu().numpy()
    out = {'metric': 'Models Genesis pretext pair: device / call / CPU restatement times, ms', 'unit': 'ms',
           'case': {'batch': B, 'shape': list(SHAPE), 'num_block': NUM_BLOCK, 'knots': utils.N_KNOTS},
           'device_ms': {}, 'call_ms': {}, 'launches': {}, 'cpu_ref_ms_per_sample': {}, 'host_plan_ms': {}}
    mg.generate_pair_batch(img, mg.make_genesis_plan(B, SHAPE))            # registers the operator
    for name, plan in plans(mg, B).items():
        blk, perm, off, curve = utils._plan_tensors(plan, img.device)
        boxes = []
        for b in range(B):
            flat = [v for q in plan.boxes[b] for v in q]
            boxes += flat + [0] * (lib.GENESIS_MAX_BOXES * 6 - len(flat))
        nbytes = lib.lib().rsuper_genesis_workspace_bytes(B, *SHAPE, NUM_BLOCK)
        ws = torch.empty((nbytes,), device='cuda', dtype=torch.uint8)
        args = (img, plan.flags, blk, perm, off, curve, [len(q) for q in plan.boxes], boxes, plan.seed, None, ws)
        out['device_ms'][name] = _device_ms(lambda: torch.ops.rsuper.genesis_pair(*args), a.reps)
        out['call_ms'][name] = _wall_ms(lambda: mg.generate_pair_batch(img, plan), a.reps)
        out['launches'][name] = mg.genesis_launches(plan)
        ts = []
        for _ in range(3):
            t = time.perf_counter()
            GR.apply_plan(host, plan, 0)
            ts.append((time.perf_counter() - t) * 1e3)
        out['cpu_ref_ms_per_sample'][name] = float(np.median(ts))
    for name, kw in (('reference_rates', {}), ('everything_fires', dict(flip_rate=1.0, local_rate=1.0, nonlinear_rate=1.0, paint_rate=1.0))):
        ts = []
        for s in range(20):
            t = time.perf_counter()
            mg.plan_genesis_pair(B, SHAPE, seed=s, **kw)
            ts.append((time.perf_counter() - t) * 1e3)
        out['host_plan_ms'][name] = [float(np.median(ts)), float(min(ts))]
    line = json.dumps(out)
    print(line, flush=True)
    with open(a.out, 'w') as f:
        f.write(line + '\n')


if __name__ == '__main__':
    main()
