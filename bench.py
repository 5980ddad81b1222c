#!/usr/bin/env python3
"""bench.py -- throughput of the R-Super training hot path on MI355X.

    python bench.py --gpus N --steps K --warmup W        (N > 1 without WORLD_SIZE: re-executes itself under
                                                          torch.distributed.run, one rank per GPU)
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P bench.py --gpus N ...

One step = one iteration of train_epoch (rsuper_train/train_ddp.py:308-357) on a synthetic batch already resident
in HBM: zero_grad -> UNet forward -> calculate_loss -> backward -> clip_grad_norm_(1.0) -> AdamW -> EMA.
Workload = BASELINE.json configs[1]: full R-Super 3D UNet (base 32, 26 PanTS classes, 40.56 M parameters), bf16,
96^3 patches, batch 2 per GPU, segmentation loss (masked BCE + adaptive-Tversky Dice), report losses off.
Rank 0 prints ONE JSON line; `value` = voxels processed by all ranks / max-over-ranks time of the K timed steps.

The timed region contains nothing but the K steps (no event records).  A plain run stops there: set-up, W warm-up steps,
the K timed steps, the outputs (--dump-outputs DIR), the JSON line.  With --full the roofline numbers come from a separate
pass AFTER it (same model, same batch, HIP events around every conv MFMA launch on the launch stream); at N = 1 further
short legs report config 3 (report supervision), the f32 parity mode and the cost of bf16 (`secondary`), then the CPU baseline.

--dump-outputs DIR writes what the last timed step handed its caller and left in the model, as .npy files (rank 0): every
loss term and the pre-clip gradient norm (float64), and a fixed seeded sample of the updated parameters, their EMA and
their gradients (float32, DUMP_SAMPLE elements each, in parameter order).  Weights and batch are seeded: the same
arguments give the same inputs in every run.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests', 'golden'))

MFMA_PEAK_TFLOPS = {'bf16': 2500.0, 'f32': 157.3}     # dense, /opt/skills/guides/MI355X_MICROARCH.md
# Fabric-side bytes (FETCH_SIZE x2 + WRITE_SIZE) of the conv MFMA launches of ONE default step are read from this file
# (written by tools/pmc_step_summary.py from the rocprofv3 --pmc passes of tools/pmc_step.sh; see its "source" key).
TRAFFIC_PROFILE = os.path.join(ROOT, 'profiles', 'conv_traffic.json')
DUMP_SAMPLE = 1 << 22          # elements per sampled array of --dump-outputs: 3 x 16 MiB of float32 (40.56 M parameters at base 32)


def conv_stack_flops(base, S, B):
    """Algorithmic FLOPs of the 43 3x3x3 convolutions of UNet(base) per forward (2*MACs), SURVEY.md section 8(d)."""
    b = base
    ch = [b, 2 * b, 4 * b, 8 * b, 10 * b]
    total = 0.0

    def blk(ci, co, s):
        n = 2.0 * B * s ** 3 * 27
        t = n * ci * co + n * co * co
        if ci != co:
            t += n * ci * co
        return t
    total += blk(b, b, S)
    s = S
    for i in range(4):
        s //= 2
        total += blk(ch[i], ch[i + 1], s) + blk(ch[i + 1], ch[i + 1], s)
    for i in range(4):
        s *= 2
        ci, co = ch[4 - i], ch[3 - i]
        total += blk(ci + co, co, s) + blk(co, co, s)
    return total


def loss_args(report):
    return argparse.Namespace(loss='ball_dice_both' if report else 'ball_dice_last', aux_weight=[0.5, 0.5], seg_loss=1.0,
                              report_volume_loss_basic=0.1 if report else 0.0, volume_loss_tolerance=0.2,
                              ball_bce_weight=1.0, ball_dice_weight=1.0, ball_volume_margin=0.2, multi_ch_tumor=False,
                              stardard_ce_ball=False, classification_branch=False, ema=True, ema_alpha=0.99)


def cpu_baseline(args, classes):
    """Oracle (CPU restatement of the reference, kind='port') timed on the host cores as BASELINE.md section 3 prescribes: the complete training
    step of train_epoch (train_ddp.py:308-357: zero_grad, forward, seg loss, backward, clip, AdamW, EMA) on the bench's own configuration (batch
    `--batch`, `--size`^3, base, classes) with the batch resident in memory, one warm-up step of the same shape, then >= 3 timed steps."""
    from oracle import unet_oracle as uo, losses_oracle as lo, train_oracle as to
    import synth
    ncores = min(os.cpu_count(), 32)      # ATen CPU conv3d stops scaling (and thrashes) far below 256 threads
    torch.set_num_threads(ncores)
    la = loss_args(False)
    B, S, base, nsteps = args.batch, args.size, args.base, max(3, args.cpu_baseline_steps)
    shapes = uo.unet_param_shapes(1, base, len(classes))
    sd = {k: torch.from_numpy(v).requires_grad_(True) for k, v in synth.fill_state_dict(shapes, 3).items()}
    params = list(sd.values())
    ema = [p.detach().clone() for p in params]
    opt = to.AdamW([p.detach() for p in params], lr=6e-4, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.05)
    img = torch.from_numpy(synth.image(B, S, seed=1234))
    bt = {k: torch.from_numpy(v) for k, v in synth.batch(B, S, classes, ['mask'] * B, seed=7).items()}

    def step(i):
        t0 = time.time()
        for p_ in params:
            p_.grad = None
        r = uo.unet_forward(sd, img)
        res = lo.calculate_loss({'segmentation': r}, bt['label'], bt['unk_channels'], la, bt['mask'], bt['volumes'], bt['diameters'], classes)
        res['overall'].backward()
        grads = [p_.grad for p_ in params]
        with torch.no_grad():
            to.clip_grad_norm_(grads, 1.0)
            opt.step(grads)
            to.update_ema(opt.params, ema, 0.99, i)
        return time.time() - t0
    t_warm = step(0)
    ts = [step(i + 1) for i in range(nsteps)]
    dt = sum(ts) / len(ts)
    return {'value': B * S ** 3 / dt, 'unit': 'voxels/s', 'cores': ncores, 'kind': 'port',
            'sample': f'{nsteps} timed full training steps (fwd + seg loss + bwd + clip + AdamW + EMA) of the fp32 torch-CPU oracle after 1 warm-up step of the '
                      f'same shape, B={B}, {S}^3, base {base}, {len(classes)} classes, {ncores} threads: mean {dt:.1f} s/step '
                      f'(min {min(ts):.1f}, max {max(ts):.1f}, warm-up {t_warm:.1f})'}


def dump_outputs(leg, out_dir):
    """The results of the leg's last step as DIR/<name>.npy (see the module docstring)."""
    os.makedirs(out_dir, exist_ok=True)
    losses, gnorm = leg.last
    arrays = {f'loss_{k}': np.asarray(torch.as_tensor(v).detach().double().cpu()) for k, v in losses.items() if v is not None}
    if gnorm is not None:
        arrays['grad_norm'] = np.asarray(torch.as_tensor(gnorm).detach().double().cpu())
    params = list(leg.net.parameters())
    n = sum(p.numel() for p in params)
    idx = np.arange(n) if n <= DUMP_SAMPLE else np.sort(np.random.default_rng(0).choice(n, size=DUMP_SAMPLE, replace=False))
    idx = torch.from_numpy(idx).to(params[0].device)

    def sample(ts):
        return torch.cat([t.detach().float().reshape(-1) for t in ts]).index_select(0, idx).cpu().numpy()
    with torch.no_grad():
        arrays['params_sample'] = sample(params)
        arrays['ema_params_sample'] = sample(list(leg.ema.parameters()))
        grads = [p.grad for p in params]
        if any(g is None for g in grads):
            raise RuntimeError('--dump-outputs: a parameter has no gradient after the last timed step')
        arrays['grads_sample'] = sample(grads)
    for name, a in arrays.items():
        np.save(os.path.join(out_dir, name + '.npy'), a)


def respawn_under_torchrun(args):
    """`python bench.py --gpus N` with N > 1 and no launcher environment: start one rank per GPU ourselves
    (train_ddp.py:726 uses mp.spawn; torchrun gives the same RANK/LOCAL_RANK/WORLD_SIZE/MASTER_* contract)."""
    s = socket.socket()
    s.bind(('127.0.0.1', 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, '-m', 'torch.distributed.run', '--nnodes=1', f'--nproc-per-node={args.gpus}',
           '--master-addr', '127.0.0.1', '--master-port', str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env.setdefault('HSA_ENABLE_IPC_MODE_LEGACY', '0')
    env.setdefault('OMP_NUM_THREADS', str(max(1, (os.cpu_count() or 8) // max(args.gpus, 1))))
    return subprocess.call(cmd, env=env)


class Leg:
    """One model + optimiser + resident synthetic batch of the bench workload."""

    def __init__(self, args, dtype, report, rank, world, local, force_ddp, classes, B, S, medformer=False, seed=0):
        import synth
        from rsuper_amd.model.dim3.unet import UNet
        from rsuper_amd.train_ddp import wrap_ddp, make_ema
        from rsuper_amd.training.utils import FusedAdamWEMA
        dev = f'cuda:{local}'
        torch.manual_seed(seed)              # identical random-init weights on every rank and in every leg (seed > 0: the ensemble members of secondary.bf16_vs_f32)
        if medformer:       # config/abdomenatlas_ufo/medformer_3d.yaml: the network R-Super trains, deep supervision on
            from rsuper_amd.model.dim3.medformer import MedFormer
            self.net = MedFormer(1, len(classes), base_chan=args.base, map_size=[3, 3, 3], conv_num=[2, 0, 0, 0, 0, 0, 2, 2],
                                 trans_num=[0, 2, 4, 6, 4, 2, 0, 0], num_heads=[1, 4, 8, 10, 8, 4, 1, 1], fusion_depth=2, fusion_dim=320,
                                 fusion_heads=10, expansion=4, aux_loss=True, compute_dtype=dtype).to(dev)
        else:
            self.net = UNet(1, args.base, num_classes=len(classes), block='BasicBlock', norm='in', compute_dtype=dtype,
                            pool=not getattr(args, 'no_pool', False)).to(dev)
        self.ema = make_ema(self.net)
        self.model = wrap_ddp(self.net, local) if (world > 1 or force_ddp) else self.net
        self.opt = FusedAdamWEMA(self.net.parameters(), lr=6e-4, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.05)
        kinds = (['mask', 'report'] * B)[:B] if report else ['mask'] * B
        bt = synth.batch(B, S, classes, kinds, seed=7 + rank + seed, diam_range=(5.0, 40.0), max_tumors=3)
        if getattr(args, 'unpacked_labels', False):      # A/B: the three volumes as uint8 planes (rounds 1-5)
            vols = dict(label=torch.from_numpy(bt['label']).to(dev), unk_channels=torch.from_numpy(bt['unk_channels']).to(dev), mask=torch.from_numpy(bt['mask']).to(dev))
        else:
            # the dataset's own storage form (np.packbits over the class axis, dataset_abdomenatlas_UFO.py:955,970,975) resident in HBM: what
            # train_epoch hands calculate_loss (dataset/packed.py ingest_packed_batch(keep_packed=True)); the loss kernels read the bits
            from rsuper_amd.training.dataset import pack_bits, PackedBits
            vols = {k: PackedBits(torch.from_numpy(pack_bits(bt[k])).to(dev), len(classes)) for k in ('label', 'unk_channels', 'mask')}
        self.batch = dict(image=torch.from_numpy(synth.image(B, S, seed=1234 + rank + seed)).to(dev),
                          volumes=torch.from_numpy(bt['volumes']).to(dev), diameters=torch.from_numpy(bt['diameters']).to(dev), **vols)
        self.largs = loss_args(report)
        self.classes = classes
        self.step = 0
        self.world = world
        self.last = None
        self.graphed = None
        self.sanity = False
        self.guard = None           # train_ddp.StepGuard: the reference's per-step guards as device flags, read one step late

    def run(self, n):
        from rsuper_amd.train_ddp import train_step
        for _ in range(n):
            if self.guard is not None:
                self.guard.check_input(self.batch['image'])
            if self.sanity:        # the reference's per-step guards, as train_epoch runs them (train_ddp.py:311-313; the loss's own at losses_foundation.py:864-869, 1070-1071)
                img = self.batch['image']
                assert not torch.isnan(img).any(), 'Input is nan'
                assert torch.max(img) <= 100, f'Input is bigger than 100: {torch.max(img)}'
                assert torch.min(img) >= -100, f'Input is smaller than -100: {torch.min(img)}'
            if self.graphed is not None:
                self.last = self.graphed(self.batch, self.step)
            else:
                self.last = train_step(self.model, self.ema, self.opt, self.batch, self.largs, self.classes, self.step)
            if self.guard is not None:
                self.guard.end_step()
                self.guard.poll()          # raises for the step before this one (its flags have landed while this step was being queued)
            self.step += 1

    def use_graph(self):
        """Replay the step from a hipGraph (rsuper_amd.graph): same kernels, one host launch per step."""
        from rsuper_amd.graph import GraphedTrainStep
        self.graphed = GraphedTrainStep(self.net, self.ema, self.opt, self.largs, self.classes, warmup=3)

    def use_net_graphs(self):
        """Forward and backward of the network from two hipGraphs around the eager loss / optimiser: the form that also covers report
        supervision (host-synchronous ball search in the loss)."""
        from rsuper_amd.graph import GraphedNetwork
        self.model = GraphedNetwork(self.net, warmup=3)

    def sync(self):
        if self.world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def timed(self, steps, warmup):
        self.run(warmup)
        self.sync()
        t0 = time.perf_counter()
        self.run(steps)
        self.sync()
        return time.perf_counter() - t0

    def loss(self):
        v = float(self.last[0]['overall'].detach())
        if not np.isfinite(v):
            raise ValueError('loss is nan, propagating this can destroy the network weights, STOP!')
        return v

    def logits(self):
        with torch.no_grad():
            return self.net(self.batch['image'])['segmentation'].float()

    def close(self):
        red = getattr(self.net, '_rsuper_reducer', None)
        if red is not None:
            red.remove()


def secondary_legs(args, rank, world, local, classes, B, S):
    """The workloads / modes the headline does not show (N = 1 only): config 3, hipGraph replay, MedFormer, the f32 parity mode and the
    cost of bf16.  Runs in a child process (`--secondary-only`): a failure here must never take the headline JSON line down with it;
    inside, every leg is guarded separately."""
    sec = {}
    n2, w2 = min(args.steps, 20), min(args.warmup, 5)
    headline_steps = args.steps + args.warmup + args.roofline_steps

    def leg_of(*a, **kw):
        return Leg(args, *a, rank, world, local, False, classes, B, S, **kw)

    def guarded(name, fn):
        try:
            fn()
        except Exception as e:                           # noqa: BLE001
            sec[name + '_error'] = repr(e)[:300]
        torch.cuda.empty_cache()

    def config3():
        l3 = leg_of(args.dtype, True)
        sec['config3_ms_per_step'] = l3.timed(n2, w2) / n2 * 1e3
        sec['config3_final_loss'] = l3.loss()
        sec['config3_workload'] = 'same UNet + Volume + Ball report losses (ball_dice_both, weight 0.1, 50/50 mask/report batch), BASELINE configs[2]'
        l3.close()

    def nopool():
        # UNet(..., pool=False): the strided BasicBlock down blocks (conv3d_igemm_s2k / _s2d / wgrad_s2) instead of max-pool + stride-1 blocks
        import copy
        a2 = copy.copy(args)
        a2.no_pool = True
        ln = Leg(a2, args.dtype, False, rank, world, local, False, classes, B, S)
        sec['nopool_ms_per_step'] = ln.timed(n2, w2) / n2 * 1e3
        sec['nopool_final_loss'] = ln.loss()
        sec['nopool_workload'] = 'headline workload with down_block(pool=False): strided [conv1 | shortcut] convolutions (unet_utils.py:38-39) instead of max-pooling'
        ln.close()

    def sanity_on():
        # the headline step with the reference's per-step guards active (input NaN / range asserts, the mask / volume consistency checks and the
        # NaN guard on the loss): each is a device -> host read that drains the launch queue; the headline keeps them outside the timed region
        from rsuper_amd.training import losses_foundation as lf
        ls = leg_of(args.dtype, False)
        ls.sanity = True
        lf.SANITY_CHECKS = True
        try:
            sec['sanity_on_ms_per_step'] = ls.timed(n2, w2) / n2 * 1e3
            sec['sanity_on_note'] = ('headline workload with SANITY_CHECKS on: isnan / max / min of the input (train_ddp.py:311-313), unk / volume consistency '
                                     '(losses_foundation.py:864-869) and the loss NaN guard that raises (:1070-1071) inside every timed step')
        finally:
            lf.SANITY_CHECKS = False
        ls.close()

    def graph():
        # the same step replayed from a hipGraph (one host launch per step instead of ~330); results are bit-identical to the eager step
        # (tests/test_gpu_edge.py::test_graphed_step_matches_eager)
        lg = leg_of(args.dtype, False)
        lg.use_graph()
        sec['graph_ms_per_step'] = lg.timed(n2, w2 + 24) / n2 * 1e3
        sec['graph_final_loss'] = lg.loss()
        lg.close()

    def medformer_graph():
        lmg = leg_of(args.dtype, False, medformer=True)
        lmg.use_graph()
        nm = min(n2, 10)
        # 3 eager warm-up steps + 13 replays: the step's self-verification against an eager step (replays 1 and 12, rsuper_amd/graph.py) falls
        # into the warm-up; the timed replays are 14 .. 23
        sec['medformer_graph_ms_per_step'] = lmg.timed(nm, 16) / nm * 1e3
        lmg.close()

    def medformer():
        lm = leg_of(args.dtype, False, medformer=True)
        nm = min(n2, 10)
        sec['medformer_ms_per_step'] = lm.timed(nm, 3) / nm * 1e3
        sec['medformer_final_loss'] = lm.loss()
        sec['medformer_workload'] = ('MedFormer of config/abdomenatlas_ufo/medformer_3d.yaml (37.9 M parameters, deep supervision), same batch and '
                                     'segmentation loss: conv stem / BasicBlock stages / up-sampling / head / depthwise / InstanceNorm on the HIP kernels, '
                                     'every 1x1x1 convolution / linear layer of the attention stages (forward, data and weight gradient) on the HIP pointwise MFMA GEMMs; '
                                     'the SemanticMapFusion transformer attention core on its own HIP kernel; round 6: the 27-token semantic-map product (as a slab-reduced dy^T x) and the 26-class aux head (padded to 28 columns) '
                                     'on the same pointwise kernels -- no library GEMM is left on the default path (SURVEY 8f-1)')
        lm.close()

    def medformer_roofline():
        # the attention stages' dominant product class is HBM-bound (K, N <= 1280 against 10^3..10^5 fp32 rows): the MBConv expand projection of the
        # 24^3 stage (27648 rows, 128 -> 512) forward / data gradient / weight gradient, HIP-event timed on the launch stream, against 8 TB/s
        from rsuper_amd.hip import ops as _ops
        R, K, N = 2 * 24 ** 3, 128, 512
        dev = torch.device('cuda', local)
        x = torch.randn(R, K, device=dev); w = torch.randn(N, K, device=dev) / K ** 0.5; dy = torch.randn(R, N, device=dev)
        comp = torch.bfloat16 if args.dtype == 'bf16' else torch.float32

        def t(fn, it=20):
            fn(); torch.cuda.synchronize()
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(it):
                fn()
            b.record(); torch.cuda.synchronize()
            return a.elapsed_time(b) / it * 1e-3
        gb = (R * K + R * N + N * K) * 4 / 1e9                         # every operand once, fp32 storage
        legs = {'forward': t(lambda: _ops.pointwise_gemm(x, w, None, 0, comp)), 'dgrad': t(lambda: _ops.pointwise_gemm(dy, w, None, 1, comp)),
                'wgrad': t(lambda: _ops.pointwise_wgrad(dy, x, False, comp))}
        tot = sum(legs.values())
        sec['medformer_roofline'] = {'kernel': 'pw_gemm / pw_wgrad (csrc/pointwise.hip), MBConv expand 128 -> 512 at 24^3 x 2 = 27648 rows', 'bound': 'hbm',
                                     'achieved': 3 * gb / tot, 'peak': 8000.0, 'unit': 'GB/s', 'frac': 3 * gb / tot / 8000.0,
                                     'per_pass_us': {k: v * 1e6 for k, v in legs.items()}, 'algorithmic_bytes_per_pass': gb * 1e9,
                                     'note': 'launch-inclusive (weight packing, slab reduce); each pass reads / writes x, y and W once'}

    def medformer_report():
        # the R-Super use proper: MedFormer with report supervision (one mask + one report sample); eager, then with the network's forward
        # and backward replayed from two hipGraphs around the eager loss (losses identical: tests/test_gpu_edge.py)
        nm = min(n2, 10)
        lr_ = leg_of(args.dtype, True, medformer=True)
        sec['medformer_report_ms_per_step'] = lr_.timed(nm, 3) / nm * 1e3
        lr_.close()
        del lr_
        torch.cuda.empty_cache()
        lg = leg_of(args.dtype, True, medformer=True)
        lg.use_net_graphs()
        sec['medformer_report_netgraph_ms_per_step'] = lg.timed(nm, 14) / nm * 1e3      # the self-verification replays (1, 12) fall into the warm-up
        lg.close()

    def f32():
        ref_logits = bf16_last_loss = None
        if not args.report:
            # the bf16 run the f32 leg is compared with: the same number of optimiser steps as the headline run, from the same initial weights
            lb = leg_of('bf16', False)
            lb.run(headline_steps)
            lb.sync()
            ref_logits, bf16_last_loss = lb.logits(), lb.loss()
            lb.close()
            del lb
            torch.cuda.empty_cache()
        lf32 = leg_of('f32', args.report)
        n3 = min(n2, 10)
        sec['f32_ms_per_step'] = lf32.timed(n3, 2) / n3 * 1e3
        if ref_logits is not None:
            lf32.run(headline_steps - lf32.step)
            lf32.sync()
            f32_logits = lf32.logits()
            sec['bf16_vs_f32'] = {
                'steps': headline_steps,
                'abs_delta_overall_loss': abs(lf32.loss() - bf16_last_loss),
                'bf16_overall_loss': bf16_last_loss, 'f32_overall_loss': lf32.loss(),
                'logits_rel_l2': float(((ref_logits - f32_logits).double().norm() / f32_logits.double().norm()).item()),
                'note': 'identical init and batch, same number of optimiser steps in both arithmetic modes (full size); loss of the last step, '
                        'logits of the trained weights on the training batch',
            }
        lf32.close()
        del lf32
        torch.cuda.empty_cache()
        if ref_logits is not None:
            # The gap of ONE trajectory is a chaotic quantity: a 1e-6 relative perturbation of the initial weights moves the f32 curve itself by 0.004 .. 0.028 at
            # step 35 and pure summation-order commits moved the seed-0 gap by +-0.03 (profiles/r06_drift_bisect.txt, r06_drift_ensemble.txt).
            # What the kernels are held to is the distribution over (initial weights, batch) seeds: signed gaps after `headline_steps` steps, their mean and spread.
            gaps = [sec['bf16_vs_f32']['bf16_overall_loss'] - sec['bf16_vs_f32']['f32_overall_loss']]
            for sd in (1, 2, 3, 4, 5):
                v = {}
                for dt in ('bf16', 'f32'):
                    le = leg_of(dt, False, seed=sd)
                    le.run(headline_steps)
                    le.sync()
                    v[dt] = le.loss()
                    le.close()
                    del le
                    torch.cuda.empty_cache()
                gaps.append(v['bf16'] - v['f32'])
            m = sum(gaps) / len(gaps)
            sec['bf16_vs_f32']['ensemble'] = {
                'seeds': [0, 1, 2, 3, 4, 5], 'signed_gap_bf16_minus_f32': gaps, 'mean': m,
                'sd': (sum((g - m) ** 2 for g in gaps) / len(gaps)) ** 0.5,
                'note': 'same comparison for six (initial weights, batch) seeds; seed 0 is the run above.  The sign of a seed\'s gap is a property of that (weights, batch) pair '
                        '(seeds 0-3 positive, 4-5 negative in the round-4 tree and in this one alike); reference measurement of rounds 4 / 6 at 35 steps: mean -0.006 / +0.0002, '
                        'sd 0.033 / 0.030, at 70 steps +0.013 / +0.017, sd 0.062 / 0.064 (profiles/r06_drift_ensemble.txt, DESIGN.md section 4)'}

    if not args.report:
        guarded('sanity_on', sanity_on)
        guarded('config3', config3)
        guarded('nopool', nopool)
        guarded('graph', graph)
        if args.base == 32:
            guarded('medformer_graph', medformer_graph)
            guarded('medformer', medformer)
            guarded('medformer_roofline', medformer_roofline)
            guarded('medformer_report', medformer_report)
    if args.dtype == 'bf16':
        guarded('f32', f32)
    return sec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--gpus', type=int, default=1)
    ap.add_argument('--steps', type=int, default=50)       # >= 50 timed steps after >= 10 warm-up
    ap.add_argument('--warmup', type=int, default=10)
    ap.add_argument('--size', type=int, default=96)
    ap.add_argument('--batch', type=int, default=2, help='per-GPU batch (bs=2/GPU in BASELINE.json)')
    ap.add_argument('--base', type=int, default=32)
    ap.add_argument('--dtype', default='bf16', choices=['bf16', 'f32'])
    ap.add_argument('--cpu-baseline-steps', type=int, default=3, help='timed CPU steps of the baseline leg (>= 3, BASELINE.md section 3)')
    ap.add_argument('--report', action='store_true', help='config 3: report supervision on (ball_dice_both, 50/50 mask/report batch)')
    ap.add_argument('--no-pool', action='store_true', help="variant (not the headline): down_block(pool=False) -- the strided BasicBlock members (SURVEY 8 row g)")
    ap.add_argument('--no-cpu-baseline', action='store_true')
    ap.add_argument('--guards', type=int, default=1, help="1: the reference's per-step guards run inside the timed region as device-side flags (default); 0: off")
    ap.add_argument('--no-secondary', action='store_true', help='skip the config-3 / f32 / bf16-vs-f32 legs')
    ap.add_argument('--unpacked-labels', action='store_true', help='A/B: label / unknown / segment volumes as uint8 planes instead of the bit-packed storage form')
    ap.add_argument('--roofline-steps', type=int, default=10, help='(--full) steps of the separate HIP-event pass after the timed region')
    ap.add_argument('--full', action='store_true', help='after the headline: roofline pass, secondary legs (N = 1) and CPU baseline (N = 1)')
    ap.add_argument('--dump-outputs', metavar='DIR', help="write the last timed step's losses and a seeded sample of parameters / EMA / gradients as DIR/<name>.npy")
    ap.add_argument('--secondary-only', action='store_true', help='(internal) run only the secondary legs and print their JSON')
    ap.add_argument('--force-ddp', action='store_true', help='wrap in the data-parallel reducer even with one rank (exercises the RCCL path)')
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error('--steps must be >= 1 and --warmup >= 0')

    if args.gpus > 1 and 'WORLD_SIZE' not in os.environ:
        sys.exit(respawn_under_torchrun(args))

    import synth
    from rsuper_amd.hip import lib, ops
    from rsuper_amd.train_ddp import init_distributed
    from rsuper_amd.training import losses_foundation as lf

    if args.force_ddp and int(os.environ.get('WORLD_SIZE', '1')) == 1:
        os.environ.setdefault('MASTER_ADDR', '127.0.0.1'); os.environ.setdefault('MASTER_PORT', '29511')
        dist.init_process_group(backend='nccl', rank=0, world_size=1)
    rank, local, world = init_distributed()
    assert world == args.gpus, f'--gpus {args.gpus} but WORLD_SIZE={world}'
    local = local % torch.cuda.device_count()          # one rank per GPU; ranks only share a device in the gloo debugging mode
    torch.cuda.set_device(local)
    lib.require_device()
    dev = f'cuda:{local}'
    # The reference's per-step guards (input isnan / range asserts train_ddp.py:311-313, mask / unknown / volume consistency losses_foundation.py:864-869,
    # NaN loss :1070-1071) run INSIDE the timed region as device-side flags (train_ddp.StepGuard: raised one step late, the update of a NaN step is
    # skipped on the device).  --sync-guards 0 turns them off; secondary.sanity_on_ms_per_step is the same step with the reference's synchronous form.
    lf.SANITY_CHECKS = bool(args.guards)
    classes = synth.PANTS_CLASSES
    B, S = args.batch, args.size

    if args.secondary_only:
        print(json.dumps(secondary_legs(args, rank, world, local, classes, B, S)))
        return
    leg = Leg(args, args.dtype, args.report, rank, world, local, args.force_ddp, classes, B, S)
    if args.guards:
        from rsuper_amd.train_ddp import StepGuard
        leg.guard = lf.GUARD = StepGuard(dev)
    dt = leg.timed(args.steps, args.warmup)
    if leg.guard is not None:
        leg.guard.poll(final=True)
        leg.guard = lf.GUARD = None
    lf.SANITY_CHECKS = False             # the legs below (roofline pass, secondary workloads) run without them, as before
    tmax = torch.tensor([dt], device=dev, dtype=torch.float64)
    if world > 1:
        dist.all_reduce(tmax, op=dist.ReduceOp.MAX)
    dt = float(tmax.item())
    loss_val = leg.loss()
    if args.dump_outputs and rank == 0:
        dump_outputs(leg, args.dump_outputs)

    out = None
    if rank == 0:
        out = {
            'metric': 'CT voxels/sec/node (96³ patch, bs=2/GPU)', 'value': world * B * S ** 3 * args.steps / dt, 'unit': 'voxels/s',
            'n_gpus': world, 'steps': args.steps, 'warmup': args.warmup, 'ms_per_step': dt / args.steps * 1e3,
            'higher_is_better': True, 'scaling': 'weak', 'vs_baseline': None, 'dtype': args.dtype, 'data': 'synthetic',
            'config': {'workload': f'R-Super 3D UNet(base {args.base}, {len(classes)} classes, BasicBlock/IN) full training step '
                                   f'(fwd + {"seg+Volume+Ball" if args.report else "masked BCE + Dice"} loss + bwd + clip + AdamW + EMA), '
                                   f'{S}^3 patches, batch {B}/GPU (BASELINE.json configs[{2 if args.report else 1}])' + (' -- VARIANT pool=False (strided down blocks)' if args.no_pool else ''),
                       'global_batch': world * B, 'patch': S, 'parallelism': f'dp{world}', 'final_loss': loss_val,
                       'label_volumes': 'uint8 planes' if args.unpacked_labels else 'bit-packed (np.packbits over classes, the dataset storage form), read packed by the loss kernels',
                       'sanity_checks_in_timed_region': bool(args.guards),
                       'sanity_checks_form': 'device-side flags read one step late (train_ddp.StepGuard)' if args.guards else 'off'},
        }

    # ---- --full only, below: nothing of it feeds the headline fields above
    if args.full and rank == 0:
        # ---- roofline pass (outside the timed region): HIP events around every conv MFMA launch, on the launch stream
        timer = ops.KernelTimer()
        ops.TIMER = timer
    if args.full and args.roofline_steps > 0:
        import gc
        gc.collect()
        gc.disable()                      # a collection between recording a start event and launching its kernel would be charged to the bracket
        for _ in range(args.roofline_steps):      # every rank runs the same steps (the reducer's collectives need all ranks)
            if rank == 0:
                timer.next_step()
            leg.run(1)
        leg.sync()
        gc.enable()
    ops.TIMER = None
    if args.full and rank == 0:
        ksum = timer.summary()
        conv_ms_sum = sum(d['ms'] for d in ksum.values())
        # union of the launch intervals (weight gradients may overlap the data-gradient chain) over the steps within 5 % of the median step (ops.KernelTimer.summary:
        # a bracket whose kernel launch the host delivered late measures the host; every step's figure is reported in conv_ms_each_step)
        rs = max(timer.steps_used, 1)
        conv_ms = timer.busy_ms
        conv_ms_mean = timer.busy_ms_all / max(len(timer.step_busy_ms), 1)
        conv_fl = sum(d['flops'] for d in ksum.values())
        fwd_fl = conv_stack_flops(args.base, S, B)
        peak = MFMA_PEAK_TFLOPS[args.dtype]
        achieved = conv_fl / (conv_ms * 1e-3) / 1e12 if conv_ms > 0 else 0.0
        traffic, traffic_src = None, None
        default_wl = args.dtype == 'bf16' and args.base == 32 and B == 2 and S == 96 and not args.report and not args.no_pool
        if default_wl and os.path.exists(TRAFFIC_PROFILE):
            tp = json.load(open(TRAFFIC_PROFILE))
            traffic, traffic_src = tp.get('conv_bytes_per_step'), tp.get('source')
        out.update({
            'roofline': {'bound': 'mfma', 'achieved': achieved, 'peak': peak, 'unit': 'TFLOP/s', 'frac': achieved / peak,
                         'traffic': traffic, 'traffic_unit': 'bytes per step over all conv MFMA launches (FETCH_SIZE x2 + WRITE_SIZE)',
                         'traffic_source': traffic_src,
                         'kernel': 'conv3d MFMA kernels (igemm fwd + dgrad, wgrad): 3x the 43 3x3x3 convs',
                         'algorithmic_gflop_per_step': conv_fl / rs / 1e9, 'expected_gflop_per_step': 3 * fwd_fl / 1e9,
                         'conv_ms_per_step': conv_ms / rs, 'conv_ms_per_step_sum_of_launches': conv_ms_sum / rs,
                         'conv_ms_per_step_all_steps': conv_ms_mean, 'steps_used': timer.steps_used, 'conv_ms_each_step': [round(v, 4) for v in timer.step_busy_ms],
                         'timing_events': 'torch.cuda.Event (default flags: system-scope release per record)' if timer.fenced else
                                          'hipEventDisableSystemFence events on the launch stream (rsuper_timer_event_*; include/rsuper_hip.h)',
                         'measured_in': f'separate pass of {args.roofline_steps} steps after the timed region (HIP events on the launch stream); steps within 5 % of the median step count',
                         'note': 'achieved = algorithmic FLOPs of all conv MFMA launches of the counted steps / union of their launch intervals; '
                                 'per_kernel.avg_us are raw per-launch durations',
                         'step_level_frac': (3 * fwd_fl / (dt / args.steps)) / 1e12 / peak,
                         'per_kernel': {k: {'launches_per_step': d['launches'] / rs, 'avg_us': d['ms'] * 1e3 / d['launches'], 'max_us': d['max_ms'] * 1e3,
                                            'tflops': d['flops'] / (d['ms'] * 1e-3) / 1e12} for k, d in ksum.items()}},
        })
    if args.full and world == 1 and not args.no_secondary and not args.force_ddp:
        # ---- secondary legs in a child process: whatever happens there (exception, hard crash), the headline line is still printed
        leg.close()
        del leg
        torch.cuda.empty_cache()
        cmd = [sys.executable, os.path.abspath(__file__), '--secondary-only'] + [a for a in sys.argv[1:] if a != '--secondary-only']
        try:
            r = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=1500)
            lines = [ln for ln in r.stdout.strip().splitlines() if ln.startswith('{')]
            out['secondary'] = json.loads(lines[-1]) if (r.returncode == 0 and lines) else {'error': f'rc {r.returncode}: ' + r.stderr.strip()[-300:]}
        except Exception as e:                           # noqa: BLE001 -- includes the timeout
            out['secondary'] = {'error': repr(e)[:300]}
    if args.full and rank == 0 and not args.no_cpu_baseline and world == 1:
        try:
            out['cpu_baseline'] = cpu_baseline(args, classes)
        except Exception as e:                           # noqa: BLE001 -- a reported baseline must not cost the headline line
            out['cpu_baseline'] = {'error': repr(e)[:300]}
    if world > 1 or args.force_ddp:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        # the ONE JSON line goes out last: RCCL printf()s a version banner into the C stdio buffer, which would
        # otherwise be flushed at process exit, after this line
        import ctypes
        sys.stdout.flush()
        ctypes.CDLL(None).fflush(None)
        print(json.dumps(out), flush=True)


if __name__ == '__main__':
    main()
