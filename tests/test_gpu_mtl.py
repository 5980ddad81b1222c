"""Multi-task and CLIP baselines on the device: the fused tail of ClassificationBranch (csrc/cls_branch.hip) and the unfused chain against float64 of the
same operands, the two losses, the whole model against the fixture of the unmodified reference (tests/golden/mtl.npz), one training step."""
import argparse
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import mtl_ref as mr
import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = torch.from_numpy
DEV = 'cuda'


def _shapes(g, key):
    return {str(n): tuple(int(d) for d in str(s).split(',')) if str(s) else () for n, s in zip(g[key + '_names'], g[key + '_shapes'])}


def _ulp(a):
    return float(np.spacing(np.float32(np.abs(np.asarray(a, np.float64)).max())))


def _bound(fixture, f64):
    """4 x the distance of the reference's own CPU float32 result from float64, plus 2 float32 ulp of the tensor's largest magnitude."""
    fixture, f64 = np.asarray(fixture, np.float64), np.asarray(f64, np.float64)
    return 4 * float(np.abs(fixture - f64).max()) + 2 * _ulp(f64)


def _dist(a, f64):
    return float(np.abs(np.asarray(a, np.float64) - np.asarray(f64, np.float64)).max())


def _branch(nc, params):
    from rsuper_amd.model.dim3.medformer import ClassificationBranch
    br = ClassificationBranch(num_classes=nc)
    br.load_state_dict({k: T(params[k]) for k in br.state_dict()})
    return br.to(DEV)


def _run_tail(br, x, go, fused):
    """(out, dx, grads by TAIL_KEYS) of the branch's tail on tokens x (B, L, 160), through autograd.grad (no gradient accumulation kernels)."""
    from rsuper_amd.model.dim3 import medformer as M
    old = M.CLS_FUSED
    M.CLS_FUSED = fused
    try:
        xt = T(np.ascontiguousarray(x)).to(DEV).requires_grad_(True)
        B, L, _ = xt.shape
        ps = dict(br.named_parameters())
        out = br.tail(xt.reshape(B, L, 1, 1, 160))
        gs = torch.autograd.grad(out, [xt] + [ps[k] for k in mr.TAIL_KEYS], T(go).to(DEV))
    finally:
        M.CLS_FUSED = old
    torch.cuda.synchronize()
    return out.detach().cpu().numpy(), gs[0].cpu().numpy(), {k: g.cpu().numpy() for k, g in zip(mr.TAIL_KEYS, gs[1:])}


@pytest.fixture(scope='module')
def tail_refs(golden):
    """float64 restatement of every branch-alone case, computed once."""
    g = golden['mtl']
    refs = {}
    for tag in mr.BRANCH_SHAPES:
        for nc in mr.BRANCH_NC:
            params = mr.fill(_shapes(g, f'branch_{"L1" if tag == "L1" else "L8"}_{nc}'), mr.BRANCH_SEED)
            refs[tag, nc] = (params,) + mr.tail_with_grads(g[f'branch_{tag}_xtail'], params, mr.out_grad(tag, nc), torch.float64)
    return refs


def _sub(a, ref_len, numel):
    return synth.subsample(np.asarray(a), ref_len if ref_len < numel else numel)[0]


@pytest.mark.parametrize('tag', list(mr.BRANCH_SHAPES))
@pytest.mark.parametrize('nc', mr.BRANCH_NC)
def test_tail_forward_and_backward_against_float64(golden, tail_refs, tag, nc):
    """Fused kernel, unfused chain and the fixture, each within 4 x (fixture - float64) + 2 ulp per tensor; L1 is the one-token soft-max."""
    g = golden['mtl']
    key = f'branch_{tag}_{nc}'
    params, out64, dx64, g64 = tail_refs[tag, nc]
    x = g[f'branch_{tag}_xtail']
    br = _branch(nc, params)
    assert br.fused(T(x).to(DEV))
    runs = {'fused': _run_tail(br, x, mr.out_grad(tag, nc), True), 'unfused': _run_tail(br, x, mr.out_grad(tag, nc), False)}
    worst = {}
    tensors = [('out', g[key + '_out'], out64.numpy(), lambda r: r[0])]
    n = len(g[key + '_dxtail_sub'])
    tensors.append(('dx', g[key + '_dxtail_sub'], _sub(dx64.numpy(), n, dx64.numel()), lambda r: _sub(r[1], n, dx64.numel())))
    for k in mr.TAIL_KEYS:
        ref = g[f'{key}_g_{k}_sub']
        tensors.append((k, ref, _sub(g64[k].numpy(), len(ref), g64[k].numel()), lambda r, k=k, m=len(ref): _sub(r[2][k], m, g64[k].numel())))
    fails = []
    for name, fix, f64, pick in tensors:
        bound = _bound(fix, f64)
        d = {'fixture': _dist(fix, f64), **{which: _dist(pick(r), f64) for which, r in runs.items()}}
        assert all(np.isfinite(pick(r)).all() for r in runs.values()), name
        print(f'{key} {name}: bound {bound:.3e} ' + ' '.join(f'{w} {v:.3e}' for w, v in d.items()))
        for w, v in d.items():
            worst[w] = max(worst.get(w, 0.0), v / bound)
            if v > bound:
                fails.append((name, w, v, bound))
    print(f'{key} worst distance / bound: ' + ' '.join(f'{w} {v:.3f}' for w, v in worst.items()))
    assert not fails, fails


def test_two_fused_runs_give_identical_bits(golden, tail_refs):
    g = golden['mtl']
    for tag, nc in (('L27', 3), ('L64', 768)):
        params = tail_refs[tag, nc][0]
        br = _branch(nc, params)
        a = _run_tail(br, g[f'branch_{tag}_xtail'], mr.out_grad(tag, nc), True)
        b = _run_tail(br, g[f'branch_{tag}_xtail'], mr.out_grad(tag, nc), True)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
        assert all(np.array_equal(a[2][k], b[2][k]) for k in mr.TAIL_KEYS)


def _kernel_names(fn):
    from torch.profiler import profile, ProfilerActivity
    fn()
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        res = fn()
        torch.cuda.synchronize()
    return res, [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]


def test_fused_tail_launch_counts(golden, tail_refs):
    """Forward 1 kernel, backward at most 3, neither with a memset or a memcpy."""
    g = golden['mtl']
    params = tail_refs['L27', 3][0]
    br = _branch(3, params)
    ps = dict(br.named_parameters())
    xt = T(g['branch_L27_xtail']).to(DEV).requires_grad_(True)
    go = T(mr.out_grad('L27', 3)).to(DEV)
    inputs = [xt] + [ps[k] for k in mr.TAIL_KEYS]
    tokens = xt.reshape(2, 27, 1, 1, 160)
    out, fwd = _kernel_names(lambda: br.tail(tokens))
    _, bwd = _kernel_names(lambda: torch.autograd.grad(out, inputs, go, retain_graph=True))
    print('forward', fwd, 'backward', bwd)
    assert len(fwd) == 1 and 'cls_tail_fwd' in fwd[0], fwd
    assert 1 <= len(bwd) <= 3 and any('cls_tail_bwd' in n for n in bwd), bwd
    assert not any('memset' in n.lower() or 'memcpy' in n.lower() for n in fwd + bwd), (fwd, bwd)


def test_unfused_switch_and_long_sequences():
    """RSUPER_MF_CLS_FUSED=0 in a fresh process selects the chain of existing operators; above 64 tokens the module takes it without being asked."""
    code = ('import os, sys, torch; sys.path.insert(0, %r); import rsuper_amd\n'
            'from rsuper_amd.model.dim3 import medformer as M\n'
            'br = M.ClassificationBranch().cuda(); x = torch.randn(1, 8, 160, device="cuda")\n'
            'from torch.profiler import profile, ProfilerActivity\n'
            'with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:\n'
            '    y = br.tail(x.reshape(1, 8, 1, 1, 160)); torch.cuda.synchronize()\n'
            'names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]\n'
            'print("FUSED", M.CLS_FUSED, br.fused(x), any("cls_tail" in n for n in names), tuple(y.shape))\n') % ROOT
    r = subprocess.run([sys.executable, '-c', code], env=dict(os.environ, RSUPER_MF_CLS_FUSED='0'), capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert 'FUSED False False False (1, 3)' in r.stdout, r.stdout
    from rsuper_amd.model.dim3.medformer import MedFormer, ClassificationBranch
    from rsuper_amd.model.dim3.medformer_utils import Feat, down_block
    torch.manual_seed(0)
    br = ClassificationBranch(extra_layer=down_block(320, 160, 0, 1, 4, 20, 4, [2, 2, 2], True)).to(DEV)
    x4 = torch.randn(1, 10, 10, 10, 320, device=DEV)                       # (1, 320, 10, 10, 10) channels-last -> 125 tokens
    assert not br.fused(torch.empty(1, 125, 160, device=DEV)) and br.fused(torch.empty(1, 64, 160, device=DEV))
    _, names = _kernel_names(lambda: br(Feat(g=x4), torch.float32))
    y = br(Feat(g=x4), torch.float32)
    assert y.shape == (1, 3) and bool(torch.isfinite(y).all()) and not any('cls_tail' in n for n in names)
    with pytest.raises(ValueError):                                         # an odd side is refused by PatchMerging, as before
        br(Feat(g=torch.randn(1, 3, 4, 4, 320, device=DEV)), torch.float32)


def _no_d2h(names):
    return not any('dtoh' in n.lower().replace(' ', '') or 'devicetohost' in n.lower().replace(' ', '') for n in names)


@pytest.mark.parametrize('form', ['packed', 'uint8'])
def test_classification_loss_against_float64(golden, form):
    """Every fixture case: value and d cls_out within 2 float32 ulp of the float64 evaluation, no device-to-host copy."""
    from rsuper_amd.training import losses_foundation as lf
    from rsuper_amd.training.dataset.packed import PackedBits, pack_bits
    g = golden['mtl']

    def dev(v):
        if v is None:
            return None
        return PackedBits(T(pack_bits(v)).to(DEV), v.shape[1]) if form == 'packed' else T(v).to(DEV)
    for name, (lab, unk, msk, cw) in mr.loss_cases().items():
        x64 = T(mr.loss_logits()).double().requires_grad_(True)
        l64 = mr.classification_loss(x64, T(lab), None if unk is None else T(unk), T(msk), mr.LOSS_CLASSES, None if cw is None else T(cw).double())
        l64.backward()
        vols = (dev(lab), dev(unk), dev(msk))
        w = None if cw is None else T(cw).to(DEV)

        def run():
            for v in vols:
                if form == 'packed' and v is not None:
                    v.reset()
            x = T(mr.loss_logits()).to(DEV).requires_grad_(True)
            l = lf.classification_loss(x, vols[0], vols[1], argparse.Namespace(), vols[2], mr.LOSS_CLASSES, w)
            l.backward()
            return l.detach(), x.grad
        (l, gx), names = _kernel_names(run)
        dv, dg = abs(float(l) - float(l64)), np.abs(gx.cpu().numpy().astype(np.float64) - x64.grad.numpy())
        print(f'cls {form} {name}: value {float(l):.8f} |d| {dv:.2e} (2 ulp {2 * _ulp(float(l64)):.2e}); grad max |d| {dg.max():.2e}; fixture |d| '
              f'{abs(float(g[f"cls_{name}_value"]) - float(l64)):.2e}')
        assert dv <= 2 * _ulp(float(l64)), name
        assert (dg <= 2 * np.spacing(np.abs(x64.grad.numpy()).astype(np.float32)).astype(np.float64)).all(), name
        assert _no_d2h(names), names
    with pytest.raises(ValueError):
        lf.classification_loss(torch.zeros(2, 3, device=DEV), dev(lab), None, argparse.Namespace(), None, mr.LOSS_CLASSES)
    with pytest.raises(RuntimeError):                                       # weights that do not broadcast against (B, Nc)
        lf.classification_loss(torch.zeros(2, 2, device=DEV), dev(lab), None, argparse.Namespace(), None, mr.LOSS_CLASSES, torch.ones(2, 5, device=DEV))


def test_info_nce_and_clip_only_against_float64(golden):
    from rsuper_amd.training import losses_foundation as lf
    from rsuper_amd.training.info_nce import info_nce
    g = golden['mtl']
    for n, d in mr.NCE_SHAPES:
        qn, kn = mr.nce_inputs(n, d)
        q64, k64 = T(qn).double().requires_grad_(True), T(kn).double().requires_grad_(True)
        l64 = mr.info_nce(q64, k64)
        l64.backward()
        q, k = T(qn).to(DEV).requires_grad_(True), T(kn).to(DEV).requires_grad_(True)
        (l, names) = _kernel_names(lambda: info_nce(q, k))
        assert sum('info_nce' in nm for nm in names) == 1, names                 # value and both gradients from one launch
        l.backward()
        for name, got, fix, ref in (('value', l.detach().cpu().numpy(), g[f'nce_{n}_{d}_value'], l64.detach().numpy()),
                                    ('dq', q.grad.cpu().numpy(), g[f'nce_{n}_{d}_dq'], q64.grad.numpy()),
                                    ('dk', k.grad.cpu().numpy(), g[f'nce_{n}_{d}_dk'], k64.grad.numpy())):
            print(f'nce {n}x{d} {name}: bound {_bound(fix, ref):.3e} fixture {_dist(fix, ref):.3e} device {_dist(got, ref):.3e}')
            assert _dist(got, ref) <= _bound(fix, ref), (n, d, name)
        if n == 1:
            assert float(l.detach()) == 0.0 and not q.grad.any() and not k.grad.any()

    class Dist:
        @staticmethod
        def get_world_size():
            return 2
    qn, kn = mr.nce_inputs(2, 768)
    q64 = T(qn).double().requires_grad_(True)
    l64 = 0.5 * (mr.info_nce(q64, T(kn).double()) + mr.info_nce(T(kn).double(), q64)) * 2
    l64.backward()
    q = T(qn).to(DEV).requires_grad_(True)
    seg = [torch.zeros(2, 5, 4, 4, 4, device=DEV, requires_grad=True) for _ in range(2)]
    loss = lf.calculate_loss({'segmentation': seg, 'clip': q}, None, None, argparse.Namespace(), None, None, None, None, mr.LOSS_CLASSES, clip_only=True,
                             report_embeddings=T(kn).to(DEV), dist=Dist)
    assert sorted(loss) == ['contrastive_loss', 'overall']
    loss['overall'].backward()
    assert _dist(loss['overall'].detach().cpu().numpy(), l64.detach().numpy()) <= _bound(g['clip_only_value'], l64.detach().numpy())
    assert _dist(q.grad.cpu().numpy(), q64.grad.numpy()) <= _bound(g['clip_only_dq'], q64.grad.numpy())
    assert all(s.grad is not None and not s.grad.any() for s in seg)
    one = lf.calculate_loss({'segmentation': seg, 'clip': q}, None, None, argparse.Namespace(), None, None, None, None, mr.LOSS_CLASSES, clip_only=True,
                            report_embeddings=T(kn).to(DEV), dist=None)            # no process group: one rank
    assert abs(float(one['overall']) * 2 - float(loss['overall'])) <= 4 * _ulp(float(loss['overall']))
    with pytest.raises(AssertionError):
        lf.calculate_loss({'segmentation': seg, 'clip': q}, None, None, argparse.Namespace(), None, None, None, None, mr.LOSS_CLASSES, clip_only=True,
                          report_embeddings=T(kn[:, :7]).to(DEV))


def test_whole_model_against_the_reference_fixture(golden):
    """64^3, both branches, f32: branch outputs against the reference in float64 (the tail's bound), both segmentation heads against the fixture, every parameter with a gradient, the ones that feed
    only the branches' semantic maps exactly zero, every gradient against the fixture's samples (the encoder's now carry the branches' share)."""
    from rsuper_amd.model.dim3.medformer import MedFormer
    g = golden['mtl']
    net = MedFormer(1, len(synth.TINY_CLASSES), compute_dtype='f32', classification_branch=True, class_list_cls=mr.MODEL_CLS, clip_branch=True,
                    clip_feats=mr.MODEL_CLIP, **mr.MODEL_CFG)
    shapes = {k: tuple(v.shape) for k, v in net.state_dict().items()}
    assert shapes == _shapes(g, 'model')
    net.load_state_dict({k: T(v) for k, v in mr.fill(shapes, mr.MODEL_SEED).items()})
    net = net.to(DEV)
    res = net(T(synth.image(1, mr.MODEL_SIZE, seed=1234)).to(DEV))
    y, aux = res['segmentation']
    assert res['classification'].shape == (1, 3) and res['clip'].shape == (1, mr.MODEL_CLIP)
    assert res['classification'].dtype == torch.float32 and res['clip'].dtype == torch.float32
    go = synth.rng(77).standard_normal(tuple(y.shape)).astype(np.float32) / y.numel()
    ga = synth.rng(78).standard_normal(tuple(aux.shape)).astype(np.float32) / aux.numel()
    gc = synth.rng(79).standard_normal((1, 3)).astype(np.float32)
    ge = synth.rng(80).standard_normal((1, mr.MODEL_CLIP)).astype(np.float32)
    ((y * T(go).to(DEV)).sum() + (aux * T(ga).to(DEV)).sum() + (res['classification'] * T(gc).to(DEV)).sum() + (res['clip'] * T(ge).to(DEV)).sum()).backward()
    torch.cuda.synchronize()
    rel = lambda a, b: float(np.abs(np.asarray(a, np.float64) - b).max() / np.abs(b).max())
    # the branch outputs: the tail's rule, 4 x (the reference's CPU float32 run - the reference in float64) + 2 ulp, against the float64 values
    misses = []
    for name in ('classification', 'clip'):
        got, fix, f64 = res[name].detach().cpu().numpy(), g['model_' + name], g['model_' + name + '_f64']
        print(f'whole model {name}: bound {_bound(fix, f64):.3e} fixture {_dist(fix, f64):.3e} device {_dist(got, f64):.3e} (largest magnitude '
              f'{np.abs(f64).max():.3f})')
        if _dist(got, f64) > _bound(fix, f64):
            misses.append(name)
    e = dict(logits=rel(synth.subsample(y.detach().cpu().numpy(), 4096)[0], g['model_logits_sub']),
             aux=rel(synth.subsample(aux.detach().cpu().numpy(), 4096)[0], g['model_aux_sub']))
    print('whole model, segmentation heads relative to the largest magnitude:', e)
    assert not misses, misses
    assert max(e.values()) <= 1e-4, e                                        # the f32 parity bound of the MedFormer fixture's heads
    gmax = max(float(g[f'model_g_{k}_summary'][2]) for k, _ in net.named_parameters())
    worst, wk, zeros = 0.0, '', 0
    for k, p in net.named_parameters():
        assert p.grad is not None, k
        ref = g[f'model_g_{k}_sub']
        if float(g[f'model_g_{k}_summary'][2]) == 0.0 and '_branch.extra_layer.' in k:      # feeds only the branch's semantic map: `+ 0 * tmp_map.sum()`
            assert not bool(p.grad.any()), k
            zeros += 1
            continue
        err = float(np.abs(synth.subsample(p.grad.cpu().numpy(), 256)[0] - ref).max() / max(float(g[f'model_g_{k}_summary'][2]), 1e-3 * gmax))
        if err > worst:
            worst, wk = err, k
    print(f'whole model: worst gradient {worst:.2e} of its largest entry @ {wk}; {zeros} parameters with an exactly zero gradient')
    assert zeros > 0 and worst <= 6e-2, (worst, wk)                           # the gradient bound of the MedFormer fixture (tests/gpu_checks.py)


def test_train_step_with_the_classification_branch():
    from rsuper_amd.model.dim3.medformer import MedFormer
    from rsuper_amd.train_ddp import train_step, make_ema
    from rsuper_amd.training.dataset.packed import PackedBits, pack_bits
    from rsuper_amd.training.utils import FusedAdamWEMA
    classes = synth.TINY_CLASSES
    largs = argparse.Namespace(loss='ball_dice_last', aux_weight=[0.5, 0.5], seg_loss=1.0, report_volume_loss_basic=0.0, volume_loss_tolerance=0.2,
                               ball_bce_weight=1.0, ball_dice_weight=1.0, ball_volume_margin=0.2, multi_ch_tumor=False, stardard_ce_ball=False,
                               classification_branch=True, ema=True, ema_alpha=0.99)
    bt = synth.batch(2, 64, classes, ['mask', 'mask'], seed=11, diam_range=(4.0, 8.0), max_tumors=2)
    pk = lambda a: PackedBits(T(pack_bits(a)).to(DEV), len(classes))
    batch = dict(image=T(synth.image(2, 64, seed=5)).to(DEV), label=pk(bt['label']), unk_channels=pk(bt['unk_channels']), mask=pk(bt['mask']),
                 volumes=T(bt['volumes']).to(DEV), diameters=T(bt['diameters']).to(DEV))
    torch.manual_seed(0)
    net = MedFormer(1, len(classes), compute_dtype='bf16', classification_branch=True, class_list_cls=['kidney_lesion', 'pancreatic_lesion'],
                    **mr.MODEL_CFG).to(DEV)
    ema = make_ema(net)
    opt = FusedAdamWEMA(net.parameters(), lr=6e-4, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.05)
    before = net.classification_branch.head.weight.detach().clone()
    from rsuper_amd.model.dim3 import medformer_utils as mu
    gemm_compute = mu.GEMM_COMPUTE                               # MedFormer.forward sets it per call, process-wide: leave it as it was
    try:
        loss, gnorm = train_step(net, ema, opt, batch, largs, classes, 0)
    finally:
        mu.GEMM_COMPUTE = gemm_compute
    assert 'classification' in loss and all(bool(torch.isfinite(v)) for v in loss.values())
    total = sum(float(v) for k, v in loss.items() if k != 'overall')
    assert abs(float(loss['overall']) - total) <= 4 * _ulp(total)
    assert all(p.grad is not None for p in net.parameters())
    assert bool((net.classification_branch.head.weight.detach() != before).any())


def test_branch_on_a_two_voxel_bottleneck():
    """x4 of (B, 320, 2, 2, 2): this project's branch, extra layer included, down to ONE token (the reference's InstanceNorm3d refuses a single
    spatial element, so no fixture exists): finite outputs and gradients for every parameter and the input, fused and unfused."""
    from rsuper_amd.model.dim3 import medformer as M
    from rsuper_amd.model.dim3.medformer_utils import Feat, down_block
    torch.manual_seed(0)
    br = M.ClassificationBranch(num_classes=3, extra_layer=down_block(320, 160, 0, 1, 4, 20, 4, [2, 2, 2], True)).to(DEV)
    for fused in (True, False):
        old, M.CLS_FUSED = M.CLS_FUSED, fused
        try:
            x4 = T(mr.x4('L1')).permute(0, 2, 3, 4, 1).contiguous().to(DEV).requires_grad_(True)          # channels-last (1, 2, 2, 2, 320)
            y = br(Feat(g=x4), torch.float32)
            gs = torch.autograd.grad(y, [x4] + list(br.parameters()), T(mr.out_grad('L1', 3)).to(DEV))
        finally:
            M.CLS_FUSED = old
        assert y.shape == (1, 3) and bool(torch.isfinite(y).all())
        assert all(bool(torch.isfinite(t).all()) for t in gs)


def test_update_output_layer_on_a_branched_model():
    """update_output_layer_onk on a MedFormer with the branch, on the device: the new head lives where the old one did, the fused tail picks up its
    class count, and the copied rows are the old head's."""
    from rsuper_amd.model.dim3.medformer import MedFormer, update_output_layer_onk
    old_cls = [c for c in mr.ONK_OLD if 'lesion' in c]
    net = MedFormer(1, len(mr.ONK_OLD), compute_dtype='f32', classification_branch=True, class_list_cls=old_cls, **mr.MODEL_CFG).to(DEV)
    old_head = net.classification_branch.head
    old_w = old_head.weight.detach().clone()
    update_output_layer_onk(net, original_classes=mr.ONK_OLD, new_classes=mr.ONK_NEW, copy_pancreas=False)
    head = net.classification_branch.head
    new_cls = [c for c in mr.ONK_NEW if any(p in c for p in ('background', 'lesion', 'pdac', 'pnet', 'cyst'))]
    assert head is not old_head and head.out_features == len(new_cls) == 6
    assert head.weight.device == old_w.device and head.weight.dtype == old_w.dtype and net.outc.out_channels == len(mr.ONK_NEW)
    assert torch.equal(head.weight[new_cls.index('pancreatic_lesion')], old_w[old_cls.index('pancreatic_lesion')])
    assert net.classification_branch.fused(torch.empty(1, 8, 160, device=DEV)) and net.classification_branch.tail_parameters()[13] is head.weight
    from rsuper_amd.model.dim3 import medformer_utils as mu
    gemm_compute = mu.GEMM_COMPUTE
    try:
        res = net(T(synth.image(1, mr.MODEL_SIZE, seed=1234)).to(DEV))
    finally:
        mu.GEMM_COMPUTE = gemm_compute
    assert res['classification'].shape == (1, 6) and bool(torch.isfinite(res['classification']).all())
    assert res['segmentation'][0].shape[1] == len(mr.ONK_NEW)


def test_errors():
    from rsuper_amd.graph import GraphedNetwork, GraphedTrainStep
    from rsuper_amd.model.dim3.medformer import MedFormer
    from rsuper_amd.training import losses_foundation as lf
    from rsuper_amd.training.utils import FusedAdamWEMA
    with pytest.raises(ValueError):
        MedFormer(1, 5, **{**mr.MODEL_CFG, 'chan_num': [16, 32, 64, 80, 64, 32, 16, 8], 'num_heads': [1, 2, 4, 5, 4, 2, 1, 1]}, classification_branch=True,
                  class_list_cls=['a'])
    net = MedFormer(1, 5, clip_branch=True, clip_feats=8, **mr.MODEL_CFG).to(DEV)
    with pytest.raises(ValueError, match='branches'):
        GraphedNetwork(net)
    opt = FusedAdamWEMA(net.parameters(), lr=1e-3, betas=(0.9, 0.999), eps=1e-5, weight_decay=0.0)
    with pytest.raises(ValueError, match='branches'):
        GraphedTrainStep(net, None, opt, argparse.Namespace(report_volume_loss_basic=0.0), synth.TINY_CLASSES)
    with pytest.raises(ValueError):
        lf.classification_loss(torch.zeros(2, 5, device=DEV), torch.zeros(2, 5, 16, 16, 16, dtype=torch.uint8, device=DEV), None, argparse.Namespace(), None,
                               synth.TINY_CLASSES)
