#!/usr/bin/env python3
"""Golden vectors for the multi-task and CLIP baselines from the UNMODIFIED reference, imported on the CPU in the authoring container
(rsuper_train/model/dim3/medformer.py ClassificationBranch / MedFormer, training/losses_foundation.py classification_loss / calculate_loss,
training/info_nce.py):

    python tests/golden/gen_golden_mtl.py   ->  tests/golden/mtl.npz

Inputs and parameters are regenerated from seeds by the tests (tests/mtl_ref.py holds the seeds and shapes); stored are outputs, gradients (whole
where small, strided samples + summaries otherwise) and the sorted parameter names and shapes.  Branch alone: besides the branch's outputs the input
of its tail (the extra layer's output as tokens) and the gradient that reaches it are stored, so the tail can be compared on the same operands.
The one-token case L1 is the reference class without its extra layer (see main).
"""
import argparse
import importlib
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import synth  # noqa: E402
import mtl_ref as mr  # noqa: E402

REF = '/root/reference/rsuper_train'
T = torch.from_numpy


def import_reference():
    nib = types.ModuleType('nibabel')
    nib.Nifti1Image = lambda *a, **k: None
    nib.save = lambda *a, **k: None
    sys.modules['nibabel'] = nib
    sys.path.insert(0, REF)
    for name, sub in (('model', 'model'), ('model.dim3', 'model/dim3')):       # bypass model/__init__ (MONAI / timm nets)
        m = types.ModuleType(name)
        m.__path__ = [os.path.join(REF, sub)]
        sys.modules[name] = m
    mf = importlib.import_module('model.dim3.medformer')
    lf = importlib.import_module('training.losses_foundation')
    nce = importlib.import_module('training.info_nce')
    lf.counter = lf.counter2 = lf.counter3 = 99
    return mf, lf, nce


def load(module, seed):
    shapes = {k: tuple(v.shape) for k, v in module.state_dict().items()}
    module.load_state_dict({k: T(v) for k, v in mr.fill(shapes, seed).items()})
    return shapes


def store_grad(out, key, g, n=256):
    g = g.detach().numpy()
    out[key + '_summary'] = synth.summary(g)
    if n:
        out[key + '_sub'], _ = synth.subsample(g, n)


def main():
    mf, lf, nce = import_reference()
    torch.manual_seed(0)
    torch.set_num_threads(8)
    out = {}
    mu = importlib.import_module('model.dim3.medformer_utils')
    utils = importlib.import_module('model.dim3.utils')

    def extra_layer():
        return mu.down_block(320, 160, 0, 1, conv_block=utils.get_block('BasicBlock'), kernel_size=[3, 3, 3], down_scale=[2, 2, 2], heads=4, dim_head=20,
                             expansion=4, attn_drop=0., proj_drop=0., map_size=[2, 2, 2], proj_type='depthwise', norm=utils.get_norm('in'),
                             act=utils.get_act('relu'), map_generate=True)

    # ---- branch alone
    for tag in mr.BRANCH_SHAPES:
        for nc in mr.BRANCH_NC:
            # L1: the reference cannot run its extra layer down to one voxel (InstanceNorm3d refuses a single spatial element), so the one-token case
            # is the reference class without an extra layer on a (1, 160, 1, 1, 1) input -- its tail on one token
            br = mf.ClassificationBranch(num_classes=nc, extra_layer=None if tag == 'L1' else extra_layer())
            shapes = load(br, mr.BRANCH_SEED)
            key = f'branch_{tag}_{nc}'
            if tag in ('L8', 'L1'):     # the other cases have L8's parameters
                out[key + '_names'] = np.array(sorted(shapes))
                out[key + '_shapes'] = np.array([','.join(str(d) for d in shapes[k]) for k in sorted(shapes)])
            x = T(mr.x4(tag) if tag != 'L1' else mr.x4(tag)[:, :160, :1, :1, :1].copy()).requires_grad_(True)
            keep = {}

            def grab(mod, inp, o):
                inp[0].retain_grad()
                keep['x'] = inp[0]
            h = br.reducer.register_forward_hook(grab)
            y = br(x)
            h.remove()
            (y * T(mr.out_grad(tag, nc))).sum().backward()
            xt = keep['x']                                                      # (B, 160, d, h, w)
            out[key + '_out'] = y.detach().numpy()
            store_grad(out, key + '_dx4', x.grad, 1024)
            if nc == mr.BRANCH_NC[0]:
                out[f'branch_{tag}_xtail'] = xt.detach().flatten(2).permute(0, 2, 1).contiguous().numpy()      # (B, L, 160) tokens
            dxt = xt.grad.flatten(2).permute(0, 2, 1).contiguous()
            store_grad(out, key + '_dxtail', dxt, dxt.numel() if nc == mr.BRANCH_NC[0] else 1024)      # whole for the first class count
            for k, p in br.named_parameters():
                # the extra layer's gradients: summaries here, samples in the whole-model case; tail: whole up to 4096 elements, else a sample
                store_grad(out, f'{key}_g_{k}', p.grad, 0 if k.startswith('extra_layer') else (p.numel() if p.numel() <= 4096 else 1024))

    # ---- whole model, 64^3, both branches
    cfg = mr.MODEL_CFG
    net = mf.MedFormer(1, len(synth.TINY_CLASSES), base_chan=cfg['base_chan'], map_size=cfg['map_size'], conv_block='BasicBlock', conv_num=cfg['conv_num'],
                       trans_num=cfg['trans_num'], chan_num=cfg['chan_num'], num_heads=cfg['num_heads'], fusion_depth=cfg['fusion_depth'],
                       fusion_dim=cfg['fusion_dim'], fusion_heads=cfg['fusion_heads'], expansion=4, proj_type='depthwise', norm='in', act='relu',
                       kernel_size=[[3, 3, 3]] * 5, scale=[[2, 2, 2]] * 4, aux_loss=True, classification_branch=True, class_list_cls=mr.MODEL_CLS,
                       clip_branch=True, clip_feats=mr.MODEL_CLIP)
    shapes = load(net, mr.MODEL_SEED)
    out['model_names'] = np.array(sorted(shapes))
    out['model_shapes'] = np.array([','.join(str(d) for d in shapes[k]) for k in sorted(shapes)])
    res = net(T(synth.image(1, mr.MODEL_SIZE, seed=1234)))
    y, aux = res['segmentation']
    go = synth.rng(77).standard_normal(tuple(y.shape)).astype(np.float32) / y.numel()
    ga = synth.rng(78).standard_normal(tuple(aux.shape)).astype(np.float32) / aux.numel()
    gc = synth.rng(79).standard_normal(tuple(res['classification'].shape)).astype(np.float32)
    ge = synth.rng(80).standard_normal(tuple(res['clip'].shape)).astype(np.float32)
    ((y * T(go)).sum() + (aux * T(ga)).sum() + (res['classification'] * T(gc)).sum() + (res['clip'] * T(ge)).sum()).backward()
    out['model_classification'], out['model_clip'] = res['classification'].detach().numpy(), res['clip'].detach().numpy()
    for nm, t in (('logits', y), ('aux', aux)):
        out[f'model_{nm}_sub'], _ = synth.subsample(t.detach().numpy(), 4096)
        out[f'model_{nm}_summary'] = synth.summary(t.detach().numpy())
    for k, p in net.named_parameters():
        store_grad(out, f'model_g_{k}', p.grad)
    # the same model and input in float64: what the branch outputs of the float32 run above, and of the device, are measured against
    import copy
    with torch.no_grad():
        res64 = copy.deepcopy(net).double()(T(synth.image(1, mr.MODEL_SIZE, seed=1234)).double())
    out['model_classification_f64'], out['model_clip_f64'] = res64['classification'].numpy(), res64['clip'].numpy()

    # ---- classification_loss
    args = argparse.Namespace()
    for name, (lab, unk, msk, cw) in mr.loss_cases().items():
        x = T(mr.loss_logits()).requires_grad_(True)
        l = lf.classification_loss(x, T(lab), None if unk is None else T(unk), args, T(msk), mr.LOSS_CLASSES, None if cw is None else T(cw))
        l.backward()
        out[f'cls_{name}_value'], out[f'cls_{name}_grad'] = l.detach().numpy(), x.grad.numpy()

    # ---- info_nce and calculate_loss(clip_only=True)
    for n, d in mr.NCE_SHAPES:
        q, k = (T(a).requires_grad_(True) for a in mr.nce_inputs(n, d))
        l = nce.info_nce(q, k)
        l.backward()
        out[f'nce_{n}_{d}_value'], out[f'nce_{n}_{d}_dq'], out[f'nce_{n}_{d}_dk'] = l.detach().numpy(), q.grad.numpy(), k.grad.numpy()

    class Dist:
        @staticmethod
        def get_world_size():
            return 2
    q, k = (T(a) for a in mr.nce_inputs(2, 768))
    q.requires_grad_(True)
    seg = [torch.zeros(2, 5, 4, 4, 4, requires_grad=True), torch.zeros(2, 5, 4, 4, 4, requires_grad=True)]
    l = lf.calculate_loss({'segmentation': seg, 'clip': q}, None, None, args, None, None, None, None, mr.LOSS_CLASSES, clip_only=True, report_embeddings=k,
                          dist=Dist)
    assert sorted(l) == ['contrastive_loss', 'overall']
    l['overall'].backward()
    out['clip_only_value'], out['clip_only_dq'] = l['overall'].detach().numpy(), q.grad.numpy()

    # ---- update_output_layer_onk on a carrier with a classification branch head (outc, aux_out, head are all the function touches)
    import torch.nn as nn

    class Carrier(nn.Module):
        def __init__(self, n, n_cls):
            super().__init__()
            self.aux_loss = True
            self.outc = nn.Conv3d(8, n, kernel_size=1)
            self.aux_out = nn.Conv3d(32, n, kernel_size=1)
            self.classification_branch = nn.Module()
            self.classification_branch.head = nn.Linear(64, n_cls)
    for tag, copy_pancreas in (('plain', False), ('copy_pancreas', True)):
        car = Carrier(len(mr.ONK_OLD), len([c for c in mr.ONK_OLD if 'lesion' in c]))
        load(car, 11)
        torch.manual_seed(mr.ONK_SEED)
        mf.update_output_layer_onk(car, original_classes=mr.ONK_OLD, new_classes=mr.ONK_NEW, copy_pancreas=copy_pancreas)
        for k, v in car.state_dict().items():
            out[f'onk_{tag}.{k}'] = v.numpy().copy()

    path = os.path.join(HERE, 'mtl.npz')
    np.savez_compressed(path, **out)
    print('wrote', path, os.path.getsize(path) // 1024, 'kB,', len(out), 'arrays')


if __name__ == '__main__':
    main()
