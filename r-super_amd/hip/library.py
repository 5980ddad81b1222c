"""torch.library registration of the HIP ops: every operator of the hot path is a dispatcher op `rsuper::<name>` with a schema, a CUDA
(= HIP on ROCm) kernel registration and an autograd formula (an AutogradCUDA registration, see below) -- "the conv / norm / loss ops are
registered as custom HIP ops behind the repo's existing model/ and training/ interfaces" (BASELINE.json north_star).  The modules call
`torch.ops.rsuper.*` through the `*Fn.apply` names they always used (hip/ops.py rebinds them to the registered ops at import).

    torch.ops.rsuper.basic_block(xa, mra, xb, mrb, w1, w2, ws, pack_bufs, pack_bns, stride) -> (out, mr_out)
    torch.ops.rsuper.maxpool2(x) -> (y, mr)                    torch.ops.rsuper.upsample_trilinear(x, size) -> (y, mr)
    torch.ops.rsuper.maxpool2_skip(x) -> (y, mr, x)            (x again as the skip connection: both gradients of x meet in one backward launch)
    torch.ops.rsuper.maxpool2_skip_lazy(x, mrx) -> (y, mr, x, mrx)   (both statistics differentiable: the blocks that read them hand their gradients over
                                                                without the InstanceNorm backward tail, which the pool's backward kernel applies)
    torch.ops.rsuper.upsample_trilinear_lazy(x, size) -> (y, mr)     (the same for the block that reads the up-sampled tensor)
    torch.ops.rsuper.stem_conv(img, w, dtype) -> (y, mr)       torch.ops.rsuper.head_conv(x, w, b) -> logits
    torch.ops.rsuper.conv3(x, w) -> y                          torch.ops.rsuper.channel_norm(x, eps, relu) -> y
    torch.ops.rsuper.depthwise_conv3(x, w) -> y                torch.ops.rsuper.squeeze_excite(x, w1, b1, w2, b2) -> y
    torch.ops.rsuper.bidir_attention(fqv, mqv, heads, scale) -> (f_out, m_out)      torch.ops.rsuper.cl_planar(x, K) -> planes
loss ops (training/losses_foundation.py; reference call sites rsuper_train/training/losses_foundation.py:945-956, 541-607, 22-99, 1387-1532):
    torch.ops.rsuper.plane_partials(logits, x_off, xstride, planes, kinv, t, k, w1, w2, kflags, tpk, tpk_classes) -> (sums of term 0, sums of the other terms)
    torch.ops.rsuper.seg_from_sums(sums, cw, B, C, V, scale) -> loss
    torch.ops.rsuper.dilate_volume(vol, kernel_size) -> vol      torch.ops.rsuper.ball_search(x, diameter, sigma) -> key   (no derivative: masks / indices)
prediction post-processing (inference/detection.py, inference/postprocess.py; no derivative):
    torch.ops.rsuper.detection_volumes(x, out_shape, thresholds, erode) -> (volumes, max_prob)
    torch.ops.rsuper.detection_binary(x, out_shape, th, erode) -> counts
    torch.ops.rsuper.organ_mask(pred, lesion, organ_a, organ_b) -> planes       torch.ops.rsuper.largest_component(mask) -> mask
spatial augmentation of the loader (training/augmentation.py; no derivative):
    torch.ops.rsuper.affine_crop(img, volumes, theta, out_size, offsets) -> (image crop, volume crops)
intensity augmentation of the loader (training/augmentation.py; no derivative):
    torch.ops.rsuper.intensity_augment(img, flags, scalars, radius, taps, seeds, noise, workspace) -> img
validation metrics (metric/metrics.py; no derivative):
    torch.ops.rsuper.surface_distances(mask_gt, mask_pred, spacing, area_table) -> (sorted distances and areas per plane, counts)
    torch.ops.rsuper.edt3(codes, box, spacing, workspace) -> squared distances
crop-on-tumour from a whole CT (training/augmentation.py; no derivative):
    torch.ops.rsuper.class_counts(packed, C, plain, workspace) -> (totals, chunk table)
    torch.ops.rsuper.select_voxel(packed, C, plain, table, b, column, k, count, add) -> (z, y, x)
    torch.ops.rsuper.crop_box(img, volumes, size, pad, center, origin) -> (image crop, volume crops, corners)
report-annotated crops from a whole CT (training/augmentation.py; no derivative):
    torch.ops.rsuper.union_bbox(packed, C, plain, sets) -> count and bounding box per sample in one buffer
    torch.ops.rsuper.union_bits(packed, C, plain, b, set, box) -> bit words of the union inside the box
    torch.ops.rsuper.bits_open(bits, nx, r, add) -> (opened bits, u8 mask, count and bounding box)
    torch.ops.rsuper.label_remap(packed, C_in, C_out, nvol, masks, ones) -> remapped packed volumes
whole-CT label upload (training/dataset/packed.py; no derivative):
    torch.ops.rsuper.pack_bits(volume) -> np.packbits(volume != 0, axis = class) of a one-byte (B, C, ...) volume
Models Genesis pre-training (baselines/model_genesis/utils.py, training/losses_foundation.py):
    torch.ops.rsuper.genesis_pair(img, flags, blocks, perm, perm_off, curve, nbox, boxes, seeds, noise, workspace) -> (x, y)      (no derivative)
    torch.ops.rsuper.mse_loss(result, label) -> mean squared difference                                                       (derivative for result)
multi-task and CLIP baselines (model/dim3/medformer.py ClassificationBranch, training/losses_foundation.py, training/info_nce.py):
    torch.ops.rsuper.cls_tail(x, 15 parameters) -> (B, Nc) outputs of the branch tail                                         (derivative for all 16)
    torch.ops.rsuper.classification_loss(logits, flags_label, flags_mask, flags_unk, weights, class_set) -> loss             (derivative for logits)
    torch.ops.rsuper.info_nce(query, positive_key, temperature) -> loss                                                      (derivative for both)
whole-case preprocessing and resampling (inference/preprocess.py, inference/resample.py; no derivative):
    torch.ops.rsuper.ct_normalize(hu, lo, hi, out_shape, offset, workspace) -> (z-scored, zero-padded volume, (mean, std))
    torch.ops.rsuper.resample3d(x, box, out_size, interp, threshold) -> resampled class stack
report-guided pseudo-label refinement (baselines/pseudo_labels/pseudo_label_report_refinement.py; no derivative):
    torch.ops.rsuper.lesion_candidates(prob, n_lesions, peak_cut, min_voxels, min_peak, batch) -> (uint8 masks, per-plane state words)
lesion tables (inference/lesions.py; no derivative):
    torch.ops.rsuper.lesion_table(masks, spacing, conn, min_voxels, max_lesions, max_candidates, return_labels) -> (rows_i, rows_f, totals, labels)
    torch.ops.rsuper.label_overlap(labels_a, labels_b, Ka, Kb) -> joint histogram of two label stacks
compressed mask files (inference/npz_writer.py; no derivative):
    torch.ops.rsuper.deflate_planes(src, n, plane_stride, planes, pitch, table, header, header_bits) -> (streams back to back, offsets / sizes / CRCs)
NIfTI front and back end of a case (inference/nifti_device.py; no derivative):
    torch.ops.rsuper.nifti_load_prefilter(raw, dtype, size, strides, offset, slope, inter, prefilter) -> canonical (Z, Y, X) float32 samples / coefficients
    torch.ops.rsuper.bspline_resample(coef, ix, wx, iy, wy, iz, outside_value) -> (Zo, Yo, Xo) float32
    torch.ops.rsuper.reorient_store(stack, dst, dst_offset, plane_stride, shape_ijk, strides, offset)       (writes the planes into dst)
NIfTI CT + mask files -> a packed training case (dataset_conversion/nii_dataset.py; no derivative):
    torch.ops.rsuper.label_gather_pack(raw, desc, nclass, lut, ix, iy, iz, src_size, dst, plane, offset)    (writes one byte plane of dst, all with a lut)
    torch.ops.rsuper.label_background(packed, bg_class, offset, box)                                        (sets the synthesised background bit)
    torch.ops.rsuper.ct_normalize_pop(hu, lo, hi, out_shape, offset, workspace) -> ct_normalize with the population std (np.std)

Only a "CUDA" kernel is registered: a CPU tensor reaches no kernel and raises (the product path has no CPU fallback).

How the registration is written: the kernels of an op and its derivative already exist as the `forward` / `backward` pair of a
torch.autograd.Function in hip/ops.py (ctypes launches on the current HIP stream).  `_register` defines the schema and registers two
kernels: at the CUDA key the forward launches alone (what runs under inference_mode / below autograd), at the AutogradCUDA key the
Function itself -- forward launches plus the autograd node whose backward launches the derivative kernels.  (torch.library's
`register_autograd` wrapper was tried first: in torch 2.10 it leaves ~7 cyclic Python objects per call, closures over the argument
tensors, for the cycle collector -- 357 per UNet step -- and a collection that frees device tensors inside a hipGraph
capture aborts the process.)  The derivative launches raw kernels: eager autograd and hipGraph capture are the execution models here,
not a tracing compiler.
"""
import torch

from . import ops as _ops

LIB = torch.library.Library('rsuper', 'DEF')


class _Ctx:
    """The ctx surface an autograd.Function-style forward touches, for the forward-only CUDA kernel (nothing is kept)."""
    needs_input_grad = ()

    def save_for_backward(self, *ts):
        pass

    def mark_non_differentiable(self, *ts):
        pass

    def set_materialize_grads(self, v):
        pass


def _register_plain(name, schema, fn):
    """Define rsuper::<name> for an operator without a derivative (uint8 masks, indices): one kernel at the CUDA key."""
    LIB.define(name + schema)
    LIB.impl(name, fn, 'CUDA')
    return getattr(torch.ops.rsuper, name)


def _register(name, schema, Fn, to_fn_args=None):
    """Define rsuper::<name> with `schema`; CUDA kernel = Fn.forward alone, AutogradCUDA kernel = Fn.apply (forward + autograd node).
    to_fn_args: schema arguments -> Fn.forward arguments (default: identical)."""
    LIB.define(name + schema)

    def kernel(*args):
        c = _Ctx()
        c.needs_input_grad = (False,) * 16
        return Fn.forward(c, *(to_fn_args(*args) if to_fn_args else args))

    def with_autograd(*args):
        return Fn.apply(*(to_fn_args(*args) if to_fn_args else args))

    LIB.impl(name, kernel, 'CUDA')
    LIB.impl(name, with_autograd, 'AutogradCUDA')
    return getattr(torch.ops.rsuper, name)


class _Apply:
    """`XFn.apply(...)` as the modules call it, routed to the registered dispatcher op."""

    def __init__(self, op, adapt=None, doc=None):
        self.op, self.adapt, self.__doc__ = op, adapt, doc

    def apply(self, *args):
        return self.op(*(self.adapt(*args) if self.adapt else args))


def _bb_fn_args(xa, mra, xb, mrb, w1, w2, ws, pack_bufs, pack_bns, stride):
    return xa, mra, xb, mrb, w1, w2, ws, (None if pack_bufs is None else (list(pack_bufs), list(pack_bns))), stride


def _bb_apply_args(xa, mra, xb, mrb, w1, w2, ws, packs=None, stride=1):
    return xa, mra, xb, mrb, w1, w2, ws, (None if packs is None else list(packs[0])), (None if packs is None else list(packs[1])), stride


def install():
    """Register every op and rebind the `*Fn` names of hip/ops.py to the dispatcher entries (idempotent)."""
    if getattr(_ops, '_LIBRARY_INSTALLED', False):
        return
    reg = [
        ('BasicBlockFn', 'basic_block',
         '(Tensor xa, Tensor mra, Tensor? xb, Tensor? mrb, Tensor w1, Tensor w2, Tensor? ws, Tensor[]? pack_bufs, int[]? pack_bns, int stride) -> (Tensor, Tensor)',
         _bb_fn_args, _bb_apply_args),
        ('MaxPoolFn', 'maxpool2', '(Tensor x) -> (Tensor, Tensor)', None, None),
        ('MaxPoolSkipFn', 'maxpool2_skip', '(Tensor(a) x) -> (Tensor, Tensor, Tensor(a))', None, None),
        ('MaxPoolSkipLazyFn', 'maxpool2_skip_lazy', '(Tensor(a) x, Tensor(b) mrx) -> (Tensor, Tensor, Tensor(a), Tensor(b))', None, None),
        ('UpsampleFn', 'upsample_trilinear', '(Tensor x, int[] size) -> (Tensor, Tensor)', lambda x, size: (x, tuple(size)), None),
        ('UpsampleLazyFn', 'upsample_trilinear_lazy', '(Tensor x, int[] size) -> (Tensor, Tensor)', lambda x, size: (x, tuple(size)), None),
        ('StemFn', 'stem_conv', '(Tensor img, Tensor w, ScalarType dtype) -> (Tensor, Tensor)', None, None),
        ('HeadFn', 'head_conv', '(Tensor x, Tensor w, Tensor b) -> Tensor', None, None),
        ('Conv3Fn', 'conv3', '(Tensor x, Tensor w) -> Tensor', None, None),
        ('PlanarFn', 'cl_planar', '(Tensor x, int K) -> Tensor', None, None),
        ('SqueezeExciteFn', 'squeeze_excite', '(Tensor x, Tensor w1, Tensor b1, Tensor w2, Tensor b2) -> Tensor', None, None),
        ('BidirAttnFn', 'bidir_attention', '(Tensor fqv, Tensor mqv, int heads, float scale) -> (Tensor, Tensor)', None, None),
        ('TokenAttnFn', 'token_attention', '(Tensor qkv, int heads, float scale) -> Tensor', None, None),
        ('ChannelNormFn', 'channel_norm', '(Tensor x, float eps, bool relu) -> Tensor', None, None),
        ('DepthwiseConvFn', 'depthwise_conv3', '(Tensor x, Tensor w) -> Tensor', None, None),
        ('ClsTailFn', 'cls_tail', '(Tensor x, Tensor reducer_w, Tensor reducer_b, Tensor norm1_w, Tensor norm1_b, Tensor qkv_w, Tensor out_w, Tensor out_b, '
         'Tensor norm2_w, Tensor norm2_b, Tensor fc1_w, Tensor fc1_b, Tensor fc2_w, Tensor fc2_b, Tensor head_w, Tensor head_b) -> Tensor', None, None),
        ('InfoNceFn', 'info_nce', '(Tensor query, Tensor positive_key, float temperature) -> Tensor', None, None),
        ('ClsLossFn', 'classification_loss', '(Tensor logits, Tensor flags_label, Tensor? flags_mask, Tensor? flags_unk, Tensor? weights, int class_set) '
         '-> Tensor', None, None),
    ]
    for cls, name, schema, to_fn, adapt in reg:
        Fn = getattr(_ops, cls)
        op = _register(name, schema, Fn, to_fn)
        setattr(_ops, '_' + cls, Fn)                              # the kernel pair itself stays reachable (tests, tools)
        setattr(_ops, cls, _Apply(op, adapt, Fn.__doc__))
    _ops._LIBRARY_INSTALLED = True


def install_loss_ops(lf):
    """Register the loss operators of training/losses_foundation.py (called at the end of that module; idempotent): the fused plane sums and
    the segmentation loss from them with their derivatives, the ball dilation and the ball search as plain CUDA kernels."""
    if getattr(lf, '_LIBRARY_INSTALLED', False):
        return

    def pp_to_fn(logits, x_off, xstride, planes, kinv, t, k, w1, w2, kflags, tpk, tpk_classes):
        from ..training.dataset.packed import PackedBits
        return logits, [lf._Term(x_off[i], xstride[i], planes[i], t[i], k[i], w1[i], w2[i], kinv[i], kflags[i],
                                 None if tpk[i] is None else PackedBits(tpk[i], tpk_classes[i])) for i in range(len(planes))]

    def pp_adapt(logits, terms):
        return (logits, [tm.x_off for tm in terms], [tm.xstride for tm in terms], [tm.planes for tm in terms], [tm.kinv for tm in terms],
                [tm.t for tm in terms], [tm.k for tm in terms], [tm.w1 for tm in terms], [tm.w2 for tm in terms], [tm.kflags for tm in terms],
                [None if tm.tpk is None else tm.tpk.packed for tm in terms], [0 if tm.tpk is None else tm.tpk.C for tm in terms])

    pp = _register('plane_partials', '(Tensor logits, int[] x_off, int[] xstride, int[] planes, bool[] kinv, Tensor?[] t, Tensor?[] k, '
                   'Tensor?[] w1, Tensor?[] w2, Tensor?[] kflags, Tensor?[] tpk, int[] tpk_classes) -> (Tensor, Tensor)', lf._PartialsFn, pp_to_fn)
    sf = _register('seg_from_sums', '(Tensor sums, Tensor? cw, int B, int C, int V, float scale) -> Tensor', lf._SegFromSums)
    dv = _register_plain('dilate_volume', '(Tensor vol, int kernel_size) -> Tensor', _ops.dilate_volume)
    bs = _register_plain('ball_search', '(Tensor x, int diameter, float sigma) -> Tensor', _ops.ball_search)
    lf._PartialsFnImpl, lf._SegFromSumsImpl = lf._PartialsFn, lf._SegFromSums
    lf._PartialsFn = _Apply(pp, pp_adapt, lf._PartialsFnImpl.__doc__)
    lf._SegFromSums = _Apply(sf, None, lf._SegFromSumsImpl.__doc__)
    _ops._dilate_volume_impl, _ops._ball_search_impl = _ops.dilate_volume, _ops.ball_search
    _ops.dilate_volume, _ops.ball_search = dv, bs
    lf._LIBRARY_INSTALLED = True


_PLAIN_GROUPS = {}


def _install_plain(group, ops):
    """Register the (op name, schema, function) entries of `group` as plain CUDA kernels on first use; the registered ops, in order."""
    if group not in _PLAIN_GROUPS:
        _PLAIN_GROUPS[group] = tuple(_register_plain(name, schema, fn) for name, schema, fn in ops)
    return _PLAIN_GROUPS[group]


def install_postprocess_ops(detection_volumes, detection_binary, organ_mask, largest_component):
    """The prediction post-processing operators of inference/detection.py and inference/postprocess.py (called at the end of postprocess.py): integer
    volumes, masks and labels have no derivative."""
    return _install_plain('postprocess', (
        ('detection_volumes', '(Tensor x, int[] out_shape, float[] thresholds, bool erode, Tensor? workspace=None) -> (Tensor, Tensor)', detection_volumes),
        ('detection_binary', '(Tensor x, int[] out_shape, float th, bool erode, Tensor? workspace=None) -> Tensor', detection_binary),
        ('organ_mask', '(Tensor pred, int[] lesion, int[] organ_a, int[] organ_b) -> Tensor', organ_mask),
        ('largest_component', '(Tensor mask, Tensor? workspace=None) -> Tensor', largest_component)))


def install_augment_ops(affine_crop):
    """The spatial augmentation operator of training/augmentation.py (on its first use): a resampled crop of the loader's input has no derivative."""
    return _install_plain('augment', (
        ('affine_crop', '(Tensor img, Tensor[] volumes, Tensor theta, int[] out_size, int[] offsets) -> (Tensor, Tensor[])', affine_crop),))[0]


def install_crop_ops(class_counts, select_voxel, crop_box):
    """The crop-on-tumour operators of training/augmentation.py (on their first use): counts, a voxel index and a copied box have no derivative."""
    return _install_plain('crop', (
        ('class_counts', '(Tensor packed, int C, bool plain, Tensor? workspace=None) -> (Tensor, Tensor)', class_counts),
        ('select_voxel', '(Tensor packed, int C, bool plain, Tensor table, int b, int column, int k, int count, int[] add) -> Tensor', select_voxel),
        ('crop_box', '(Tensor? img, Tensor[] volumes, int[] size, int[] pad, Tensor? center, int[] origin) -> (Tensor, Tensor[], Tensor)', crop_box)))


def install_report_crop_ops(union_bbox, union_bits, bits_open, label_remap):
    """The report-crop operators of training/augmentation.py (on their first use): counts, boxes, bit masks and remapped labels have no derivative.
    Class sets are 64-bit sets as signed ints (the schema has no unsigned type)."""
    return _install_plain('report_crop', (
        ('union_bbox', '(Tensor packed, int C, bool plain, int[] sets) -> Tensor', union_bbox),
        ('union_bits', '(Tensor packed, int C, bool plain, int b, int set, int[] box) -> Tensor', union_bits),
        ('bits_open', '(Tensor bits, int nx, int r, int[] add) -> (Tensor, Tensor, Tensor)', bits_open),
        ('label_remap', '(Tensor packed, int C_in, int C_out, int nvol, int[] masks, int[] ones) -> Tensor[]', label_remap)))


def install_pack_ops(pack_bits):
    """The label packing operator of training/dataset/packed.py (on its first use): packed label bits have no derivative."""
    return _install_plain('pack', (('pack_bits', '(Tensor volume) -> Tensor', pack_bits),))[0]


def install_intensity_ops(intensity_augment):
    """The intensity augmentation operator of training/augmentation.py (on its first use): the loader's input has no derivative.  seeds are the 64-bit
    Philox keys as signed ints (the schema has no unsigned type)."""
    return _install_plain('intensity', (
        ('intensity_augment', '(Tensor img, int[] flags, float[] scalars, int[] radius, float[] taps, int[] seeds, '
         'Tensor? noise=None, Tensor? workspace=None) -> Tensor', intensity_augment),))[0]


def install_genesis_ops(genesis_pair):
    """The pretext-pair operator of baselines/model_genesis (on its first use): the network's input and target have no derivative.  seeds are the 64-bit
    Philox keys as signed ints (the schema has no unsigned type)."""
    return _install_plain('genesis', (
        ('genesis_pair', '(Tensor img, int[] flags, Tensor? blocks, Tensor? perm, Tensor? perm_off, Tensor? curve, int[] nbox, int[] boxes, int[] seeds, '
         'Tensor? noise=None, Tensor? workspace=None) -> (Tensor, Tensor)', genesis_pair),))[0]


_MSE = []


def install_mse_op(MseFn):
    """The voxel-wise MSE of model_genesis_loss (training/losses_foundation.py, on its first use) with its derivative."""
    if not _MSE:
        _MSE.append(_register('mse_loss', '(Tensor result, Tensor label) -> Tensor', MseFn))
    return _MSE[0]


def install_preprocess_ops(ct_normalize):
    """The whole-CT z-score of inference/preprocess.py (at the end of that module): the network's input has no derivative."""
    return _install_plain('preprocess', (
        ('ct_normalize', '(Tensor hu, float lo, float hi, int[] out_shape, int[] offset, Tensor? workspace=None) -> (Tensor, Tensor)', ct_normalize),))[0]


def install_resample_ops(resample3d):
    """The class-stack resampler of inference/resample.py (at the end of that module): labels and thresholded probabilities have no derivative."""
    return _install_plain('resample', (
        ('resample3d', '(Tensor x, int[] box, int[] out_size, str interp, float? threshold=None) -> Tensor', resample3d),))[0]


def install_metric_ops(surface_distances, edt3):
    """The validation-metric operators of metric/metrics.py (at the end of that module's setup): distances between mask surfaces have no derivative."""
    return _install_plain('metric', (
        ('surface_distances', '(Tensor mask_gt, Tensor mask_pred, float[] spacing, Tensor area_table) -> (Tensor[], Tensor)', surface_distances),
        ('edt3', '(Tensor codes, int[] box, float[] spacing, Tensor? workspace=None) -> Tensor', edt3)))


def install_pseudo_label_ops(lesion_candidates):
    """The lesion-candidate extraction of baselines/pseudo_labels (at the end of that module): masks and counters have no derivative."""
    return _install_plain('pseudo_label', (
        ('lesion_candidates', '(Tensor prob, int[] n_lesions, float peak_cut, int min_voxels, float min_peak, int batch) -> (Tensor mask, Tensor state)',
         lesion_candidates),))[0]


def install_lesion_ops(lesion_table, label_overlap):
    """The lesion-table operators of inference/lesions.py (at the end of that module's setup): integer tables, measured sizes and label volumes have
    no derivative."""
    return _install_plain('lesions', (
        ('lesion_table', '(Tensor masks, float[] spacing, int conn, int min_voxels, int max_lesions, int max_candidates, bool return_labels) '
         '-> (Tensor rows_i, Tensor rows_f, Tensor totals, Tensor labels)', lesion_table),
        ('label_overlap', '(Tensor labels_a, Tensor labels_b, int Ka, int Kb) -> Tensor', label_overlap)))


def install_deflate_ops(deflate_planes):
    """The DEFLATE encoder of inference/npz_writer.py (on its first use): compressed bytes have no derivative."""
    return _install_plain('deflate', (
        ('deflate_planes', '(Tensor src, int n, int plane_stride, int planes, int pitch, Tensor table, Tensor header, int header_bits) -> (Tensor, Tensor)',
         deflate_planes),))[0]


def install_nifti_ops(load_prefilter, bspline_resample, reorient_store):
    """The NIfTI operators of inference/nifti_device.py (at the end of that module's setup): a resampled network input and stored masks have no
    derivative."""
    return _install_plain('nifti', (
        ('nifti_load_prefilter', '(Tensor raw, int dtype, int[] size, int[] strides, int offset, float slope, float inter, bool prefilter) -> Tensor',
         load_prefilter),
        ('bspline_resample', '(Tensor coef, Tensor ix, Tensor wx, Tensor iy, Tensor wy, Tensor iz, float outside_value) -> Tensor', bspline_resample),
        ('reorient_store', '(Tensor stack, Tensor(a!) dst, int dst_offset, int plane_stride, int[] shape_ijk, int[] strides, int offset) -> ()',
         reorient_store)))


def install_nii_dataset_ops(label_gather_pack, label_background, ct_normalize_pop):
    """The dataset-conversion operators of dataset_conversion/nii_dataset.py (at the end of that module's setup): packed label bits and a z-scored
    image have no derivative."""
    return _install_plain('nii_dataset', (
        ('label_gather_pack', '(Tensor raw, Tensor desc, int nclass, Tensor? lut, Tensor ix, Tensor iy, Tensor iz, int[] src_size, Tensor(a!) dst, '
         'int plane, int[] offset) -> ()', label_gather_pack),
        ('label_background', '(Tensor(a!) packed, int bg_class, int[] offset, int[] box) -> ()', label_background),
        ('ct_normalize_pop', '(Tensor hu, float lo, float hi, int[] out_shape, int[] offset, Tensor? workspace=None) -> (Tensor, Tensor)',
         ct_normalize_pop)))
