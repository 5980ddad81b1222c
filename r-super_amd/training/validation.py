"""rsuper_train/training/validation.py: validation (:16-97) on the MI355X path.

The reference copies the thresholded prediction and the labels to the host and measures every class there (two scipy distance transforms and a
Python sort per class).  Here the prediction never leaves the device: sliding-window inference, `> 0.5`, and one batched
`surface_distances_stack` over the channels present in the ground truth, which yields the voxel counts (Dice) and the sorted surface distances
(ASD, HD95) from the same read of the masks.

Reference quirks fixed here on purpose (in the style of SURVEY Appendix A):
  * validation_ddp :129 reads `label_pred` before assigning it (the inference result is bound to `pred`): a NameError.  One function serves
    both here; `label_pred` is the thresholded inference result.
  * calculate_distance :19 slices a depth plane instead of a channel (see metric/utils.py).
  * The reference feeds bool multi-channel stacks to calculate_dice_split, whose scatter treats them as label vectors.  Here Dice is per
    channel, 2 |gt & pred| / (|gt| + |pred| + 1e-5), the reference's smoothing term included.
The networks of this port have no background channel (sigmoid outputs, args.classes = number of channels), so every channel is measured and the
returned arrays have args.classes entries, not classes - 1.
"""
import logging

import numpy as np
import torch

from ..hip.lib import RSuperHipError
from ..inference.utils import get_inference
from ..metric import metrics

CLIP = 500.0          # validation.py:69-70: nan_to_num(nan=500), clip to [0, 500]


def _label_stack(labels, C):
    """Ground truth of one case as a (C, D, H, W) bool stack: a (1, C, D, H, W) / (C, D, H, W) multi-channel mask as it is, an integer label
    map (1, 1, D, H, W) / (1, D, H, W) / (D, H, W) with channel c = (label == c + 1)."""
    if labels.dim() == 5:
        labels = labels.squeeze(0)
    if labels.dim() == 4 and labels.shape[0] == C and C > 1:
        return labels != 0
    if labels.dim() == 4 and labels.shape[0] == 1:
        labels = labels.squeeze(0)
    if labels.dim() != 3:
        raise RSuperHipError(f'validation: labels of shape {tuple(labels.shape)} for {C} classes')
    if C == 1:
        return (labels != 0).unsqueeze(0)
    ids = torch.arange(1, C + 1, device=labels.device, dtype=labels.dtype).view(C, 1, 1, 1)
    return labels.unsqueeze(0) == ids


def validation(net, dataloader, args, matcher=None, percentage=95):
    """The loader yields (images (1, 1, D, H, W), labels, spacing (1, 3)).  Returns (dice, ASD, HD) float64 numpy arrays of args.classes entries:
    per channel the mean over the cases whose ground truth has that channel (NaN for a channel no case has, as the reference's mean of an empty
    list).  ASD and HD are nan_to_num(nan=500) and clipped to [0, 500] per case.  `matcher` (the Hungarian matcher of multi-channel tumours) is
    passed through untouched: called as matcher(label_pred, labels) -> (out_ids, label_ids).  The surfel area table is resolved as
    metric/lookup_tables.py describes, or taken from args.surface_area_table."""
    net.eval()
    C = args.classes
    dice_list, ASD_list, HD_list = ([[] for _ in range(C)] for _ in range(3))
    inference = get_inference(args)
    dev = next(net.parameters()).device
    logging.info('Evaluating')
    with torch.no_grad():
        for images, labels, spacing in dataloader:
            if images.shape[0] != 1:
                raise RSuperHipError('validation: one case per batch (the cases of a test set differ in shape)')
            inputs, labels = images.float().to(dev), labels.to(dev)
            label_pred = inference(net, inputs, args, to_cpu=False) > 0.5
            if matcher is not None:
                out_ids, label_ids = matcher(label_pred, labels)
                label_pred, labels = label_pred[out_ids], labels[label_ids]
            label_pred = label_pred.squeeze(0)
            gt = _label_stack(labels, C)
            if gt.shape != label_pred.shape:
                raise RSuperHipError(f'validation: prediction {tuple(label_pred.shape)} against labels {tuple(gt.shape)}')
            present = torch.nonzero(gt.flatten(1).any(1)).flatten().tolist()       # only classes in the ground truth are evaluated (:80-87)
            if not present:
                continue
            whole = present == list(range(C))
            sp = [float(s) for s in np.asarray(spacing[0].cpu() if hasattr(spacing[0], 'cpu') else spacing[0]).reshape(-1)]
            res, counts = metrics.surface_distances_stack(gt if whole else gt[present], label_pred if whole else label_pred[present], sp,
                                                          getattr(args, 'surface_area_table', None))
            counts = counts.cpu().numpy()
            for k, c in enumerate(present):
                a, b = metrics.compute_average_surface_distance(res[k])
                asd, hd = (a + b) / 2, metrics.compute_robust_hausdorff(res[k], percentage)
                ASD_list[c].append(float(np.clip(np.nan_to_num(asd, nan=CLIP), 0, CLIP)))
                HD_list[c].append(float(np.clip(np.nan_to_num(hd, nan=CLIP), 0, CLIP)))
                dice_list[c].append(2.0 * counts[k, 2] / (counts[k, 0] + counts[k, 1] + 1e-5))

    def mean(v):
        return float(np.mean(v)) if v else float('nan')
    return (np.array([mean(v) for v in dice_list]), np.array([mean(v) for v in ASD_list]), np.array([mean(v) for v in HD_list]))
