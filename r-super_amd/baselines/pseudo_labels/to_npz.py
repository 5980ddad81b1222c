"""Organ labels + refined pseudo-labels -> the per-voxel training label (rsuper_train/baselines/pseudo_labels/to_npz.py process_file :34-63, the branch
for cases no radiologist annotated), on the device: the result is what `WholeVolumeDataset` / `tools.pack_dataset` train from, optionally already in
the bit-packed form (`pack_bits_device`)."""
import torch

from ...hip import lib as _l


def merge_plan(organ_names, lesion_masks, label_names):
    """Where every output plane comes from, host logic only: [('organ', index into organ_names) | ('lesion', label) | ('zeros', label)] for the labels in
    sorted order.  lesion_masks: the labels that have a pseudo mask (any container)."""
    organ_at = {name: i for i, name in enumerate(organ_names)}
    plan = []
    for label in sorted(label_names):
        if label in organ_at:
            plan.append(('organ', organ_at[label]))
        else:
            assert 'lesion' in label, f'{label!r} is neither an organ plane nor a lesion class'
            plan.append(('lesion', label) if label in lesion_masks else ('zeros', label))
    return plan


def merge_pseudo_labels(organs, organ_names, lesion_masks, label_names, packed=False):
    """organs: one-byte device tensor (len(organ_names), D, H, W), plane i is the organ organ_names[i]; lesion_masks: {lesion class: (D, H, W) device mask},
    e.g. refine_case's; label_names: the target label list.  Returns uint8 (len(label_names), D, H, W) on the device with the labels in sorted order
    (to_npz.py sorts the list before it stacks, :132): an organ plane is taken by name, a lesion plane is the pseudo mask or zeros where the case has
    none.  A label that is neither an organ nor has 'lesion' in its name raises AssertionError, as in the reference.

    packed=True passes the stack through pack_bits_device and returns the PackedBits whose `.packed[0]` is np.packbits(stack, axis=0), the array
    tools.pack_dataset writes as `<id>_gt.npy`."""
    if not isinstance(organs, torch.Tensor) or not organs.is_cuda:
        raise _l.RSuperHipError('merge_pseudo_labels: the organ labels must be on the MI355X device (no CPU fallback)')
    if organs.dim() != 4 or organs.shape[0] != len(organ_names) or organs.element_size() != 1:
        raise ValueError(f'merge_pseudo_labels: one-byte (len(organ_names), D, H, W) organs, got {organs.dtype} {tuple(organs.shape)}')
    zeros = None
    planes = []
    for kind, key in merge_plan(organ_names, lesion_masks, label_names):
        if kind == 'organ':
            plane = organs[key]
        elif kind == 'lesion':
            plane = lesion_masks[key]
            if not plane.is_cuda or tuple(plane.shape) != tuple(organs.shape[1:]):
                raise ValueError(f'merge_pseudo_labels: the mask of {key} must be a device tensor of shape {tuple(organs.shape[1:])}')
        else:
            if zeros is None:
                zeros = torch.zeros(organs.shape[1:], device=organs.device, dtype=torch.uint8)
            plane = zeros
        planes.append(plane.view(torch.uint8) if plane.element_size() == 1 else plane.to(torch.uint8))
    out = torch.stack(planes)
    if packed:
        from ...training.dataset.packed import pack_bits_device
        return pack_bits_device(out)
    return out
