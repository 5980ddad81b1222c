"""Validation metrics mirroring rsuper_train/metric on the MI355X path: surface distances, average surface distance, robust Hausdorff,
surface Dice (NSD) and Dice, computed from device masks by the kernels of csrc/surfdist.hip."""
from .lookup_tables import ENCODE_NEIGHBOURHOOD_3D_KERNEL, set_surface_area_table_fn, resolve_surface_area_table  # noqa: F401
from .metrics import (compute_surface_distances, compute_average_surface_distance, compute_robust_hausdorff,  # noqa: F401
                      compute_surface_overlap_at_tolerance, compute_surface_dice_at_tolerance, compute_dice_coefficient,
                      surface_distances_stack, edt3)
from .utils import calculate_distance, calculate_dice, calculate_dice_split  # noqa: F401
