"""Report-refined pseudo-labels (rsuper_train/baselines/pseudo_labels of the reference) on the device."""
from .pseudo_label_report_refinement import (DEFAULT_BATCH, dump_yaml, extract_lesion_candidates, last_state, load_yaml, refine_case,  # noqa: F401
                                             slice_indices)
from .to_npz import merge_pseudo_labels  # noqa: F401
