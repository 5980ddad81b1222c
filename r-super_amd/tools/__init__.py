"""Command-line tools of the whole-CT path: `python -m rsuper_amd.tools.pack_dataset` (one-time conversion of a nii2npz directory to mmap-able files)."""
