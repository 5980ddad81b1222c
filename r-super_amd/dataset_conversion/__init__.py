"""NIfTI CTs and masks -> the packed training cases `train_ddp --dataset abdomenatlas[_ufo] --data_root` reads, on the device: what the reference's
dataset_conversion/abdomenatlas_3d.py and dataset_conversion/nii2npz.py do with SimpleITK.

    nii_dataset.convert_case     one case: (image, PackedBits, geometry)
    nii2packed                   the command line: python -m rsuper_amd.dataset_conversion.nii2packed
"""
