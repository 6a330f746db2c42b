"""Stands in for connectomics.common.object_utils, which the reference's
ffn/training/augmentation.py imports and its section augmentations never
call."""
