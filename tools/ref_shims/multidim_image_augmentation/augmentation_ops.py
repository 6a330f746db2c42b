"""Stands in for multidim_image_augmentation.augmentation_ops, which only the
reference's apply_rotation calls."""
