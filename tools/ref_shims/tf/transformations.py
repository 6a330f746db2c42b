"""Stands in for the `tf.transformations` package (quaternion helpers) that
the reference's ffn/training/augmentation.py imports for its rotations."""
