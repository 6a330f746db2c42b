"""Stands in for tensorflow.experimental.numpy (imported, never called by the
section augmentations)."""
