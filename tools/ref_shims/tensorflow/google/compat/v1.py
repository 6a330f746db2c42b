"""Stands in for tensorflow.google.compat.v1 in the reference's
ffn/training/augmentation.py: the names its function signatures mention when
the module is imported.  The numpy section augmentations call none of it."""
from tensorflow.compat.v1 import *  # noqa: F401,F403
from tensorflow.compat.v1 import Operation  # noqa: F401


class Tensor:
  pass


def function(fn=None, **kwargs):
  """@tf.function, bare or with arguments: the function as it is."""
  return fn if fn is not None else (lambda f: f)
