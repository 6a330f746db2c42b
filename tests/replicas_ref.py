"""Oracle for the aggregation of replica gradients (include/ffn_optimizer.h,
aggregate): the header's definition restated in numpy with one explicit
np.float32 operation per written operation, on top of tests/optimizer_ref.py's
clip.  numpy's f32 add and divide round once each and never contract, so the
result is the definition's, bit for bit.
"""

import numpy as np

from tests import optimizer_ref

F32 = np.float32


def fold(arrays, clip):
  """arrays: the n replica arrays in replica order -> clip each, add them left
  to right, divide by f32(n)."""
  arrays = [np.asarray(a, F32) for a in arrays]
  clip = F32(clip)
  with np.errstate(all='ignore'):
    t = optimizer_ref.clip_gradient(arrays[0], clip).astype(F32)
    for a in arrays[1:]:
      c = optimizer_ref.clip_gradient(a, clip).astype(F32)
      t = np.add(t, c, dtype=F32)
    out = np.divide(t, F32(len(arrays)), dtype=F32)
  assert out.dtype == F32
  return out


def fold_strided(src, count, n, stride, clip):
  """The fold over the n arrays of `count` floats that lie `stride` floats
  apart in the flat array `src`."""
  src = np.asarray(src, F32)
  return fold([src[r * stride:r * stride + count] for r in range(n)], clip)


#: (a + b) + c = 0 but a + (b + c) = 1 in f32: 1 is below half an ulp of 2^24
ORDER_TRIPLE = (F32(1.0), F32(16777216.0), F32(-16777216.0))
#: the same inside a clip of 0.7: 2^-25 is half an ulp of 0.5, the tie goes to
#: the even 0.5, so (a + b) + c = 0 and a + (b + c) = 2^-25
ORDER_TRIPLE_SMALL = (F32(2.0 ** -25), F32(0.5), F32(-0.5))
