"""The basic augmentation of the reference's train.py: a random permutation of
some axes and a random reflection of some (augmentation.PermuteAndReflect,
train.py:262-267), for [z, y, x] arrays.

The reference samples both inside the TensorFlow graph (tf.random.shuffle and
tf.random.uniform) and applies them to rank-5 tensors, so train.py adds 1 to its
--permutable_axes / --reflectable_axes flags for the batch axis.  Here the axes
are the flags' own zyx numbers, the decisions come from a
numpy.random.Generator, and the transform itself runs on the device
(EvaluationOps.load_augmented); `apply` is the same transform in numpy for
hosts and tests.  TensorFlow's random number stream is NOT reproduced: a seed
gives a reproducible run of this package, not the reference's sequence of
transforms.  The distribution is the same (a uniform permutation of the
permutable axes, independent fair coins for the reflectable ones).

Section, rotation, warp and contrast augmentations are not implemented.
"""

from __future__ import annotations

from typing import Sequence, Tuple

import numpy as np

RANK = 3


class PermuteAndReflect:
  """Samples (perm, reflect) pairs.

  perm: 3 ints, the source axis of each output axis (np.transpose); the
    identity off `permutable_axes`.
  reflect: 3 values 0 / 1, whether each output axis is reversed after the
    permutation; 0 off `reflectable_axes`.
  """

  def __init__(self, permutable_axes: Sequence[int],
               reflectable_axes: Sequence[int], rng=None):
    permutable_axes = [int(x) for x in permutable_axes]
    reflectable_axes = [int(x) for x in reflectable_axes]
    # (augmentation.py:439-447 with rank = 3)
    if len(set(permutable_axes)) != len(permutable_axes):
      raise ValueError('permutable_axes must not contain duplicates')
    if len(set(reflectable_axes)) != len(reflectable_axes):
      raise ValueError('reflectable_axes must not contain duplicates')
    if not all(0 <= x < RANK for x in permutable_axes):
      raise ValueError('permutable_axes must be a subset of [0, rank-1].')
    if not all(0 <= x < RANK for x in reflectable_axes):
      raise ValueError('reflectable_axes must be a subset of [0, rank-1].')
    self.permutable_axes = np.array(permutable_axes, dtype=np.int32)
    self.reflectable_axes = np.array(reflectable_axes, dtype=np.int32)
    if rng is None or isinstance(rng, (int, np.integer)):
      rng = np.random.default_rng(rng)
    self.rng = rng

  def sample(self) -> Tuple[Tuple[int, int, int], Tuple[int, int, int]]:
    """One transform: reflection decisions first, then the permutation, as the
    reference's constructor orders them."""
    reflect = [0] * RANK
    if self.reflectable_axes.size > 0:
      decisions = self.rng.random(len(self.reflectable_axes)) > 0.5
      for axis, decision in zip(self.reflectable_axes, decisions):
        reflect[int(axis)] = int(decision)
    full_permutation = list(range(RANK))
    if self.permutable_axes.size > 0:
      permutation = self.rng.permutation(self.permutable_axes)
      for i, d in enumerate(self.permutable_axes):
        full_permutation[int(d)] = int(permutation[i])
    return tuple(full_permutation), tuple(reflect)


def check_transform(perm, reflect):
  perm = tuple(int(p) for p in perm)
  reflect = tuple(int(r) for r in reflect)
  if sorted(perm) != list(range(RANK)):
    raise ValueError('%r is not a permutation of 0, 1, 2' % (perm,))
  if len(reflect) != RANK or any(r not in (0, 1) for r in reflect):
    raise ValueError('reflect holds three values 0 / 1, got %r' % (reflect,))
  return perm, reflect


def apply(x: np.ndarray, perm, reflect) -> np.ndarray:
  """flip(transpose(x, perm), axes with reflect = 1) of a [z, y, x] array, by
  index arithmetic: out[i] = x[k] with j_a = S_a - 1 - i_a where reflect[a]
  else i_a, and k[perm[a]] = j_a."""
  perm, reflect = check_transform(perm, reflect)
  x = np.asarray(x)
  if x.ndim != RANK:
    raise ValueError('a [z, y, x] array, got shape %r' % (x.shape,))
  out_shape = tuple(x.shape[p] for p in perm)
  index = np.indices(out_shape)
  source = [None] * RANK
  for a in range(RANK):
    j = out_shape[a] - 1 - index[a] if reflect[a] else index[a]
    source[perm[a]] = j
  return x[tuple(source)]


def keeps_shape(shape, perm) -> bool:
  """Whether every axis that changes places has the size of the axis it takes
  the place of (the reference's permute_axes cannot keep a static shape
  otherwise, and the device slots have one)."""
  return all(shape[a] == shape[int(p)] for a, p in enumerate(perm))
