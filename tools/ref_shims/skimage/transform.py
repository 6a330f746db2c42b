"""Stands in for skimage.transform so that the reference's
ffn/training/augmentation.py imports.  Nothing here computes: the elastic and
affine augmentations, which need the real functions, cannot be minted."""


def _missing(*args, **kwargs):
  raise NotImplementedError('skimage.transform is not installed')


AffineTransform = _missing
warp = _missing
