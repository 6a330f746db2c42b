"""What the Python handles over the side units of libffn_hip.so share
(labels.LabelOps, seeding.Seeder, decision.DecisionOps, analysis.Analyzer,
partitions.PartitionOps, coordinates.CoordinateOps, metrics.MetricOps,
training.evaluation.EvaluationOps, training.gradients.GradientOps,
training.optimizer.OptimizerOps): the handle lifecycle, the per-device default instances, and the retry of a call
whose output arrays were too small.
"""

from __future__ import annotations

import atexit
import ctypes
import threading

from . import _lib


class Handle:
  """Owns one `ffn_*` handle: made by the library's `create` symbol on
  `device_id`, released by its `destroy` symbol in close() (at most once)."""

  def __init__(self, create: str, destroy: str, device_id: int = 0):
    self._lib = _lib.load()
    self._destroy = getattr(self._lib, destroy)
    self._h = ctypes.c_void_p()
    self.device_id = int(device_id)
    _lib.check(getattr(self._lib, create)(self.device_id,
                                          ctypes.byref(self._h)))

  def close(self):
    if self._h:
      self._destroy(self._h)
      self._h = ctypes.c_void_p()

  def __del__(self):
    try:
      self.close()
    except Exception:  # pylint:disable=broad-except
      pass


_registries = []


class Registry:
  """Process-wide default handle per device, created on first use."""

  def __init__(self, factory):
    self._factory = factory
    self._handles = {}
    self._lock = threading.Lock()
    _registries.append(self)

  def get(self, device_id: int = 0):
    with self._lock:
      h = self._handles.get(device_id)
      if h is None:
        h = self._factory(device_id)
        self._handles[device_id] = h
      return h

  def close_all(self):
    for h in list(self._handles.values()):
      try:
        h.close()
      except Exception:  # pylint:disable=broad-except
        pass
    self._handles.clear()


@atexit.register
def _close_registries():
  # release device objects while the HIP runtime is still alive
  for r in reversed(_registries):
    r.close_all()


def grow_until_fits(call, cap: int):
  """Runs `call(cap)` until its outputs fit.

  `call` allocates outputs for `cap` entries, makes the library call and
  returns (rc, found, result), `found` being the ctypes counter the library
  wrote.  A failed call that found more than `cap` entries is repeated with
  room for all of them; any other failure raises.  Returns (found, result) of
  the call that fitted.
  """
  while True:
    rc, found, result = call(cap)
    if rc != 0 and found.value > cap:
      cap = int(found.value)
      continue
    _lib.check(rc)
    return int(found.value), result
