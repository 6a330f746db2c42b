"""Lifecycle of the four side-unit handles on a GPU (ffn_amd/_unit.py over
csrc/ffn_unit.h): bad device ids, double close, calls on a closed handle, and
buffers that are freed with one instance, regrown and reused by the next."""

import numpy as np
import pytest

from ffn_amd import _lib

pytestmark = pytest.mark.gpu


def _volume(shape, ids):
  """Deterministic label volume over `ids`."""
  n = int(np.prod(shape))
  return np.asarray(ids, np.uint32)[(np.arange(n) // 2) % len(ids)].reshape(
      shape)


def _labels():
  from ffn_amd import labels
  return labels.LabelOps


def _seeder():
  from ffn_amd import seeding
  return seeding.Seeder


def _decision():
  from ffn_amd import decision
  return decision.DecisionOps


def _analyzer():
  from ffn_amd import analysis
  return analysis.Analyzer


def _pair_counts(ops, shape=(3, 4, 5)):
  vol = _volume(shape, (2, 4, 9))
  pa, pb, pc, ps = ops.pair_counts(vol)
  order = np.argsort(pa)
  # the slots are only meaningful to the handle: use them
  assert np.array_equal(ops.apply_pair_labels(ps, pa), vol)
  return pa[order], pb[order], pc[order]


def _edt(seeder, shape=(3, 4, 5)):
  mask = np.zeros(shape, np.uint8)
  mask[1, 2, 3] = mask[shape[0] - 1, 0, shape[2] - 1] = 1
  return (seeder.edt(mask, (2, 1, 3)),)


def _expand(ops, shape=(3, 4, 5)):
  vol = _volume(shape, (0, 0, 0, 3, 0, 0, 8))
  return ops.watershed_expand(vol, (8, 8, 33))


def _endpoint_overlaps(analyzer, shape=(3, 4, 5)):
  from ffn_amd import analysis
  probs = np.zeros(shape, np.uint8)
  seg = np.zeros(shape, np.uint64)
  return analyzer.endpoint_overlaps([analysis.EndpointInput(probs, seg)],
                                    analysis.object_table(0.5))


UNITS = {
    'LabelOps': (_labels, _pair_counts),
    'Seeder': (_seeder, _edt),
    'DecisionOps': (_decision, _expand),
    'Analyzer': (_analyzer, _endpoint_overlaps),
}


@pytest.mark.parametrize('name', sorted(UNITS))
def test_device_id_out_of_range(name):
  import torch
  cls = UNITS[name][0]()
  for device_id in (-1, torch.cuda.device_count()):
    with pytest.raises(_lib.FFNHipError, match='not present'):
      cls(device_id)


@pytest.mark.parametrize('name', sorted(UNITS))
def test_close_twice(name):
  obj = UNITS[name][0]()(0)
  assert obj.device_id == 0 and obj._h
  obj.close()
  assert not obj._h
  obj.close()
  obj.__del__()


@pytest.mark.parametrize('name', sorted(UNITS))
def test_call_on_closed_handle_raises(name):
  # a closed handle is NULL to the library, and each entry point used here
  # rejects a NULL handle ("NULL argument") before it touches the device
  cls, op = UNITS[name]
  obj = cls()(0)
  obj.close()
  with pytest.raises(_lib.FFNHipError):
    op(obj)


def _same(got, want):
  assert len(got) == len(want)
  for g, w in zip(got, want):
    assert g.dtype == w.dtype and g.shape == w.shape
    assert g.tobytes() == w.tobytes()


@pytest.mark.parametrize('name,small,large', [
    ('LabelOps', (4, 5, 6), (8, 5, 6)),
    ('Seeder', (5, 6, 7), (10, 6, 7)),
    ('DecisionOps', (4, 5, 6), (8, 5, 6)),
])
def test_second_instance_regrows_and_reuses_buffers(name, small, large):
  cls, op = UNITS[name]
  first = cls()(0)
  want = op(first, small)
  first.close()
  second = cls()(0)
  try:
    _same(op(second, small), want)
    big = op(second, large)  # every buffer is freed and allocated again
    assert all(b.size >= w.size for b, w in zip(big, want))
    _same(op(second, small), want)  # the larger buffers are kept
  finally:
    second.close()

