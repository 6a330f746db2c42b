"""The scaffold the four side-unit handles share (ffn_amd/_unit.py), against a
stub standing in for the loaded library: no GPU, no libffn_hip.so."""

import ctypes

import pytest

from ffn_amd import _lib
from ffn_amd import _unit


class StubLib:
  """create / destroy that count their calls; create hands out handle 0x1000,
  0x1001, ... unless `create_rc` is non-zero."""

  def __init__(self, create_rc=0):
    self.create_rc = create_rc
    self.created = []
    self.destroyed = []

  def stub_create(self, device_id, out):
    self.created.append(device_id)
    if self.create_rc == 0:
      out._obj.value = 0x1000 + len(self.created) - 1
    return self.create_rc

  def stub_destroy(self, h):
    self.destroyed.append(h.value)

  def ffn_last_error(self):
    return b'stub error'


@pytest.fixture
def stub(monkeypatch):
  lib = StubLib()
  monkeypatch.setattr(_lib, 'load', lambda: lib)
  return lib


def _handle(device_id=0):
  return _unit.Handle('stub_create', 'stub_destroy', device_id)


def test_close_twice_destroys_once(stub):
  h = _handle(3)
  assert h.device_id == 3 and stub.created == [3]
  h.close()
  h.close()
  assert stub.destroyed == [0x1000]


def test_del_after_close_calls_nothing(stub):
  h = _handle()
  h.close()
  h.__del__()
  assert stub.destroyed == [0x1000]


def test_del_closes_and_swallows_a_raising_destroy(stub):
  h = _handle()
  h.__del__()
  assert stub.destroyed == [0x1000]

  def boom(h):
    raise RuntimeError('destroy failed')
  h2 = _handle()
  h2._destroy = boom
  h2.__del__()  # must not raise


def test_failed_create_raises_and_leaves_no_handle(stub):
  stub.create_rc = -2
  h = _unit.Handle.__new__(_unit.Handle)  # (to look at the half-made object)
  with pytest.raises(_lib.FFNHipError, match='stub error'):
    h.__init__('stub_create', 'stub_destroy', 0)
  assert stub.created == [0]
  assert not h._h
  h.close()
  h.__del__()
  assert stub.destroyed == []


@pytest.fixture
def registry(stub):
  del stub
  r = _unit.Registry(_handle)
  yield r
  _unit._registries.remove(r)


def test_registry_one_handle_per_device(registry):
  a = registry.get(0)
  assert registry.get(0) is a
  b = registry.get(1)
  assert b is not a and registry.get(1) is b
  assert (a.device_id, b.device_id) == (0, 1)


def test_exit_hook_closes_each_handle_once(stub, registry):
  a, b = registry.get(0), registry.get(1)
  assert registry in _unit._registries
  _unit._close_registries()
  assert sorted(stub.destroyed) == [0x1000, 0x1001]
  assert not a._h and not b._h
  _unit._close_registries()  # nothing left to close
  assert sorted(stub.destroyed) == [0x1000, 0x1001]


def test_exit_hook_survives_a_raising_close(stub, registry):
  a, b, c = registry.get(0), registry.get(1), registry.get(2)

  def boom():
    raise RuntimeError('close failed')
  b.close = boom
  _unit._close_registries()
  assert sorted(stub.destroyed) == [0x1000, 0x1002]
  assert not a._h and not c._h
  del b.close
  b.close()


# -- grow_until_fits ----------------------------------------------------------------


def _call(script):
  """call(cap) that answers from `script`, a list of (rc, found), and records
  the capacities it was given."""
  caps = []

  def call(cap):
    rc, found = script[len(caps)]
    caps.append(cap)
    return rc, ctypes.c_size_t(found), ('outputs for cap', cap)
  return call, caps


def test_grow_repeats_once_with_the_found_count(stub):
  del stub
  call, caps = _call([(-2, 250), (0, 250)])
  assert _unit.grow_until_fits(call, 100) == (250, ('outputs for cap', 250))
  assert caps == [100, 250]


def test_grow_raises_when_the_outputs_were_large_enough(stub):
  del stub
  for found in (100, 7):
    call, caps = _call([(-2, found), (0, found)])
    with pytest.raises(_lib.FFNHipError, match='stub error'):
      _unit.grow_until_fits(call, 100)
    assert caps == [100]


def test_grow_does_not_repeat_a_success(stub):
  del stub
  call, caps = _call([(0, 40), (0, 40)])
  assert _unit.grow_until_fits(call, 100) == (40, ('outputs for cap', 100))
  assert caps == [100]
  # nor a success that reports more than cap (the library never does)
  call, caps = _call([(0, 250), (0, 250)])
  assert _unit.grow_until_fits(call, 100)[0] == 250
  assert caps == [100]
