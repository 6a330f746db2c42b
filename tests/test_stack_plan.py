"""ffn_amd/csrc/ffn_stack_plan.h on the CPU: what a FoV's geometry fixes for the conv
kernels (conv_caps) and which kernel family runs a stack (plan_stack), through
tests/stack_plan_shim.cpp built with g++ -- no HIP, no GPU.

The expected values are restated here independently: counts from V and the chunk sizes,
spans by brute force over every chunk, the schedules from the tap formula, the plan from
the rules as a Python function."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from tests import fov_edges

HERE = os.path.dirname(os.path.abspath(__file__))

CAPS_FIELDS = ['fz', 'fy', 'fx', 'XS', 'oa0', 'oa1', 'oa2', 'permuted', 'nchunks_c',
               'nchunks_k', 'nchunks_e', 'nchunks_m', 'Rc', 'Rc_k', 'lds_bytes',
               'lds_bytes_c', 'lds_bytes_d', 'lds_bytes_e', 'k_ok', 'd_ok', 'e_ok', 'm_ok',
               't_ok', 'n_main', 'n_tail', 'n_tail3', 'n_half', 'h_geom_ok',
               'exact_variant', 'default_variant', 'act_stride']
SCHEDULES = ['dsched_aoff', 'dsched_btap', 'esched_aoff', 'tsched_aoff', 't3sched_aoff']
FAMILIES = ['Conv32', 'Conv32c', 'D160', 'D96', 'M', 'MT', 'H']

# chunk sizes (voxels) and LDS rows per dz segment of the kernel families
C_CHUNK, D_CHUNK, E_CHUNK, M_CHUNK, H_CHUNK = 144, 160, 96, 128, 80
E_ROWS, M_ROWS, T_ROWS, T3_ROWS, H_ROWS = 208, 240, 144, 208, 192
# kSched of conv32d_body: the taps of the four waves, -1 = wave 3's dummy seventh
SCHED = [[0, 1, 8, 9, 16, 18, 19], [2, 3, 10, 11, 17, 20, 21],
         [4, 5, 12, 13, 22, 23, 24], [6, 7, 14, 15, 25, 26, -1]]

FOV33 = ((33, 33, 33), (8, 8, 8), 12)
FOV_C5 = ((21, 41, 41), (5, 10, 10), 3)
FOV17 = ((17, 17, 17), (4, 4, 4), 12)
# the geometries at the limits of the rules (tests/fov_edges.py), at the depth the GPU
# tests run them with
EDGE_CASES = [pytest.param(fov, deltas, 2, id=name) for name, fov, deltas, _ in fov_edges.EDGES]
GEOMETRIES = [FOV33, FOV_C5, FOV17] + EDGE_CASES


@pytest.fixture(scope='module')
def shim(tmp_path_factory):
  out = os.path.join(str(tmp_path_factory.mktemp('stack_plan')), 'stack_plan_shim.so')
  subprocess.check_call(['g++', '-O2', '-std=c++17', '-Wall', '-Werror', '-shared', '-fPIC',
                         '-o', out, os.path.join(HERE, 'stack_plan_shim.cpp')])
  lib = ctypes.CDLL(out)
  lib.shim_caps_create.restype = ctypes.c_void_p
  lib.shim_caps_create.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_int]
  lib.shim_caps_destroy.argtypes = [ctypes.c_void_p]
  lib.shim_caps_clear_ok.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_int]
  lib.shim_caps_fields.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
  lib.shim_caps_schedule.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p]
  lib.shim_plan_stack.argtypes = [ctypes.c_void_p] + [ctypes.c_int] * 6 + [ctypes.c_void_p]
  return lib


class Caps:
  """conv_caps of one FoV: the scalar fields as attributes, the schedules by name."""

  def __init__(self, lib, fov, deltas, depth, clear_e_ok=False, clear_m_ok=False):
    self.lib = lib
    f = np.asarray(fov, np.int32)
    d = np.asarray(deltas, np.int32)
    self.handle = lib.shim_caps_create(f.ctypes.data, d.ctypes.data, depth)
    lib.shim_caps_clear_ok(self.handle, int(clear_e_ok), int(clear_m_ok))
    assert lib.shim_caps_fields(self.handle, None) == len(CAPS_FIELDS)
    vals = np.zeros(len(CAPS_FIELDS), np.int64)
    lib.shim_caps_fields(self.handle, vals.ctypes.data)
    for name, v in zip(CAPS_FIELDS, vals):
      setattr(self, name, int(v))

  def schedule(self, name):
    out = np.zeros(32, np.int32)
    self.lib.shim_caps_schedule(self.handle, SCHEDULES.index(name), out.ctypes.data)
    return out

  def plan(self, variant, flow, flow_skip, tail_batched, batch_chunks, n):
    out = np.zeros(4, np.int32)
    self.lib.shim_plan_stack(self.handle, variant, flow, flow_skip, tail_batched,
                             batch_chunks, n, out.ctypes.data)
    return FAMILIES[out[0]], bool(out[1]), int(out[2]), int(out[3])

  def __del__(self):
    self.lib.shim_caps_destroy(self.handle)


def test_counts_of_the_33_cube(shim):
  """Chunk counts of FoV 33^3, deltas 8, depth 12: they follow from V = 35,937 and the
  chunk sizes alone."""
  c = Caps(shim, *FOV33)
  assert 33 ** 3 == 35937
  assert (c.nchunks_m, c.n_main, c.n_tail, c.n_tail3) == (281, 256, 100, 34)
  assert (c.nchunks_k, c.nchunks_e, c.nchunks_c, c.n_half) == (225, 375, 250, 450)
  assert c.t_ok and c.m_ok and c.d_ok
  assert not c.permuted and (c.oa0, c.oa1, c.oa2) == (0, 1, 2)
  assert c.default_variant == 9


def _span(f, chunk, start=0):
  """Largest padded span of a chunk of `chunk` dense voxels of the layout f = (fz, fy,
  fx), chunks counted from dense voxel `start`: brute force over every chunk, on the
  padded position z plane + y XS + x of EVERY voxel of the chunk."""
  fz, fy, fx = f
  xs, plane = fx + 1, (fy + 1) * (fx + 1)
  z, y, x = np.unravel_index(np.arange(fz * fy * fx), f)
  pad = z * plane + y * xs + x
  return max(int(pad[lo:lo + chunk].max() - pad[lo:lo + chunk].min()) + 1
             for lo in range(start, fz * fy * fx, chunk))


def _rows32(span, xs, floor=256):
  return max(floor, (span + 2 * (xs + 1) + 31) // 32 * 32)


def _expected(fov, depth):
  """The spans, flags and the choice of layout of a FoV, restated."""
  v = fov[0] * fov[1] * fov[2]

  def m_fits(f):
    return _span(f, M_CHUNK) + 2 * (f[2] + 2) <= M_ROWS

  oa = (0, 1, 2)
  if not m_fits(fov):
    # the permutations in the header's order; of those that fit, the shortest rows win
    fits = [p for p in [(0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0)]
            if m_fits(tuple(fov[a] for a in p))]
    if fits:
      oa = min(fits, key=lambda p: fov[p[2]])  # (min keeps the first of equals)
  q = tuple(fov[a] for a in oa)
  halo = 2 * (q[2] + 2)
  e = {'oa': oa, 'permuted': oa != (0, 1, 2)}
  e['Rc'] = _rows32(_span(fov, C_CHUNK), fov[2] + 1)
  e['Rc_k'] = _rows32(_span(q, D_CHUNK), q[2] + 1)
  nk, ne, nm = -(-v // D_CHUNK), -(-v // E_CHUNK), -(-v // M_CHUNK)
  e['k_ok'] = e['Rc_k'] <= 320 and nk >= 2
  lds_d = max(3 * 128 * e['Rc_k'], 4 * D_CHUNK * 144 + 64)
  e['d_ok'] = e['k_ok'] and lds_d <= 160 * 1024 and depth >= 2
  lds_e = max(3 * 128 * E_ROWS, 4 * E_CHUNK * 144 + 64)
  e['e_ok'] = (e['d_ok'] and _span(q, E_CHUNK) + halo <= E_ROWS and ne >= 2 and
               lds_e <= 80 * 1024)
  e['m_ok'] = e['d_ok'] and _span(q, M_CHUNK) + halo <= M_ROWS and nm >= 2
  e['t_ok'] = False
  if e['m_ok'] and nm > 256:
    rest = v - 256 * M_CHUNK
    e['t_ok'] = (_span(q, 32, 256 * M_CHUNK) + halo <= T_ROWS and
                 _span(q, 96, 256 * M_CHUNK) + halo <= T3_ROWS and -(-rest // 32) <= 256)
  e['h_geom_ok'] = (e['t_ok'] and depth >= 2 and -(-v // H_CHUNK) >= 2 and
                    _span(q, H_CHUNK) + halo <= H_ROWS)
  e['exact_variant'] = 2 if e['Rc'] in (256, 288) else 0
  e['default_variant'] = (9 if e['t_ok'] else 8 if e['m_ok'] else 6 if e['d_ok']
                          else e['exact_variant'])
  return e


@pytest.mark.parametrize('fov,deltas,depth', GEOMETRIES)
def test_spans_flags_and_layout(shim, fov, deltas, depth):
  c = Caps(shim, fov, deltas, depth)
  want = _expected(fov, depth)
  assert (c.oa0, c.oa1, c.oa2) == want['oa']
  assert (c.fz, c.fy, c.fx) == tuple(fov[a] for a in want['oa']) and c.XS == c.fx + 1
  for name in ['permuted', 'Rc', 'Rc_k', 'k_ok', 'd_ok', 'e_ok', 'm_ok', 't_ok', 'h_geom_ok',
               'exact_variant', 'default_variant']:
    assert getattr(c, name) == want[name], (name, getattr(c, name), want[name])
  assert c.lds_bytes_c == 2 * c.Rc * 40 * 4
  assert c.lds_bytes_d == max(3 * 128 * c.Rc_k, 4 * D_CHUNK * 144 + 64)
  facts = _edge_facts(fov, depth)
  assert (c.nchunks_m, c.nchunks_k, c.lds_bytes) == (
      facts['nchunks_m'], facts['nchunks_k'], facts['lds_bytes'])
  if c.m_ok and c.nchunks_m > 256:  # (the tail counts exist with a tail, taken or not)
    assert (c.n_main, c.n_tail, c.n_tail3) == (256, facts['n_tail'], facts['n_tail3'])
  else:
    assert (c.n_main, c.n_tail, c.n_tail3) == (0, 0, 0)
  assert c.n_half == facts['n_half']
  if fov == FOV_C5[0]:
    assert c.permuted and c.fx == 21  # rows of 21
  if fov == FOV17[0]:
    assert c.nchunks_m <= 256 and not c.t_ok and c.n_main == 0 and not c.h_geom_ok


@pytest.mark.parametrize('fov,deltas,depth', GEOMETRIES)
def test_tap_schedules(shim, fov, deltas, depth):
  """Entry [w * 8 + j] of a schedule is kz 128 rows + ((ky - 1) XS + (kx - 1)) 16 for
  the tap kSched[w][j]; wave 3's dummy seventh tap repeats the sixth, and only
  dsched_btap reads 27 (the all-zero tap) there."""
  c = Caps(shim, fov, deltas, depth)
  rows = {'dsched_aoff': c.Rc_k, 'esched_aoff': E_ROWS}
  if c.nchunks_m > 256 and c.m_ok:  # (the tail schedules exist with a tail)
    rows.update(tsched_aoff=T_ROWS, t3sched_aoff=T3_ROWS)
  for name, r in rows.items():
    got = c.schedule(name)
    for w in range(4):
      for j in range(7):
        s = SCHED[w][j] if SCHED[w][j] >= 0 else SCHED[w][j - 1]
        kz, ky, kx = s // 9, (s // 3) % 3, s % 3
        assert got[w * 8 + j] == kz * 128 * r + ((ky - 1) * c.XS + (kx - 1)) * 16, (name, w, j)
    assert got[3 * 8 + 6] == got[3 * 8 + 5], name
  btap = c.schedule('dsched_btap')
  for w in range(4):
    for j in range(7):
      assert btap[w * 8 + j] == (SCHED[w][j] if SCHED[w][j] >= 0 else 27)
  assert sorted(btap.reshape(4, 8)[:, :7].ravel()) == list(range(28))


def _plan_rules(c, variant, flow, flow_skip, tail_batched, batch_chunks, n):
  """The rules of plan_stack: (family, resident, tail_tiles, chunks)."""
  tail_tiles = 1
  if variant == 0:
    family, chunks = 'Conv32', None  # (its head is never fused: no count to size)
  elif variant == 2:
    family, chunks = 'Conv32c', c.nchunks_c
  elif variant == 10 and n == 1:
    family, chunks = 'H', c.n_half
  elif variant == 9 and (n == 1 or tail_batched):
    family = 'MT'
    chunks = c.n_main + (c.n_tail if n == 1 else c.n_tail3)
    tail_tiles = 1 if n == 1 else 3
  elif variant >= 8:
    family, chunks = 'M', c.nchunks_m
  elif variant == 6 and n >= 2 and batch_chunks == 2 and c.m_ok:
    family, chunks = 'M', c.nchunks_m
  elif variant == 6 and n >= 2 and batch_chunks == 1 and c.e_ok:
    family, chunks = 'D96', c.nchunks_e
  elif variant == 7:
    family, chunks = 'D96', c.nchunks_e
  else:
    family, chunks = 'D160', c.nchunks_k
  resident = family in ('MT', 'H') and n == 1 and flow == 2 and flow_skip == 0
  return family, resident, tail_tiles, chunks


def _edge_facts(fov, depth=2):
  """What tests/fov_edges.py states about a geometry, from _span, _expected and the
  constants at the top of this file alone (nothing from the shim).  A slack is the row
  budget minus span + halo in the layout the rules choose."""
  e = _expected(fov, depth)
  q = tuple(fov[a] for a in e['oa'])
  v, halo = fov[0] * fov[1] * fov[2], 2 * (q[2] + 2)
  nm = -(-v // M_CHUNK)
  rest = v - 256 * M_CHUNK
  n_tail = -(-rest // 32) if nm > 256 else 0
  return dict(
      default=e['default_variant'], exact=e['exact_variant'], oa=e['oa'], Rc=e['Rc'],
      Rc_k=e['Rc_k'], rck_raw=_span(q, D_CHUNK) + halo,
      m_slack=M_ROWS - (_span(q, M_CHUNK) + halo),
      e_slack=E_ROWS - (_span(q, E_CHUNK) + halo),
      nchunks_m=nm, nchunks_k=-(-v // D_CHUNK), last_m=v - (nm - 1) * M_CHUNK,
      n_tail=n_tail, n_tail3=-(-rest // 96) if nm > 256 else 0,
      tail_voxels=rest - (n_tail - 1) * 32 if nm > 256 else 0,
      n_half=-(-v // H_CHUNK) if e['t_ok'] else 0,
      lds_bytes=3 * (160 + 2 * (fov[2] + 2)) * 32 * 4)


@pytest.mark.parametrize('name', sorted(fov_edges.FACTS))
def test_edge_geometries_are_still_edges(name):
  """Each geometry of tests/fov_edges.py still has the property it is in the list for,
  by brute force over its chunks and the constants above: a changed row budget or chunk
  size must not turn an edge test into a mid-range one without anyone noticing."""
  _, fov, _, what = fov_edges.BY_NAME[name]
  got = _edge_facts(fov)
  for key, want in fov_edges.FACTS[name].items():
    assert got[key] == want, (
        '%s %s (%s): %s is %s, stated %s -- the rules or their constants changed: re-run '
        'tools/fov_edges.py and pick the geometry that has this property now' %
        (name, fov, what, key, got[key], want))


def test_edge_list_covers_what_the_six_hand_picked_fovs_do_not():
  """The classes the list exists for, each met by at least one entry."""
  facts = {name: _edge_facts(fov) for name, fov, _, _ in fov_edges.EDGES}
  defaults = {f['default'] for f in facts.values()}
  assert defaults == {0, 2, 6, 8, 9}
  # (no geometry tools/fov_edges.py swept chooses (2,0,1) or (2,1,0))
  assert {f['oa'] for f in facts.values()} == {(0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0)}
  assert {f['Rc_k'] for f in facts.values() if f['default'] >= 6} == {256, 288, 320}
  assert {1, 256} <= {f['n_tail'] for f in facts.values() if f['default'] == 9}
  assert any(f['m_slack'] == 0 for f in facts.values())
  assert any(f['default'] == 9 and f['exact'] == 0 for f in facts.values())
  assert 160 * 1024 - 3 * 2 * 128 < facts['widest']['lds_bytes'] <= 160 * 1024
  assert _edge_facts(fov_edges.TOO_WIDE[1])['lds_bytes'] > 160 * 1024
  for name, fov, deltas, _ in fov_edges.EDGES + [fov_edges.TOO_WIDE]:
    assert all(f % 2 == 1 and f >= 3 and 2 * d + 1 <= f for f, d in zip(fov, deltas)), name


@pytest.mark.parametrize('fov,deltas', [FOV33[:2], ((5, 5, 5), (1, 1, 1))])
def test_depth_one_has_no_split_product_family(shim, fov, deltas):
  """Depth 1 is conv0_a, conv0_b and the head: d_ok is false, so is everything built on
  it, and the default is the exact-f32 kernel."""
  c = Caps(shim, fov, deltas, 1)
  want = _expected(fov, 1)
  assert not (c.d_ok or c.e_ok or c.m_ok or c.t_ok or c.h_geom_ok)
  assert not (want['d_ok'] or want['m_ok'] or want['t_ok'])
  assert c.exact_variant == want['exact_variant'] == 2
  assert c.default_variant == want['default_variant'] == c.exact_variant
  assert c.k_ok == want['k_ok']  # (the geometry alone: 33^3 fits conv32d's slots)
  two = Caps(shim, fov, deltas, 2)
  assert two.default_variant == (9 if fov == FOV33[0] else 2)


@pytest.mark.parametrize('clear_e_ok,clear_m_ok', [(False, False), (True, False),
                                                   (False, True), (True, True)])
def test_plan_stack_truth_table(shim, clear_e_ok, clear_m_ok):
  c = Caps(shim, *FOV33, clear_e_ok=clear_e_ok, clear_m_ok=clear_m_ok)
  assert c.e_ok == (not clear_e_ok) and c.m_ok == (not clear_m_ok)
  cases = itertools.product([0, 2, 6, 7, 8, 9, 10], [1, 2, 16], [0, 1, 2], [0, 1], [0, 1],
                            [1, 2])
  seen = set()
  for variant, n, flow, flow_skip, tail_batched, batch_chunks in cases:
    args = (variant, flow, flow_skip, tail_batched, batch_chunks, n)
    got = c.plan(*args)
    want = _plan_rules(c, *args)
    assert got[:2] == want[:2], (args, got, want)
    if want[0] == 'MT':
      assert got[2] == want[2], (args, got, want)
    if want[3] is not None:
      assert got[3] == want[3], (args, got, want)
    seen.add(got[0])
  assert seen == set(FAMILIES)


def test_plan_stack_chunks_of_the_33_cube(shim):
  """Entries per item in `count` when the head is fused, per family, at n = 1."""
  c = Caps(shim, *FOV33)
  want = {9: ('MT', 356), 8: ('M', 281), 7: ('D96', 375), 6: ('D160', 225),
          2: ('Conv32c', 250), 10: ('H', 450)}
  for variant, (family, chunks) in want.items():
    got = c.plan(variant, 2, 0, 0, 1, 1)
    assert (got[0], got[3]) == (family, chunks), (variant, got)
