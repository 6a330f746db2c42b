"""The production form of the resident stack against its LAB form, as the compiler built
them into libffn_hip.so: the point of the production form is what it does NOT carry --
fewer scalar registers spilled to lanes between the tap loops, no more scratch, fewer
kernel arguments.  Read from the AMDGPU metadata notes of the library's gfx950 code objects
(tests/codeobj.py), both kernels from the same build: relative checks, no numbers of a
particular compiler.  No GPU needed.
"""

import collections
import re

from ffn_amd import _lib
from tests import codeobj


def test_production_stack_carries_less_than_the_lab_stack(tmp_path):
  kernels = codeobj.kernel_notes(_lib.LIB_PATH, tmp_path)
  forms = {}
  for name, fields in kernels.items():
    m = re.match(r'_ZN3ffn15conv32ps_kernelILb([01])E', name)
    if m:
      forms[m.group(1) == '1'] = fields
  assert set(forms) == {True, False}, sorted(k for k in kernels if 'conv32ps' in k)
  lab, prod = forms[True], forms[False]
  print('conv32ps LAB %s\nconv32ps production %s' % (lab, prod))
  assert prod['sgpr_spill_count'] < lab['sgpr_spill_count']
  assert prod['private_segment_fixed_size'] <= lab['private_segment_fixed_size']
  assert prod['kernarg_segment_size'] < lab['kernarg_segment_size']


def test_every_kernel_is_in_one_code_object(tmp_path):
  """Without relocatable device code a unit that names a kernel gets a device copy and a
  registration of its own: an attribute set through one unit's copy would not reach a
  launch made through another's.  So every kernel symbol of the library comes from ONE
  unit.  Two kinds of names are a unit's own business and may recur: kernels in an
  anonymous namespace, and the id-table templates of ffn_table.h, which every side unit
  that keeps such a table instantiates for its own launches (no attribute is set on them)."""
  where = collections.defaultdict(list)
  for k, name, _ in codeobj.kernel_notes_by_object(_lib.LIB_PATH, tmp_path):
    where[name].append(k)
  assert len(where) > 100, 'the notes of the library were not read: %d kernels' % len(where)
  assert any('conv32mt_kernel' in name for name in where)
  twice = {name: ks for name, ks in where.items()
           if len(ks) > 1 and not name.startswith(('_ZN12_GLOBAL__N_1', '_ZN9ffn_table'))}
  assert not twice, twice
