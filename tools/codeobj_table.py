#!/usr/bin/env python
"""tools/codeobj_table.py LIB: the gfx950 kernels of a build of the HIP library, one line
per kernel, sorted by symbol: what the compiler says about it in the code object's metadata
(registers, spills, scratch, LDS, kernel arguments, workgroup size) and the size of its
code (llvm-readelf -s).  Two builds whose tables are equal hold the same kernels; no GPU
needed.  (The code object a kernel comes from is not printed: it changes with the order of
the units alone.)
"""

import os
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..'))
from tests import codeobj  # noqa: E402

COLUMNS = ('vgpr_count', 'agpr_count', 'sgpr_count', 'vgpr_spill_count', 'sgpr_spill_count',
           'private_segment_fixed_size', 'group_segment_fixed_size', 'kernarg_segment_size',
           'max_flat_workgroup_size')


def table(lib_path):
  """[(symbol, {column: int, 'code_bytes': int})] sorted by symbol"""
  with tempfile.TemporaryDirectory() as tmp:
    notes = codeobj.kernel_notes_by_object(lib_path, tmp)
    sizes = {}
    for k in sorted({k for k, _, _ in notes}):
      sizes[k] = codeobj.symbol_sizes(os.path.join(tmp, 'co%d.elf' % k))
  return sorted((name, dict(fields, code_bytes=sizes[k].get(name, -1)))
                for k, name, fields in notes)


def main():
  if len(sys.argv) != 2:
    sys.exit(__doc__)
  print('# ' + ' '.join(COLUMNS + ('code_bytes', 'symbol')))
  for name, row in table(sys.argv[1]):
    print(' '.join(str(row.get(c, -1)) for c in COLUMNS + ('code_bytes',)) + ' ' + name)


if __name__ == '__main__':
  main()
