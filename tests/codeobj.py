"""What the compiler built into a HIP library, read without a GPU: the gfx950 code objects
of its offload bundles and the AMDGPU metadata notes of their kernels (llvm-readelf).
Shared by tests/test_lean_stack_codeobj.py and tools/codeobj_table.py.
"""

import os
import re
import struct
import subprocess

_MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'

#: the metadata fields read per kernel
FIELDS = ('sgpr_spill_count', 'private_segment_fixed_size', 'kernarg_segment_size',
          'vgpr_spill_count', 'vgpr_count', 'sgpr_count', 'agpr_count',
          'group_segment_fixed_size', 'max_flat_workgroup_size')


def readelf():
  for root in (os.environ.get('ROCM_PATH', '/opt/rocm'), '/opt/rocm'):
    path = os.path.join(root, 'llvm', 'bin', 'llvm-readelf')
    if os.path.exists(path):
      return path
  raise FileNotFoundError('llvm-readelf of the ROCm tree not found')


def code_objects(lib_bytes):
  """the gfx950 code objects of every offload bundle in the library"""
  at = 0
  while True:
    at = lib_bytes.find(_MAGIC, at)
    if at < 0:
      return
    (count,) = struct.unpack_from('<Q', lib_bytes, at + len(_MAGIC))
    p = at + len(_MAGIC) + 8
    for _ in range(count):
      off, size, tlen = struct.unpack_from('<QQQ', lib_bytes, p)
      triple = lib_bytes[p + 24:p + 24 + tlen].decode()
      p += 24 + tlen
      if 'gfx950' in triple and size:
        yield lib_bytes[at + off:at + off + size]
    at += len(_MAGIC)


def extract(lib_path, tmp_path):
  """writes the library's code objects to tmp_path; returns their paths in order"""
  assert os.path.exists(lib_path), 'build the library first (__graft_entry__.build())'
  with open(lib_path, 'rb') as f:
    data = f.read()
  paths = []
  for k, co in enumerate(code_objects(data)):
    path = os.path.join(str(tmp_path), 'co%d.elf' % k)
    with open(path, 'wb') as f:
      f.write(co)
    paths.append(path)
  return paths


def kernel_notes_by_object(lib_path, tmp_path):
  """[(code object index, kernel symbol, {metadata field: int})] of every kernel of every
  code object, in the order of the library"""
  found = []
  for k, path in enumerate(extract(lib_path, tmp_path)):
    text = subprocess.check_output([readelf(), '--notes', path], text=True)
    # amdhsa.kernels: a list of maps at indent 2; a kernel's own keys stand at indent 4
    # (the first one behind the '- '), those of its '.args' deeper
    own = r'(?m)^(?:    |  - )\.%s:\s+(\S+)'
    for block in re.split(r'(?m)^  - (?=\.)', text)[1:]:
      block = '  - ' + block
      names = re.findall(own % 'name', block)
      if not names or 'kernarg_segment_size' not in block:
        continue
      fields = {}
      for key in FIELDS:
        m = re.findall(own % key, block)
        if m:
          fields[key] = int(m[-1])
      found.append((k, names[-1].strip("'\""), fields))
  return found


def kernel_notes(lib_path, tmp_path):
  """{kernel symbol: {metadata field: int, 'code_object': index}} of the library"""
  return {name: dict(fields, code_object=k)
          for k, name, fields in kernel_notes_by_object(lib_path, tmp_path)}


def symbol_sizes(path):
  """{function symbol: bytes} of one extracted code object"""
  text = subprocess.check_output([readelf(), '-s', '--wide', path], text=True)
  sizes = {}
  for line in text.splitlines():
    col = line.split()
    if len(col) >= 8 and col[3] == 'FUNC':
      sizes[col[7]] = int(col[2], 0)
  return sizes
