"""The production form of the resident stack against its LAB form, as the compiler built
them into libffn_hip.so: the point of the production form is what it does NOT carry --
fewer scalar registers spilled to lanes between the tap loops, no more scratch, fewer
kernel arguments.  Read from the AMDGPU metadata notes of the library's gfx950 code objects
(llvm-readelf --notes), both kernels from the same build: relative checks, no numbers of a
particular compiler.  No GPU needed.
"""

import os
import re
import struct
import subprocess

import pytest

from ffn_amd import _lib

_MAGIC = b'__CLANG_OFFLOAD_BUNDLE__'


def _readelf():
  for root in (os.environ.get('ROCM_PATH', '/opt/rocm'), '/opt/rocm'):
    path = os.path.join(root, 'llvm', 'bin', 'llvm-readelf')
    if os.path.exists(path):
      return path
  pytest.fail('llvm-readelf of the ROCm tree not found')


def _code_objects(lib_bytes):
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


def _kernel_notes(tmp_path):
  """{kernel symbol: {metadata field: int}} of every kernel in the library"""
  assert os.path.exists(_lib.LIB_PATH), 'build the library first (__graft_entry__.build())'
  with open(_lib.LIB_PATH, 'rb') as f:
    data = f.read()
  kernels = {}
  for k, co in enumerate(_code_objects(data)):
    path = tmp_path / ('co%d.elf' % k)
    path.write_bytes(co)
    text = subprocess.check_output([_readelf(), '--notes', str(path)], text=True)
    # amdhsa.kernels: a list of maps, keys in alphabetical order; a kernel's '.args' list
    # comes first, so the piece behind the last '- .' of a kernel holds its other fields
    for block in re.split(r'\n\s*- \.', text):
      names = re.findall(r'^\s*\.?name:\s+(\S+)', block, re.M)
      if not names or 'kernarg_segment_size' not in block:
        continue
      fields = {}
      for key in ('sgpr_spill_count', 'private_segment_fixed_size', 'kernarg_segment_size',
                  'vgpr_spill_count'):
        m = re.findall(r'\.%s:\s+(\d+)' % key, block)
        if m:
          fields[key] = int(m[-1])
      kernels[names[-1].strip("'\"")] = fields
  return kernels


def test_production_stack_carries_less_than_the_lab_stack(tmp_path):
  kernels = _kernel_notes(tmp_path)
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
