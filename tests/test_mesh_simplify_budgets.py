"""Registers, scratch and LDS of the mesh simplification kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_mesh_budgets.py holds the clean-up kernels.  The budgets are the measured values
rounded up to the next allocation granule (8 VGPRs): the placement kernel 70 -> 72 (nine float64 sums of the quadric, the
three of the mean, the nine float64 coordinates of a face and the six cofactors of the solve, all in named scalars), the
key kernel 13 -> 16, the cluster kernel 10 -> 16, the face kernel 14 -> 16, every other kernel 8 or fewer.  No kernel uses
LDS — the 16 partial sums of a cluster meet through DPP — and none may spill: the 3 x 3 system is never indexed."""
import re
import shutil
import sys
from pathlib import Path

import pytest

from taichi_splatting_amd import simplify_mesh              # what these kernels are for

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

# kernel (demangled prefix) : (max VGPRs, LDS bytes)
BUDGETS = {
  'ms::simplify_origin_kernel': (16, 0),
  'ms::simplify_mark_kernel': (8, 0),
  'ms::simplify_keys_kernel': (16, 0),
  'ms::simplify_heads_kernel': (8, 0),
  'ms::simplify_clusters_kernel': (16, 0),
  'ms::simplify_corner_keys_kernel': (8, 0),
  'ms::simplify_place_kernel': (72, 0),
  'ms::simplify_faces_kernel': (16, 0),
  'ms::simplify_pair_keys_kernel': (8, 0),
  'ms::simplify_dedup_kernel': (8, 0),
  'ms::simplify_map_kernel': (8, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_simplify_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'mesh_simplify.hip').items()}

  def find(kernel):
    match = [r for name, r in table.items() if name.startswith(kernel + '(')]
    assert len(match) == 1, (kernel, sorted(table))
    return match[0]

  problems = []
  for kernel, (max_vgpr, max_lds) in BUDGETS.items():
    r = find(kernel)
    if r['vgpr'] > max_vgpr:
      problems.append(f"{kernel}: {r['vgpr']} VGPRs > {max_vgpr}")
    if r.get('lds', 0) > max_lds:
      problems.append(f"{kernel}: {r['lds']} bytes of LDS > {max_lds}")
    if r.get('scratch', 0) != 0:
      problems.append(f"{kernel}: {r['scratch']} bytes of scratch")
  assert len(table) == len(BUDGETS), sorted(table)          # every kernel of the file has a budget
  assert max(b[0] for b in BUDGETS.values()) <= 128         # four waves per SIMD at the least
  assert not problems, problems


def test_the_file_is_built_and_states_its_kernel_count():
  assert callable(simplify_mesh)
  source = Path(__file__).resolve().parent.parent / 'taichi_splatting_amd' / 'csrc'
  assert 'mesh_simplify.hip' in re.search(r'^SRCS = (.*)$', (source / 'Makefile').read_text(), flags=re.M).group(1).split()
  text = (source / 'mesh_simplify.hip').read_text()
  assert int(re.search(r'Kernels of this file = (\d+)', text).group(1)) == len(BUDGETS)
  assert len(re.findall(r'^__global__', text, flags=re.M)) == len(BUDGETS)
  code = [line for line in text.splitlines() if not line.lstrip().startswith('//')]
  assert not any('atomicAdd' in line or '__shared__' in line for line in code)      # no float atomics, no LDS
