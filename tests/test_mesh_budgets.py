"""Registers, scratch and LDS of the mesh clean-up kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_tsdf_budgets.py holds the TSDF kernels.  The budgets are the measured values
rounded up to the next allocation granule (8 VGPRs): the hook kernel 16 (two path walks and a compare-and-swap), the
gather 16, the count kernel 10 -> 16, the normals kernel 34 -> 40 (three float64 sums and the nine float64 coordinates of a face), every other kernel
10 or fewer.  No kernel uses LDS — equal labels are combined by ballot, not through shared memory — and none may spill."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

# kernel (demangled prefix) : (max VGPRs, LDS bytes)
BUDGETS = {
  'ms::mesh_init_kernel': (8, 0),
  'ms::mesh_hook_kernel': (16, 0),
  'ms::mesh_flatten_kernel': (8, 0),
  'ms::mesh_label_kernel': (8, 0),
  'ms::mesh_count_kernel': (16, 0),
  'ms::mesh_filter_keys_kernel': (16, 0),
  'ms::mesh_filter_take_kernel': (8, 0),
  'ms::mesh_filter_mask_kernel': (8, 0),
  'ms::mesh_mark_kernel': (8, 0),
  'ms::mesh_head_kernel': (8, 0),
  'ms::mesh_gather_kernel': (16, 0),
  'ms::mesh_corner_keys_kernel': (8, 0),
  'ms::mesh_normals_kernel': (40, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_mesh_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'mesh.hip').items()}

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
