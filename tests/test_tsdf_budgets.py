"""Registers, scratch and LDS of the TSDF kernels (no GPU: the compiler's metadata for gfx950, tools/kernel_resources.py),
as tests/test_geometry_budgets.py holds the geometry kernels.  The budgets are the measured values rounded up to the next
allocation granule (8 VGPRs): integrate 80 (a lane keeps 4 samples' tsdf, weight, colour and positions, 32 values, over
the camera loop: six waves per SIMD, under the issue's target of 128), classify 11, emit 36.  No kernel uses LDS — the
camera rows come through the scalar cache and the cull result through a ballot — and none may spill."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

# kernel (demangled prefix) : (max VGPRs, LDS bytes)
BUDGETS = {
  'ms::tsdf_integrate_kernel': (80, 0),
  'ms::tsdf_classify_kernel': (16, 0),
  'ms::tsdf_emit_kernel': (40, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_tsdf_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'tsdf.hip').items()}

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
