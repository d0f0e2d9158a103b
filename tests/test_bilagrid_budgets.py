"""Registers, scratch and LDS of the bilateral-grid kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_photometric_budgets.py holds the loss kernels.  The budgets are the measured
values rounded up to the next allocation granule (8 VGPRs); LDS is the arithmetic of csrc/bilagrid.hip, exact: the
forward and the image gradient stage up to 4096 coefficients (16 KB float, 32 KB double: nine and five workgroups per
CU by LDS), the grid gradient keeps one (bins x 12) row of doubles per wave.  The grid gradient with groups of 8 bins
holds 96 accumulators per lane (192 registers in double) and runs two waves per SIMD; the other kernels stay at or under
the 128 registers of four."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

# kernel (demangled prefix) : (max VGPRs, LDS bytes).  Measured: forward 71 / 99, image gradient 61 / 132, grid gradient
# 61 / 205 (float, groups of 2 / 8 bins) and 92 / 240 (double), the reduction 10
BUDGETS = {
  'ms::bilagrid_fwd_kernel<float>': (72, 4096 * 4),
  'ms::bilagrid_fwd_kernel<double>': (104, 4096 * 8),
  'ms::bilagrid_image_grad_kernel<float>': (64, 4096 * 4),
  'ms::bilagrid_image_grad_kernel<double>': (136, 4096 * 8),
  'ms::bilagrid_grid_grad_kernel<float, 2>': (64, 4 * 2 * 12 * 8),
  'ms::bilagrid_grid_grad_kernel<float, 8>': (208, 4 * 8 * 12 * 8),
  'ms::bilagrid_grid_grad_kernel<double, 2>': (96, 4 * 2 * 12 * 8),
  'ms::bilagrid_grid_grad_kernel<double, 8>': (240, 4 * 8 * 12 * 8),
  'ms::bilagrid_grid_finalize_kernel<float>': (16, 0),
  'ms::bilagrid_grid_finalize_kernel<double>': (16, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_bilagrid_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'bilagrid.hip').items()}

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
  for name, r in table.items():
    if r.get('scratch', 0) != 0 or r.get('lds', 0) > 65536:
      problems.append(f"{name}: scratch {r.get('scratch', 0)}, LDS {r.get('lds', 0)}")
  assert not problems, problems
