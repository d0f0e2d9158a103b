"""Registers, scratch and LDS of the fixed-budget densification kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_knn_budgets.py holds the k-nearest-neighbour kernels.  VGPR budgets are the
measured values rounded up to the 8-register allocation granule, and each must leave the waves per SIMD (512 registers
per lane) that DESIGN.md claims for the kernel: 8 for the four that are nothing but loads, a little arithmetic and
stores and need the waves to keep HBM busy, 6 for the opacity correction, which is double-precision pow / exp / log on
the drawn rows only.  Zero scratch: the double sum of the opacity correction runs over a table in memory and two running
values, never over a per-lane array.  LDS is exact: the move parks one table word and one row byte per touched row of its block (256 x 5 bytes, + 4 counts),
the position noise stages three (256, 3) float32 arrays (3 x 3072 bytes), draw and fresh park one count per wave."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

# kernel (demangled prefix) : (max VGPRs, LDS bytes, waves per SIMD).  Measured: weights 14, draw 22, fresh 76, move 30,
# perturb 50
BUDGETS = {
  'ms::relocate_weights_kernel': (16, 0, 8),
  'ms::relocate_draw_kernel': (24, 4 * 4, 8),
  'ms::relocate_fresh_kernel': (80, 4 * 4, 6),
  'ms::relocate_move_kernel': (32, 256 * 4 + 256 + 4 * 4, 8),
  'ms::perturb_positions_kernel': (56, 3 * 256 * 3 * 4, 8),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_relocate_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'relocate.hip').items()}

  def find(kernel):
    match = [r for name, r in table.items() if name.startswith(kernel + '(')]
    assert len(match) == 1, (kernel, sorted(table))
    return match[0]

  problems = []
  for kernel, (max_vgpr, lds, waves) in BUDGETS.items():
    r = find(kernel)
    assert 512 // max_vgpr >= waves, (kernel, max_vgpr, waves)
    if r['vgpr'] > max_vgpr:
      problems.append(f"{kernel}: {r['vgpr']} VGPRs > {max_vgpr}")
    if r.get('lds', 0) != lds:
      problems.append(f"{kernel}: {r.get('lds', 0)} bytes of LDS, expected {lds}")
    if r.get('scratch', 0) != 0:
      problems.append(f"{kernel}: {r['scratch']} bytes of scratch")
  assert len(table) == len(BUDGETS), sorted(table)          # every kernel of the file has a budget
  assert not problems, problems
