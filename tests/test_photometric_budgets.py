"""Registers, scratch and LDS of the photometric-loss kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_kernel_budgets.py holds the frame's kernels.  The budgets are the measured
values rounded up to the next allocation granule (8 VGPRs; LDS is the tile arithmetic of csrc/loss.hip, exact).  They
matter twice here: the kernels' first form, a fully unrolled walk over the staged rows, compiled to 410 registers or,
capped, to a kilobyte of scratch; and the LDS footprint decides the workgroups per CU (forward 5 x 31.6 KB, backward
3 x 47.4 KB of the CU's 160 KB at C = 3)."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

# kernel (demangled prefix) : (max VGPRs, LDS bytes).  Measured: float forward 77 / 81 / 81 / 97, backward 97 / 129 / 129 / 129;
# double forward 140 / 142 / 142 / 142, backward 129 / 129 / 169 / 169; the reduction 18
def _lds(arrays, rows, c, size, extra=0):
  return arrays * rows * (64 + 10 * c) * size + extra


BUDGETS = {
  'ms::photometric_fwd_kernel<float, 1>': (80, _lds(2, 42, 1, 4, 64)),
  'ms::photometric_fwd_kernel<float, 2>': (88, _lds(2, 42, 2, 4, 64)),
  'ms::photometric_fwd_kernel<float, 3>': (88, _lds(2, 42, 3, 4, 64)),
  'ms::photometric_fwd_kernel<float, 4>': (104, _lds(2, 42, 4, 4, 64)),
  'ms::photometric_bwd_kernel<float, 1>': (104, _lds(3, 42, 1, 4)),
  'ms::photometric_bwd_kernel<float, 2>': (136, _lds(3, 42, 2, 4)),
  'ms::photometric_bwd_kernel<float, 3>': (136, _lds(3, 42, 3, 4)),
  'ms::photometric_bwd_kernel<float, 4>': (136, _lds(3, 42, 4, 4)),
  'ms::photometric_finalize_kernel<float>': (24, 4096),
  'ms::photometric_fwd_kernel<double, 1>': (144, _lds(2, 26, 1, 8, 64)),
  'ms::photometric_fwd_kernel<double, 2>': (144, _lds(2, 26, 2, 8, 64)),
  'ms::photometric_fwd_kernel<double, 3>': (144, _lds(2, 26, 3, 8, 64)),
  'ms::photometric_fwd_kernel<double, 4>': (144, _lds(2, 26, 4, 8, 64)),
  'ms::photometric_bwd_kernel<double, 1>': (136, _lds(3, 26, 1, 8)),
  'ms::photometric_bwd_kernel<double, 2>': (136, _lds(3, 26, 2, 8)),
  'ms::photometric_bwd_kernel<double, 3>': (176, _lds(3, 26, 3, 8)),
  'ms::photometric_bwd_kernel<double, 4>': (176, _lds(3, 26, 4, 8)),       # 64 896 bytes: under the 64 KB of a static allocation
  'ms::photometric_finalize_kernel<double>': (24, 4096),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_photometric_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'loss.hip').items()}

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
