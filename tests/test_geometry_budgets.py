"""Registers, scratch and LDS of the geometry kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_bilagrid_budgets.py holds the bilateral-grid kernels.  The budgets are the
measured values rounded up to the next allocation granule (8 VGPRs); LDS is the arithmetic of csrc/geometry.hip, exact
(each array rounded up to 16 bytes): the consistency forward stages depth (T) and the alpha test (one byte) of a
64 x 16 tile + 1 and keeps one double per wave; its backward stages the same of tile + 2 and three values of T for each
centre of tile + 1 (21 KB float: seven workgroups per CU by LDS; 40 KB double: three).  The per-gaussian kernels use no
LDS.  Every kernel stays under the 128 registers of four waves per SIMD."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

TW, TH = 64, 16                     # NC_TW, NC_TH


def up16(n):
  return (n + 15) // 16 * 16


def fwd_lds(size):
  cells = (TH + 2) * (TW + 2)
  return up16(cells * size) + up16(cells) + 4 * 8


def bwd_lds(size):
  return up16((TH + 4) * (TW + 4) * size) + up16((TH + 4) * (TW + 4)) + 3 * (TH + 2) * (TW + 2) * size


# kernel (demangled prefix) : (max VGPRs, LDS bytes).  Measured: normals forward 30 / 48 (float / double), backward
# 31 / 52; consistency forward 34 / 48, backward 65 / 97, the reduction 10
BUDGETS = {
  'ms::gaussian_normals_fwd_kernel<float>': (32, 0),
  'ms::gaussian_normals_fwd_kernel<double>': (48, 0),
  'ms::gaussian_normals_bwd_kernel<float>': (32, 0),
  'ms::gaussian_normals_bwd_kernel<double>': (56, 0),
  'ms::normal_consistency_fwd_kernel<float>': (40, fwd_lds(4)),
  'ms::normal_consistency_fwd_kernel<double>': (48, fwd_lds(8)),
  'ms::normal_consistency_finalize_kernel<float>': (16, 256 * 8),
  'ms::normal_consistency_finalize_kernel<double>': (16, 256 * 8),
  'ms::normal_consistency_bwd_kernel<float>': (72, bwd_lds(4)),
  'ms::normal_consistency_bwd_kernel<double>': (104, bwd_lds(8)),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_geometry_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'geometry.hip').items()}

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
