"""Registers, scratch and LDS of the k-nearest-neighbour kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_photometric_budgets.py holds the loss kernels.  VGPR budgets are the measured
values rounded up to the 8-register allocation granule; every one is under 64, so registers never limit the search to
fewer than 8 waves per SIMD, which it needs: its rows arrive by scalar loads whose latency only other waves hide.
Zero scratch is the point of the per-lane list being an unrolled insertion over a template K: a dynamically indexed
list would live in scratch memory.  LDS is exact: the block reduction parks 6 floats (box minimum and maximum) per
wave, 4 waves; the search stages nothing (wave-uniform rows come through the scalar cache)."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

from taichi_splatting_amd import _lib      # noqa: E402

WAVES = _lib.KNN_BLOCK // 64

# kernel (demangled prefix) : (max VGPRs, LDS bytes).  Measured: gather 21; search K = 1..8: 50, 35, 35, 37, 39, 41, 43, 45
BUDGETS = {
  'ms::knn_gather_blocks_kernel': (24, WAVES * 6 * 4),
  'ms::knn_search_kernel<1>': (56, 0),
  'ms::knn_search_kernel<2>': (40, 0),
  'ms::knn_search_kernel<3>': (40, 0),
  'ms::knn_search_kernel<4>': (40, 0),
  'ms::knn_search_kernel<5>': (40, 0),
  'ms::knn_search_kernel<6>': (48, 0),
  'ms::knn_search_kernel<7>': (48, 0),
  'ms::knn_search_kernel<8>': (48, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_knn_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'knn.hip').items()}

  def find(kernel):
    match = [r for name, r in table.items() if name.startswith(kernel + '(')]
    assert len(match) == 1, (kernel, sorted(table))
    return match[0]

  problems = []
  for kernel, (max_vgpr, lds) in BUDGETS.items():
    r = find(kernel)
    if r['vgpr'] > max_vgpr:
      problems.append(f"{kernel}: {r['vgpr']} VGPRs > {max_vgpr}")
    if r.get('lds', 0) != lds:
      problems.append(f"{kernel}: {r.get('lds', 0)} bytes of LDS, expected {lds}")
    if r.get('scratch', 0) != 0:
      problems.append(f"{kernel}: {r['scratch']} bytes of scratch")
  assert len(table) == len(BUDGETS), sorted(table)          # every kernel of the file has a budget
  assert not problems, problems
