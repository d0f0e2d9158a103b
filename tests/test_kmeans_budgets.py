"""Registers, scratch and LDS of the k-means kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_knn_budgets.py holds the neighbour search.  The register figure is the
unified file (architectural + accumulator registers: the MFMA accumulators may live in either half); budgets are the
measured values rounded up to the 8-register allocation granule.  Every assignment kernel stays at or under 256, so two
workgroups share a CU and one stages its next chunk of codes while the other multiplies.  Zero scratch is the point of
DP being a template parameter: the A fragments, the running minima and their tiles are arrays indexed by unrolled
constants only.  LDS is exact: MS_KMEANS_CHUNK codes of DP floats and their norms for the assignment, four waves of
64 + 1 doubles for a chunk sum of the update, one int per thread for the chunk scan."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

from taichi_splatting_amd import _lib      # noqa: E402

CHUNK = _lib.KMEANS_CHUNK


def assign_lds(dp):
  return CHUNK * dp * 4 + CHUNK * 4


# kernel (demangled prefix) : (max VGPRs, LDS bytes).  Measured: assign DP = 8..64: 152, 160, 156, 164, 188, 196, 208, 216;
# codes 16, pairs 6, ranges 12, chunk scan 17, partial 20, finish 14
BUDGETS = {
  'ms::kmeans_codes_kernel': (16, 0),
  'ms::kmeans_assign_kernel<8>': (152, assign_lds(8)),
  'ms::kmeans_assign_kernel<16>': (160, assign_lds(16)),
  'ms::kmeans_assign_kernel<24>': (160, assign_lds(24)),
  'ms::kmeans_assign_kernel<32>': (168, assign_lds(32)),
  'ms::kmeans_assign_kernel<40>': (192, assign_lds(40)),
  'ms::kmeans_assign_kernel<48>': (200, assign_lds(48)),
  'ms::kmeans_assign_kernel<56>': (208, assign_lds(56)),
  'ms::kmeans_assign_kernel<64>': (216, assign_lds(64)),
  'ms::kmeans_pairs_kernel': (8, 0),
  'ms::kmeans_ranges_kernel': (16, 0),
  'ms::kmeans_chunk_scan_kernel': (24, 1024 * 4),
  'ms::kmeans_partial_kernel': (24, 4 * (_lib.KMEANS_MAX_D + 1) * 8),
  'ms::kmeans_finish_kernel': (16, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_kmeans_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'kmeans.hip').items()}

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
    if kernel.startswith('ms::kmeans_assign_kernel') and r['vgpr'] > 256:
      problems.append(f"{kernel}: {r['vgpr']} VGPRs leave one wave per SIMD")
  assert len(table) == len(BUDGETS), sorted(table)          # every kernel of the file has a budget
  assert not problems, problems
