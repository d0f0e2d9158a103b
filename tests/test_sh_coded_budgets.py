"""Registers, scratch and LDS of the coded SH kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_kmeans_budgets.py holds the k-means kernels.  Budgets are the measured VGPRs
rounded up to the 8-register allocation granule; every kernel stays far below 128, so occupancy is never the limit of
these memory-bound passes.  Zero scratch: the basis and a code row are arrays indexed by unrolled constants only.  LDS is
exact: a tile of 256 entries of M basis values at the odd row stride M | 1 and 3 masked gradients, in float32, and four
waves of 3 M float64 sums."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))


def partial_lds(degree):
  m = (degree + 1) ** 2 - 1
  return 256 * (m | 1) * 4 + 256 * 3 * 4 + 4 * 3 * m * 8


# kernel (demangled prefix) : (max VGPRs, LDS bytes).  Measured: forward degree 1 / 2 / 3: 33, 49, 61;
# prep 9 (with records: 24); partial degree 1 / 2 / 3: 18, 24, 36; finish 12
BUDGETS = {
  'ms::sh_coded_fwd_kernel<1>': (40, 0),
  'ms::sh_coded_fwd_kernel<2>': (56, 0),
  'ms::sh_coded_fwd_kernel<3>': (64, 0),
  'ms::sh_coded_prep_kernel<false>': (16, 0),
  'ms::sh_coded_prep_kernel<true>': (24, 0),
  'ms::sh_coded_partial_kernel<1>': (24, partial_lds(1)),
  'ms::sh_coded_partial_kernel<2>': (24, partial_lds(2)),
  'ms::sh_coded_partial_kernel<3>': (40, partial_lds(3)),
  'ms::sh_coded_finish_kernel': (16, 0),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_sh_coded_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'sh_coded.hip').items()}

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
