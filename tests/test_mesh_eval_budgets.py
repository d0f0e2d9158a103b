"""Registers, scratch and LDS of the cross-set nearest-neighbour kernels (csrc/knn_query.hip) and of the surface sampler
(csrc/mesh_sample.hip) — no GPU: the compiler's metadata for gfx950, tools/kernel_resources.py, as
tests/test_knn_budgets.py holds the self search.  VGPR budgets are the measured values rounded up to the 8-register
allocation granule, with the measurement beside each; every search kernel is under 64, so registers never limit it to
fewer than 8 waves per SIMD, which it needs: its rows arrive by scalar loads whose latency only other waves hide.  Zero
scratch everywhere: the per-lane list is an unrolled insertion over a template K.  LDS is exact: the gather's box
reduction parks 6 floats per wave, 4 waves; the search and the sampler stage nothing."""
import re
import shutil
import sys
from pathlib import Path

import pytest

from taichi_splatting_amd import _lib, knn_query, sample_mesh_points      # what these kernels are for

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

WAVES = _lib.KNN_BLOCK // 64
SOURCE = Path(__file__).resolve().parent.parent / 'taichi_splatting_amd' / 'csrc'

# file : kernel (demangled prefix) : (max VGPRs, LDS bytes).
# Measured: gather 21; search K = 1..8: 33, 37, 37, 39, 39, 41, 43, 47; face areas 20; sampler 42
BUDGETS = {
  'knn_query.hip': {
    'ms::knn_query_gather_kernel': (24, WAVES * 6 * 4),
    'ms::knn_query_search_kernel<1>': (40, 0),
    'ms::knn_query_search_kernel<2>': (40, 0),
    'ms::knn_query_search_kernel<3>': (40, 0),
    'ms::knn_query_search_kernel<4>': (40, 0),
    'ms::knn_query_search_kernel<5>': (40, 0),
    'ms::knn_query_search_kernel<6>': (48, 0),
    'ms::knn_query_search_kernel<7>': (48, 0),
    'ms::knn_query_search_kernel<8>': (48, 0),
  },
  'mesh_sample.hip': {
    'ms::mesh_face_areas_kernel': (24, 0),
    'ms::mesh_sample_points_kernel': (48, 0),
  },
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
@pytest.mark.parametrize('file', sorted(BUDGETS))
def test_kernels_stay_inside_their_budgets(file):
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / file).items()}

  def find(kernel):
    match = [r for name, r in table.items() if name.startswith(kernel + '(')]
    assert len(match) == 1, (kernel, sorted(table))
    return match[0]

  problems = []
  for kernel, (max_vgpr, lds) in BUDGETS[file].items():
    r = find(kernel)
    if r['vgpr'] > max_vgpr:
      problems.append(f"{kernel}: {r['vgpr']} VGPRs > {max_vgpr}")
    if r.get('lds', 0) != lds:
      problems.append(f"{kernel}: {r.get('lds', 0)} bytes of LDS, expected {lds}")
    if r.get('scratch', 0) != 0:
      problems.append(f"{kernel}: {r['scratch']} bytes of scratch")
  assert len(table) == len(BUDGETS[file]), sorted(table)          # every kernel of the file has a budget
  assert not problems, problems


def test_the_search_keeps_eight_waves_per_simd():
  assert all(vgpr < 64 for kernel, (vgpr, _) in BUDGETS['knn_query.hip'].items() if 'search' in kernel)
  assert all(vgpr % 8 == 0 for kernels in BUDGETS.values() for vgpr, _ in kernels.values())


def test_the_files_are_built():
  assert callable(knn_query) and callable(sample_mesh_points)
  srcs = re.search(r'^SRCS = (.*)$', (SOURCE / 'Makefile').read_text(), flags=re.M).group(1).split()
  assert 'knn_query.hip' in srcs and 'mesh_sample.hip' in srcs
  for name in ('ms_knn_query', 'ms_mesh_face_areas', 'ms_mesh_sample_points'):
    assert name in _lib.SIGNATURES and hasattr(_lib.load(), name)
  for file, kernels in BUDGETS.items():
    text = (SOURCE / file).read_text()
    assert len(re.findall(r'^__global__', text, flags=re.M)) == len({k.split('<')[0] for k in kernels}), file
    code = [line for line in text.splitlines() if not line.lstrip().startswith('//')]
    assert not any('__shared__' in line for line in code) or file == 'knn_query.hip'      # only the gather's box reduction
  sampler = [line for line in (SOURCE / 'mesh_sample.hip').read_text().splitlines() if not line.lstrip().startswith('//')]
  assert not any('atomicAdd' in line for line in sampler)                  # no atomics on data: the status word is an OR
