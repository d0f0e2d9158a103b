"""Registers, scratch and instantiation count of the camera-coverage kernel (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_scene_transform_budgets.py holds the scene-transform kernels.

The loop over the cameras is compute bound (a sqrt, a log and a dozen divisions per (gaussian, camera) pair): the float32
instantiation must keep eight waves per SIMD (<= 64 VGPRs) to hide their latency, the float64 one four (<= 128), and
neither may spill.  The file holds the float and the double instantiation of one kernel and nothing else, the count its
header comment states."""
import re
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

PREFIX = 'ms::camera_coverage_kernel<'
VGPR_CAP = {'float': 64, 'double': 128}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_camera_coverage_kernels_keep_their_budgets():
  import kernel_resources as kr
  source = kr.SRC / 'camera_coverage.hip'
  table = {name.replace('void ', ''): r for name, r in kr.resources(source).items()}
  found = {name.split('(')[0]: r for name, r in table.items() if name.startswith(PREFIX)}
  assert set(found) == {f'{PREFIX}{t}>' for t in VGPR_CAP}, sorted(found)
  assert len(table) == len(found), sorted(table)          # the file has no other kernel
  stated = re.search(r'for T in \{float, double\} = (\d+)', source.read_text())
  assert stated and int(stated.group(1)) == len(found)
  problems = []
  for t, cap in VGPR_CAP.items():
    r = found[f'{PREFIX}{t}>']
    print(f"camera_coverage_kernel<{t}>: {r['vgpr']} VGPRs, {r.get('scratch', 0)} bytes of scratch, {r.get('lds', 0)} of LDS")
    if r.get('scratch', 0) != 0:
      problems.append(f"{t}: {r['scratch']} bytes of scratch")
    if r['vgpr'] > cap:
      problems.append(f"{t}: {r['vgpr']} VGPRs > {cap}")
  assert not problems, problems


def test_camera_coverage_source_keeps_contraction_off_and_is_built():
  """the culling comparisons are shared with projection.hip: both files turn FMA contraction off before any code"""
  import kernel_resources as kr
  lines = [l for l in (kr.SRC / 'camera_coverage.hip').read_text().splitlines() if l.strip() and not l.startswith('//')]
  assert lines[0] == '#pragma clang fp contract(off)'
  assert 'camera_coverage.hip' in re.search(r'^SRCS = (.*)$', (kr.SRC / 'Makefile').read_text(), flags=re.M).group(1).split()
