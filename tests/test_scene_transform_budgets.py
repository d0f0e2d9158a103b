"""Scratch and instantiation count of the scene-transform kernel (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_sh_active_budgets.py holds the active-degree kernels.

The transform travels in the kernel arguments and a degree-3 vector is 16 registers per lane: every instantiation must
be free of scratch.  Their count is the one the header comment of csrc/scene_transform.hip states: dtype (float,
double) x degree (0 = no feature, 1, 2, 3) = 8; the float32 ones must also keep the eight waves per SIMD (<= 64 VGPRs)
that hide the latency of a kernel with three barriers per chunk."""
import re
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

PREFIX = 'ms::scene_transform_kernel<'
ROWS = 256          # MS_SCENE_XFORM_ROWS: the LDS image is one vector per lane


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_scene_transform_kernels_have_no_scratch():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'scene_transform.hip').items()}
  found = {name.split('(')[0]: r for name, r in table.items() if name.startswith(PREFIX)}
  want = {f'{PREFIX}{t}, {d}>' for t in ('float', 'double') for d in range(4)}
  assert set(found) == want, sorted(found)
  assert len(table) == len(found), sorted(table)          # the file has no other kernel
  stated = re.search(r'x DEG in \{0, 1, 2, 3\} = (\d+)', (kr.SRC / 'scene_transform.hip').read_text())
  assert stated and int(stated.group(1)) == len(found)
  problems = []
  for name, r in found.items():
    size, degree = (4 if '<float' in name else 8), int(name[-2])
    if r.get('scratch', 0) != 0:
      problems.append(f"{name}: {r['scratch']} bytes of scratch")
    lds = ROWS * (degree + 1) ** 2 * size if degree else 0
    if r.get('lds', 0) != lds:
      problems.append(f"{name}: {r.get('lds', 0)} bytes of LDS, {lds} expected")
    if size == 4 and r['vgpr'] > 64:
      problems.append(f"{name}: {r['vgpr']} VGPRs > 64")
  assert not problems, problems
