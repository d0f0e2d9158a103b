"""Registers and scratch of the active-SH-degree kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_kernel_budgets.py holds the kernels that evaluate every stored band.

Every ``*_active_kernel`` instantiation of csrc/sh.hip and csrc/gaussian_bwd.hip must be free of scratch (a private
segment, even one that only backs scalar-register spill slots, is set up per wave and its reloads wait on vmcnt(0)),
and the float32 ones of the frame path — the SH forward and the per-gaussian backward — must stay at or below 168
VGPRs, the three-waves-per-SIMD step the degree-3 kernels are tuned at.  The count of instantiations is asserted too:
active degree 0..2 per (dtype, variant), the stored row length being a run-time argument, not a template pair."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

VGPR_STEP = 168
# kernel template : instantiations (active degree 0..2 x dtype x variants)
EXPECTED = {
  ('sh.hip', 'ms::sh_fwd_active_kernel<'): 3 * 2,
  ('sh.hip', 'ms::sh_bwd_active_kernel<'): 3 * 2,
  ('sh.hip', 'ms::sh_bwd_params_active_kernel<'): 3 * 2 * 2,          # x UNIQUE
  ('gaussian_bwd.hip', 'ms::gaussian_bwd_active_kernel<'): 3 * (3 + 1),   # float: arrays, moments, fixed-point moments; double
}
FRAME_F32 = ('ms::sh_fwd_active_kernel<float,', 'ms::gaussian_bwd_active_kernel<float,')


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_active_degree_kernels_have_no_scratch_and_keep_three_waves():
  import kernel_resources as kr
  from concurrent.futures import ThreadPoolExecutor
  files = sorted({f for f, _ in EXPECTED})
  with ThreadPoolExecutor(len(files)) as pool:
    tables = dict(zip(files, pool.map(lambda f: kr.resources(kr.SRC / f), files)))
  problems = []
  for (f, prefix), count in EXPECTED.items():
    found = {name.replace('void ', ''): r for name, r in tables[f].items() if name.replace('void ', '').startswith(prefix)}
    assert len(found) == count, (prefix, sorted(found))
    for name, r in found.items():
      kernel = name.split('(')[0]
      if r.get('scratch', 0) != 0:
        problems.append(f"{kernel}: {r['scratch']} bytes of scratch")
      if kernel.startswith(FRAME_F32) and r['vgpr'] > VGPR_STEP:
        problems.append(f"{kernel}: {r['vgpr']} VGPRs > {VGPR_STEP}")
  # nothing named *_active_kernel escapes the list above
  for f in files:
    stray = [n for n in tables[f] if '_active_kernel<' in n and not any(p in n for _, p in EXPECTED)]
    assert not stray, stray
  assert not problems, problems
