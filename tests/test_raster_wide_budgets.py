"""Registers, scratch and LDS of the wide-feature raster kernels (no GPU: the compiler's metadata for gfx950,
tools/kernel_resources.py), as tests/test_kmeans_budgets.py holds the k-means kernels.  The register figure is the unified
file (architectural + accumulator registers: the MFMA accumulators and the backward's register-resident dL/dimage
operands may live in either half), at most 512 for a 256-thread workgroup; budgets are the measured values rounded up to
the 8-register allocation granule.  Zero scratch is the point of NB being a template parameter: the accumulator tiles,
the operand registers and the 32 unrolled chain steps are indexed by constants only.  LDS is exact and at most 160 KB:

  records      64 splats x (48-byte blend record + 32-byte cull record)
  forward      + 64 feature rows of FP + 1 floats (FP = 32 NB)
  backward     + 64 ids + 4 waves x 64 hit slots + the word of the tile-wide saturation vote
               + 64 feature rows of FP + 1 floats          with grad_points7   (else a 4-byte stand-in)
               + 4 waves x 64 pixels x 33 weights           with grad_features  (else a 4-byte stand-in)
               + 64 x FP floats of the batch's feature gradient  with grad_features  (else a 4-byte stand-in)
  rounded up to the 256-byte granule the metadata is written in."""
import shutil
import sys
from pathlib import Path

import pytest

sys.path.insert(0, str(Path(__file__).resolve().parent.parent / 'tools'))

BATCH = 64
RECORDS = BATCH * (48 + 32)
LDS_LIMIT = 160 * 1024


def granule(nbytes):
  return (nbytes + 255) // 256 * 256


def fwd_lds(nb):
  return granule(RECORDS + BATCH * (32 * nb + 1) * 4)


def bwd_lds(nb, gp, gf):
  fp = 32 * nb
  return granule(RECORDS + BATCH * 4 + 4 * 64 * 4 + 4
                 + (BATCH * (fp + 1) * 4 if gp else 4)
                 + (4 * 64 * 33 * 4 if gf else 4)
                 + (BATCH * fp * 4 if gf else 4))


# kernel (demangled prefix) : (max unified VGPRs, LDS bytes).  Measured: forward NB = 1..4: 86, 110, 139, 174; backward
# (both gradients / grad_points7 only / grad_features only): NB = 1: 197 / 110 / 142, NB = 2: 202 / 142 / 172,
# NB = 3: 280 / 172 / 177, NB = 4: 314 / 207 / 181.  All but the two widest both-gradient kernels (one workgroup per CU by
# their LDS anyway) stay at or under 256: two waves per SIMD
BUDGETS = {
  'ms::raster_wide_fwd_kernel<1>': (88, fwd_lds(1)),
  'ms::raster_wide_fwd_kernel<2>': (112, fwd_lds(2)),
  'ms::raster_wide_fwd_kernel<3>': (144, fwd_lds(3)),
  'ms::raster_wide_fwd_kernel<4>': (176, fwd_lds(4)),
  'ms::raster_wide_bwd_kernel<1, true, true>': (200, bwd_lds(1, True, True)),
  'ms::raster_wide_bwd_kernel<1, true, false>': (112, bwd_lds(1, True, False)),
  'ms::raster_wide_bwd_kernel<1, false, true>': (144, bwd_lds(1, False, True)),
  'ms::raster_wide_bwd_kernel<2, true, true>': (208, bwd_lds(2, True, True)),
  'ms::raster_wide_bwd_kernel<2, true, false>': (144, bwd_lds(2, True, False)),
  'ms::raster_wide_bwd_kernel<2, false, true>': (176, bwd_lds(2, False, True)),
  'ms::raster_wide_bwd_kernel<3, true, true>': (280, bwd_lds(3, True, True)),
  'ms::raster_wide_bwd_kernel<3, true, false>': (176, bwd_lds(3, True, False)),
  'ms::raster_wide_bwd_kernel<3, false, true>': (184, bwd_lds(3, False, True)),
  'ms::raster_wide_bwd_kernel<4, true, true>': (320, bwd_lds(4, True, True)),
  'ms::raster_wide_bwd_kernel<4, true, false>': (208, bwd_lds(4, True, False)),
  'ms::raster_wide_bwd_kernel<4, false, true>': (184, bwd_lds(4, False, True)),
}


@pytest.mark.skipif(shutil.which('hipcc') is None and not Path('/opt/rocm/bin/hipcc').exists(), reason="no hipcc")
def test_wide_raster_kernels_stay_inside_their_budgets():
  import kernel_resources as kr
  table = {name.replace('void ', ''): r for name, r in kr.resources(kr.SRC / 'raster_wide.hip').items()}

  def find(kernel):
    match = [r for name, r in table.items() if name.startswith(kernel + '(')]
    assert len(match) == 1, (kernel, sorted(table))
    return match[0]

  problems = []
  for kernel, (max_vgpr, lds) in BUDGETS.items():
    r = find(kernel)
    assert max_vgpr % 8 == 0 and max_vgpr <= 512 and lds <= LDS_LIMIT, kernel
    if r['vgpr'] > max_vgpr:
      problems.append(f"{kernel}: {r['vgpr']} VGPRs > {max_vgpr}")
    if r.get('lds', 0) != lds:
      problems.append(f"{kernel}: {r.get('lds', 0)} bytes of LDS, expected {lds}")
    if r.get('scratch', 0) != 0:
      problems.append(f"{kernel}: {r['scratch']} bytes of scratch")
  assert len(table) == len(BUDGETS), sorted(table)          # every kernel of the file has a budget
  assert not problems, problems
