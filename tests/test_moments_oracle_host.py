"""CPU: tests/moments_oracle.py against the oracle the suite already trusts, and the two conditions on the fixed-point
units of the deterministic raster backward that need no GPU.

* The moment rows of scene A (tests/threshold_cases.py), pushed through the float64 transcription of
  raster_moments_finalize_kernel, reproduce ``oracle.raster.backward``'s gradients and heuristics and ``forward``'s
  visibility (column 11 plus the weight of the pairs behind a pixel's saturation point, which the backward drops and the
  forward keeps adding) to 1e-9 of the largest entry of each.
* Precision floor: on scene A, with a randn dL/dimage and with the constant one of a mean-reduced loss, quantisation of
  the commits takes at most 1 % of the 1e-4 contract in every column 0..10: max_i P[i] u_c / 2 <= 1e-6 max_i |M[i, c]|,
  for the units of ms_fixed_point_exponents and for those of ms_fixed_point_exponents_ranged (figures in
  tests/test_gpu_fixed_point.py's docstring).
* The headroom cases of tests/test_gpu_fixed_point.py exceed 2^63 units of ms_fixed_point_exponents in the column they
  are aimed at and stay below 2^62 units of ms_fixed_point_exponents_ranged in every column; so does the control under
  both."""
import functools
import math

import pytest
import torch

from oracle import raster as orast
from taichi_splatting_amd import RasterConfig
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d

from . import moments_oracle as mo
from . import threshold_cases as tc


@functools.lru_cache(maxsize=None)
def scene_a_rows(name, g_kind):
  """scene A at config ``name`` ('default' or a key of threshold_cases.CONFIGS), tile 16, heuristics and visibility on"""
  kw = dict(compute_point_heuristic=True, compute_visibility=True)
  cfg = RasterConfig(tile_size=16, **kw) if name == 'default' else tc.config(name, 16, **kw)
  g = tc.scene_a(name)
  p, f = project_gaussians2d(g).double(), g.feature.double()
  o2p, ranges = tc.oracle_lists(g, tc.SIZE_A, cfg)
  w, h = tc.SIZE_A
  G = tc.grad_image(tc.SIZE_A, 3) if g_kind == 'randn' else torch.full((h, w, 3), 1.0 / (h * w * 3), dtype=torch.float64)
  image, _, vis = orast.forward(p, f, ranges, o2p, tc.SIZE_A, cfg)
  want = orast.backward(p, f, ranges, o2p, image, G, tc.SIZE_A, cfg)
  rows = mo.moment_rows(p, f, ranges, o2p, image, G, tc.SIZE_A, cfg)
  return cfg, p, f, G, vis, want, rows


@pytest.mark.parametrize('name', ['default', 'ALL'])
def test_moment_rows_finalized_reproduce_the_oracle_backward(name):
  cfg, p, f, G, vis, (gp, gf, heur), (M, A, P, dropped) = scene_a_rows(name, 'randn')
  got_gp, got_gf, got_heur, got_vis = mo.finalize(p, M)
  for what, got, want in (('grad_points', got_gp, gp), ('grad_features', got_gf, gf), ('heuristics', got_heur, heur),
                          ('visibility', got_vis + dropped, vis)):
    scale = float(want.abs().max())
    err = float((got - want).abs().max())
    print(f"{name} {what}: {err / scale:.3e} of the largest entry")
    assert scale > 0 and err <= 1e-9 * scale, (name, what, err / scale)
  assert bool((A >= M.abs()).all()) and int(P.max()) > 1 and bool((P[M.abs().sum(1) > 0] > 0).all())
  if name == 'ALL':
    assert float(dropped.max()) > 0          # (saturate_threshold 0.8: the forward's visibility really holds more)


@pytest.mark.parametrize('g_kind', ['randn', 'mean'])
def test_quantisation_takes_at_most_one_percent_of_the_contract(g_kind):
  cfg, p, f, G, _, _, (M, A, P, _) = scene_a_rows('default', g_kind)
  amax, fmax, smin = mo.launch_stats(p, f, G)
  pixels = tc.SIZE_A[0] * tc.SIZE_A[1]
  for form, exps in (('amax only', mo.exponents(amax)), ('ranged', mo.exponents_ranged(amax, fmax, smin, pixels, cfg.alpha_threshold))):
    u = mo.column_units(*exps)
    ratio = float(P.max()) * u[:11] / 2 / M[:, :11].abs().max(dim=0).values
    print(f"{g_kind} dL/dimage, {form}: exponents {exps}, P max {int(P.max())}, quantisation / largest sum per column:",
          [f"{float(r):.1e}" for r in ratio])
    assert bool((ratio <= 1e-6).all()), (g_kind, form, ratio)


@functools.lru_cache(maxsize=None)
def headroom_rows(case):
  colour, alpha, g, column = mo.HEADROOM_CASES[case]
  cfg = RasterConfig(tile_size=16, compute_point_heuristic=True)
  p, f, depth = mo.headroom_scene(colour, alpha)
  o2p, ranges = mo.oracle_lists(p, depth, mo.HEADROOM_SIZE, cfg)
  w, h = mo.HEADROOM_SIZE
  G = torch.full((h, w, 3), g, dtype=torch.float64)
  image, _, _ = orast.forward(p.double(), f.double(), ranges, o2p, mo.HEADROOM_SIZE, cfg)
  M, A, P, _ = mo.moment_rows(p, f, ranges, o2p, image, G, mo.HEADROOM_SIZE, cfg)
  return cfg, p, f, G, M, A, P


@pytest.mark.parametrize('case', list(mo.HEADROOM_CASES))
def test_headroom_cases_leave_the_range_of_the_amax_only_units_and_stay_inside_the_ranged_ones(case):
  column = mo.HEADROOM_CASES[case][3]
  cfg, p, f, G, M, A, P = headroom_rows(case)
  amax, fmax, smin = mo.launch_stats(p, f, G)
  old = M.abs() / mo.column_units(*mo.exponents(amax))
  new = A / mo.column_units(*mo.exponents_ranged(amax, fmax, smin, mo.HEADROOM_SIZE[0] * mo.HEADROOM_SIZE[1], cfg.alpha_threshold))
  print(f"{case}: log2 units per column, amax-only form:", [round(math.log2(float(v)), 1) for v in old.max(dim=0).values],
        "ranged form (absolute sums):", [round(math.log2(float(v)), 1) for v in new.max(dim=0).values])
  if column is None:
    assert float(old.max()) < 2.0 ** 62
  else:
    assert float(old[:, column].max()) > 2.0 ** 63, (case, column, math.log2(float(old[:, column].max())))
  assert float(new.max()) < 2.0 ** 62
