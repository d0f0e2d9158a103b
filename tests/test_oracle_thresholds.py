"""The oracle itself at the blend thresholds tests/test_gpu_thresholds.py leans on (tests/threshold_cases.py): the
vectorised oracle.raster against the independent scalar loops of oracle.raster_scalar at configs ALL and S_half, and, on
scene A, the two conditions every GPU case starts from — the config changes the oracle's result on at least 10 % of rows,
and at most 2 % of rows have a pair on the backward's saturation limit."""
import functools

import pytest
import torch

from oracle import mapper as omap, raster as orast, raster_scalar as osc
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
from taichi_splatting_amd.testing import random_2d_gaussians

from . import threshold_cases as tc


@pytest.mark.parametrize('name', ['ALL', 'S_half'])
def test_vectorised_oracle_agrees_with_scalar_loops(name):
  size, tile = (40, 24), 8
  cfg = tc.config(name, tile, compute_point_heuristic=True)
  torch.manual_seed(7)
  g = random_2d_gaussians(120, size, scale_factor=1.5, alpha_range=tc.alpha_range(name))
  p, f = project_gaussians2d(g).double(), g.feature.double()
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), g.depths.numpy(), size, tile, cfg.alpha_threshold)
  o2p_t, ranges_t = torch.from_numpy(o2p), torch.from_numpy(ranges)
  image, alpha, vis = orast.forward(p, f, ranges_t, o2p_t, size, cfg)
  G = tc.grad_image(size, 3)
  gp, gf, heur = orast.backward(p, f, ranges_t, o2p_t, image, G, size, cfg)
  # the thresholds are at work on this small scene as well
  d = tc.default_of(cfg)
  o2p_d, ranges_d = tc.oracle_lists(g, size, d)
  default = tc.oracle_outputs(p, f, ranges_d, o2p_d, size, d, G)
  assert tc.differing_rows(gp, default['grad_points']) > 0.1
  if name == 'ALL':
    assert float(alpha.max()) > 0.8 and tc.differing_rows(image, default['image']) > 0.1

  kw = dict(tile_size=tile, clamp_max_alpha=cfg.clamp_max_alpha, alpha_threshold=cfg.alpha_threshold)
  rl = [tuple(int(v) for v in r) for r in ranges.reshape(-1, 2)]
  image_s, alpha_s, vis_s = osc.forward(p.tolist(), f.tolist(), rl, o2p.tolist(), size, **kw)
  gp_s, gf_s, heur_s = osc.backward(p.tolist(), f.tolist(), rl, o2p.tolist(), image.tolist(), G.tolist(), size,
                                    saturate_threshold=cfg.saturate_threshold, **kw)
  for what, got, want in (('image', image_s, image), ('alpha', alpha_s, alpha), ('visibility', vis_s, vis),
                          ('d gaussians2d', gp_s, gp), ('d features', gf_s, gf), ('heuristics', heur_s, heur)):
    err = float((torch.tensor(got, dtype=torch.float64) - want).abs().max())
    assert err <= 1e-12 * max(1.0, float(want.abs().max())), (what, err)


@functools.lru_cache(maxsize=None)
def _scene_a_outputs(name, default):
  g = tc.scene_a(name)
  p, f = project_gaussians2d(g).double(), g.feature.double()
  cfg = tc.config(name)
  cfg = tc.default_of(cfg) if default else cfg
  o2p, ranges = tc.oracle_lists(g, tc.SIZE_A, cfg)
  return p, ranges, o2p, cfg, tc.oracle_outputs(p, f, ranges, o2p, tc.SIZE_A, cfg, tc.grad_image(tc.SIZE_A, 3))


@pytest.mark.parametrize('name', list(tc.CONFIGS))
def test_scene_a_is_sensitive_to_the_config(name):
  p, ranges, o2p, cfg, case = _scene_a_outputs(name, False)
  # (the default-config runs are shared by the configs with the same alpha range)
  shared = 'ALL' if tc.alpha_range(name) == tc.alpha_range('ALL') else 'T_hi'
  tc.assert_sensitive(name, case, _scene_a_outputs(shared, True)[4])
  if 'saturate_threshold' in tc.CONFIGS[name]:
    flagged = tc.flagged_rows(p, ranges, o2p, tc.SIZE_A, cfg)
    assert int(flagged.sum()) > 0                  # and the rule for them is exercised
