"""Shared by tests/test_oracle_thresholds.py (CPU) and tests/test_gpu_thresholds.py: the non-default blend thresholds the
suite runs at, scene A, and the two oracle-only conditions every case is held to before a kernel is looked at:

* ``assert_sensitive``: the oracle at the case's config and at the default config, on the same scene, differ by more
  than 1e-3 of the largest entry on at least 10 % of rows — the parameter reaches the output the case compares;
* ``saturation_rows``: which gradient rows have a (pixel, splat) pair within 1e-4 (relative) of the backward's
  saturation limit ``1 - saturate_threshold`` (oracle.raster.saturation_margin).  Such a pair may fall on either side of
  the limit in float32; a flipped pair changes only its own splat's row (the pairs behind it are inactive anyway, those
  in front do not see it).  Those rows — at most 2 % of all rows, a condition — are held to the interval between the
  oracle backward at limit (1 - 1e-4) and at limit (1 + 1e-4); every other row to the full tolerance."""
from dataclasses import replace

import numpy as np
import torch

from oracle import mapper as omap, raster as orast
from taichi_splatting_amd import RasterConfig
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
from taichi_splatting_amd.testing import random_2d_gaussians

CONFIGS = {
  'T_hi': dict(alpha_threshold=0.05),
  'T_lo': dict(alpha_threshold=1e-4),
  'C_half': dict(clamp_max_alpha=0.5),
  'C_80': dict(clamp_max_alpha=0.8),
  'S_half': dict(saturate_threshold=0.5),
  'S_90': dict(saturate_threshold=0.9),
  'ALL': dict(alpha_threshold=0.02, clamp_max_alpha=0.7, saturate_threshold=0.8),
}
SIZE_A = (150, 100)          # not a multiple of any tile size
SENSITIVE_ROWS = 0.10
FLAGGED_ROWS = 0.02
SATURATION_MARGIN = 1e-4


def config(name, tile=16, **kw):
  return RasterConfig(tile_size=tile, pixel_stride=(1, 1) if tile == 8 else (2, 2), **CONFIGS[name], **kw)


def default_of(cfg):
  """``cfg`` with the three blend thresholds back at their defaults"""
  d = RasterConfig()
  return replace(cfg, alpha_threshold=d.alpha_threshold, clamp_max_alpha=d.clamp_max_alpha, saturate_threshold=d.saturate_threshold)


def alpha_range(name):
  """(0.3, 1.0) where the clamp is to engage, the suite's usual range elsewhere"""
  return (0.3, 1.0) if name.startswith('C_') or name == 'ALL' else (0.1, 0.9)


def scene_a(name, channels=3, seed=0):
  torch.manual_seed(seed)
  return random_2d_gaussians(3000, SIZE_A, num_channels=channels, scale_factor=1.5, alpha_range=alpha_range(name))


def oracle_lists(g, size, cfg):
  p = project_gaussians2d(g)
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), g.depths.numpy(), size, cfg.tile_size, cfg.alpha_threshold)
  return torch.from_numpy(o2p), torch.from_numpy(ranges).reshape(-1, 2)


def grad_image(size, channels, seed=0):
  """dL/dimage of both signs, as in test_forward_backward_f64 (a positive one hides the clamp: the gradients of the few
  splats it reaches then drown in the largest row)"""
  torch.manual_seed(seed)
  return torch.randn(size[1], size[0], channels, dtype=torch.float64)


def oracle_outputs(p, f, ranges, o2p, size, cfg, G):
  """dict of the float64 oracle's image, alpha, visibility, d gaussians2d, d features, heuristics"""
  p, f = p.cpu().double(), f.cpu().double()
  ranges, o2p = ranges.cpu(), o2p.cpu()
  image, alpha, vis = orast.forward(p, f, ranges, o2p, size, cfg)
  gp, gf, heur = orast.backward(p, f, ranges, o2p, image, G.cpu().double(), size, cfg)
  return dict(image=image, alpha=alpha, visibility=vis, grad_points=gp, grad_features=gf, heuristics=heur)


def differing_rows(a, b):
  """share of rows of ``a`` that differ from ``b`` by more than 1e-3 of the largest entry"""
  rows = a.reshape(-1, a.shape[-1]) if a.dim() > 1 else a.reshape(-1, 1)
  other = b.reshape(rows.shape)
  scale = max(float(rows.abs().max()), float(other.abs().max()))
  return float(((rows - other).abs().max(dim=1).values > 1e-3 * scale).double().mean())


def sensitive_outputs(name):
  """the outputs the parameters of config ``name`` reach"""
  return ('grad_points', 'grad_features') if name.startswith('S_') else ('image', 'grad_points', 'grad_features')


def assert_sensitive(name, case, default):
  shares = {k: differing_rows(case[k], default[k]) for k in sensitive_outputs(name)}
  print(f"sensitivity {name}:", {k: round(v, 4) for k, v in shares.items()})
  for k, share in shares.items():
    assert share >= SENSITIVE_ROWS, f"{name}: the oracle's {k} at this config differs from the default's on {share:.1%} of rows only"
  return shares


def limit_config(cfg, factor):
  """``cfg`` with the saturation limit 1 - saturate_threshold scaled by ``factor``"""
  return replace(cfg, saturate_threshold=1.0 - (1.0 - cfg.saturate_threshold) * factor)


def first_saturated_entry(p, ranges, o2p, size, cfg):
  """(H, W) int: the position in its tile's list of the first entry a pixel's backward drops for saturation (the
  accumulated weight in front of it has reached saturate_threshold), -1 where the pixel never saturates"""
  p, ranges, o2p = p.cpu().double(), ranges.cpu().reshape(-1, 2), o2p.cpu()
  (w, h), ts = size, cfg.tile_size
  tiles_wide = (w + ts - 1) // ts
  out = torch.full((h, w), -1, dtype=torch.int64)
  for tile in range(ranges.shape[0]):
    start, end = int(ranges[tile, 0]), int(ranges[tile, 1])
    if end <= start:
      continue
    px, py, inb, pix = orast._tile_pixels(tile, tiles_wide, ts, w, h, p.dtype)
    g = p[o2p[start:end].long()]
    a_raw = g[None, :, 6] * orast.pdf(pix[inb], g, cfg.antialias)
    a = torch.where(a_raw > cfg.alpha_threshold, torch.clamp_max(a_raw, cfg.clamp_max_alpha), torch.zeros_like(a_raw))
    T_incl = torch.cumprod(1 - a, dim=1)
    T_excl = torch.cat([torch.ones((a.shape[0], 1), dtype=p.dtype), T_incl[:, :-1]], dim=1)
    sat = (1 - T_excl) >= cfg.saturate_threshold
    first = torch.where(sat.any(dim=1), torch.argmax(sat.to(torch.int8), dim=1), torch.full((a.shape[0],), -1))
    out[py[inb], px[inb]] = first
  return out


def flagged_rows(p, ranges, o2p, size, cfg):
  """(V,) bool: the rows with a pair within SATURATION_MARGIN of the saturation limit; at most FLAGGED_ROWS of all rows"""
  margin, _ = orast.saturation_margin(p.cpu().double(), ranges.cpu(), o2p.cpu(), size, cfg)
  flagged = margin < SATURATION_MARGIN
  share = float(flagged.double().mean())
  print(f"flagged rows: {int(flagged.sum())} of {flagged.numel()} ({share:.2%})")
  assert share <= FLAGGED_ROWS, f"{share:.2%} of rows have a pair within {SATURATION_MARGIN} of the saturation limit"
  return flagged


def saturation_rows(p, f, ranges, o2p, size, cfg, image, G):
  """(flagged (V,) bool, lo, hi): ``flagged_rows`` and the elementwise interval spanned by the oracle backward with the
  limit moved by SATURATION_MARGIN either way, as dicts of grad_points / grad_features / heuristics."""
  flagged = flagged_rows(p, ranges, o2p, size, cfg)
  p, f = p.cpu().double(), f.cpu().double()
  ranges, o2p = ranges.cpu(), o2p.cpu()
  ends = [orast.backward(p, f, ranges, o2p, image, G.cpu().double(), size, limit_config(cfg, factor))
          for factor in (1.0 - SATURATION_MARGIN, 1.0 + SATURATION_MARGIN)]
  keys = ('grad_points', 'grad_features', 'heuristics')
  lo = {k: torch.minimum(a, b) for k, a, b in zip(keys, *ends)}
  hi = {k: torch.maximum(a, b) for k, a, b in zip(keys, *ends)}
  return flagged, lo, hi
