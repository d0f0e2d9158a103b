"""-m gpu, round 6: every product path round 5 added, held against the ORACLE directly — not
against another HIP kernel:

* the long-run segment kernels (ms_raster_fwd_split / ms_raster_bwd_moments_split) with a RUN-TIME threshold (runs above
  512 entries, three segments per tile), tile 8 / 16 / 32, with visibility and with point heuristics, through the
  C-ABI and through the frame executor;
* a segment that starts behind an opaque surface (the second, visibility walk leaves its loop before staging anything:
  ADVICE round 5, high) and a plan that does not fit its capacities;
* the splat-row entry points (ms_splat_rows_pack / ms_raster_fwd_rows / ms_raster_bwd_moments_rows);
* the backward's three-deep staging pipeline at tile lists of exactly 268 / 269 / 530 / 2300 entries.

Oracle = oracle.raster.forward / backward in float64 (rasterizer/forward.py:77-110, backward.py:114-224 restated) on
the lists the GPU mapper built.  Scenes are GATE-STABLE (no (pixel, splat) pair within 1e-4 relative of the blend gate,
oracle.raster.gate_margin), so the contract tolerance applies to EVERY pixel and EVERY row: 1e-4 absolute on pixels,
1e-4 of the largest gradient on gradient rows.  Rows beyond 2e-5 are listed with the side of the backward's saturation
test their nearest pair sits on (oracle.raster.saturation_margin), not merely counted."""
import ctypes
import json

import pytest
import torch

from oracle import raster as orast
from taichi_splatting_amd import RasterConfig, _lib, frame, map_to_tiles, rasterize, rasterize_with_tiles
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
from taichi_splatting_amd.testing import random_2d_gaussians

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
TOL = 1e-4


def cfg_for(tile, **kw):
  return RasterConfig(tile_size=tile, pixel_stride=(1, 1) if tile == 8 else (2, 2), **kw)


def confined_scene(per_tile, size, tile, seed, alpha_range=(0.01, 0.03), sigma=(0.5, 0.4), inset=4.0, pool=1.5,
                   exact=False, cfg=None):
  """``per_tile`` gate-stable splats per tile with their centres ``inset`` px inside the tile.  A pool of
  ``pool * per_tile`` candidates per tile is drawn, the candidates with a (pixel, splat) pair within 1e-4 of the blend
  gate are dropped (the margin of a pair does not depend on the other splats), the first ``per_tile`` of each tile kept.
  ``cfg``: the config whose blend gate (alpha_threshold) the margin is measured at; the default one of the tile size if None."""
  tw, th = (size[0] + tile - 1) // tile, (size[1] + tile - 1) // tile
  tiles = tw * th
  n = int(per_tile * pool) * tiles
  torch.manual_seed(seed)
  g = random_2d_gaussians(n, size, scale_factor=0.6, alpha_range=alpha_range)
  owner = torch.arange(n) % tiles
  span = tile - 2 * inset
  g.position[:] = torch.stack([(owner % tw) * tile + inset + span * torch.rand(n), (owner // tw) * tile + inset + span * torch.rand(n)], 1)
  g.log_scaling[:] = torch.log(sigma[0] + sigma[1] * torch.rand(n, 2))
  cfg = cfg_for(tile) if cfg is None else cfg
  assert cfg.tile_size == tile
  p = project_gaussians2d(g)
  o2p, ranges = map_to_tiles(p.to(DEV), g.depths.reshape(-1, 1).to(DEV), size, cfg)
  margin = orast.gate_margin(p.double(), ranges.cpu(), o2p.cpu(), size, cfg)
  stable = margin > 1e-4
  keep = torch.zeros(n, dtype=torch.bool)
  for t in range(tiles):
    idx = torch.nonzero(stable & (owner == t)).squeeze(1)
    assert idx.numel() >= per_tile, (t, idx.numel(), per_tile)
    keep[idx[:per_tile]] = True
  g = g[keep]
  if exact:
    p = project_gaussians2d(g)
    o2p, ranges = map_to_tiles(p.to(DEV), g.depths.reshape(-1, 1).to(DEV), size, cfg)
    runs = (ranges[..., 1] - ranges[..., 0]).flatten()
    assert int(runs.min()) == per_tile and int(runs.max()) == per_tile, (int(runs.min()), int(runs.max()))
  return g


def lists_for(g, size, cfg):
  p = project_gaussians2d(g).to(DEV).contiguous()
  depth, f = g.depths.reshape(-1, 1).to(DEV), g.feature.to(DEV).contiguous()
  o2p, ranges = map_to_tiles(p, depth, size, cfg)
  return p, f, o2p, ranges.view(-1, 2).contiguous()


def oracle_pair(p, f, ranges, o2p, size, cfg, G):
  p64, f64 = p.cpu().double(), f.cpu().double()
  img, alpha, vis = orast.forward(p64, f64, ranges.cpu(), o2p.cpu(), size, cfg)
  gp, gf, heur = orast.backward(p64, f64, ranges.cpu(), o2p.cpu(), img, G.cpu().double(), size, cfg)
  return img, alpha, vis, gp, gf, heur


def report_rows(what, got, want, p, ranges, o2p, size, cfg, tol=TOL, flagged=None, interval=None):
  """Every row within ``tol`` of the largest gradient; the rows beyond 2e-5 are LISTED with the side of the saturation
  test their nearest pair sits on and its distance to it (gate_excess style: printed and appended to the parity log).

  ``flagged`` (rows,) bool with ``interval`` = (lo, hi): rows that have a pair on the saturation limit itself
  (tests/threshold_cases.py).  Their error is the distance, element by element, to the interval [lo, hi] instead of the
  distance to ``want``; it is held to the same ``tol``, and every one of them is listed."""
  want = want.double().cpu()
  scale = float(want.abs().max())
  assert scale > 0
  got64 = got.detach().cpu().double()
  err = (got64 - want).abs()
  listed = None
  if flagged is not None:
    lo, hi = interval
    outside = torch.clamp_min(lo - got64, 0) + torch.clamp_min(got64 - hi, 0)
    err = torch.where(flagged.reshape([-1] + [1] * (err.dim() - 1)), outside, err)
    listed = flagged
  rel = (err / scale).reshape(want.shape[0], -1).max(dim=1).values
  over = torch.nonzero(rel > 2e-5).squeeze(1)
  entry = {"what": what, "kind": "rows vs oracle", "rows": int(rel.numel()), "beyond_2e-5": int(over.numel()), "largest": float(rel.max())}
  if listed is not None:
    entry["flagged"] = int(listed.sum())
    over = torch.nonzero((rel > 2e-5) | listed).squeeze(1)
    order = torch.argsort(~listed[over], stable=True)          # the flagged rows first: all of them are listed
    over = over[order][:max(32, int(listed.sum()))]
  if over.numel():
    margin, side = orast.saturation_margin(p.cpu().double(), ranges.cpu(), o2p.cpu(), size, cfg)
    entry["beyond_2e-5_rows"] = [{"row": int(i), "rel": float(rel[i]), "saturation_side": int(side[i]),
                                  "saturation_margin": float(margin[i]),
                                  **({"flagged": bool(listed[i])} if listed is not None else {})} for i in over[:32 if listed is None else None]]
  print('parity rows:', json.dumps(entry))
  try:
    from oracle.gate_excess import _record
    _record(entry)
  except Exception:
    pass
  assert float(rel.max()) < tol, entry
  return entry


def finalize(lib, p, mom, heuristics, stream, deterministic=0, fixed_exp=None):
  n = p.shape[0]
  gp, gf = torch.empty((n, 7), device=DEV), torch.empty((n, 3), device=DEV)
  heur = torch.empty((n, 2), device=DEV) if heuristics else None
  _lib.check(lib.ms_raster_moments_finalize(p.data_ptr(), mom.data_ptr(), deterministic, _lib.ptr(fixed_exp), n, gp.data_ptr(),
                                            gf.data_ptr(), _lib.ptr(heur), stream), "finalize")
  return gp, gf, heur


def split_forward_backward(lib, p, f, o2p, ranges, size, cfg, G, min_run, seg_len, k_capacity=None, deterministic=0,
                           fixed_exp=None, rows_out=None):
  """ms_raster_fwd_split + ms_raster_bwd_moments_split + ms_raster_moments_finalize through the C-ABI.  ``deterministic``
  with ``fixed_exp`` (device int32[2]): int64 rows committed in fixed point; ``rows_out``: a list the raw rows are appended to"""
  (w, h), tile, n = size, cfg.tile_size, p.shape[0]
  k = o2p.shape[0] if k_capacity is None else k_capacity
  cfg_c, stream = _lib.raster_config_c(cfg), _lib.current_stream(torch.device(DEV))
  th = (h + tile - 1) // tile
  scratch = torch.empty((lib.ms_raster_split_scratch_bytes(k, tile, min_run, seg_len),), dtype=torch.uint8, device=DEV)
  image, alpha = torch.full((h, w, 3), float('nan'), device=DEV), torch.full((h, w), float('nan'), device=DEV)
  vis = torch.zeros(n, device=DEV) if cfg.compute_visibility else None
  _lib.check(lib.ms_raster_fwd_split(p.data_ptr(), f.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), k, w, h, cfg_c,
                                     image.data_ptr(), alpha.data_ptr(), _lib.ptr(vis), scratch.data_ptr(), min_run, seg_len,
                                     0, th, stream), "fwd split")
  counts = scratch[:16].view(torch.int32).cpu()
  mom = torch.zeros((n, _lib.MOMENT_ROW), dtype=torch.int64 if deterministic else torch.float32, device=DEV)
  _lib.check(lib.ms_raster_bwd_moments_split(p.data_ptr(), f.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), k, image.data_ptr(),
                                             G.data_ptr(), w, h, cfg_c, mom.data_ptr(), deterministic, _lib.ptr(fixed_exp),
                                             scratch.data_ptr(), min_run, seg_len, 0, th, stream), "bwd split")
  if rows_out is not None:
    rows_out.append(mom.clone())
  gp, gf, heur = finalize(lib, p, mom, cfg.compute_point_heuristic, stream, deterministic, fixed_exp)
  return image, alpha, vis, gp, gf, heur, counts


SEG_SIZES = {8: (32, 24), 16: (64, 48), 32: (96, 64)}


@pytest.mark.parametrize('tile,visibility,heuristics', [(8, False, False), (16, True, False), (16, False, True), (32, True, False)])
def test_segment_kernels_vs_oracle(tile, visibility, heuristics):
  """Tile lists of ~1400 low-opacity splats, runs above 512 entries cut into three segments of 512 (run-time
  split_min_run / split_seg_len): the forward's composition of the segments' (colour, transmittance) pairs, the second
  (visibility) walk from the composed start states, and the backward started per segment from those states, against the
  float64 oracle that walks each list front to back in one go."""
  lib = _lib.load()
  size = SEG_SIZES[tile]
  inset = 4.0 if tile > 8 else 2.5
  # (tile 8: 1400 splats on 64 pixels — opacities just above the blend gate keep every pixel short of saturation)
  g = confined_scene(1400, size, tile, seed=60 + tile, inset=inset, alpha_range=(0.0045, 0.009) if tile == 8 else (0.01, 0.03))
  cfg = cfg_for(tile, compute_visibility=visibility, compute_point_heuristic=heuristics)
  p, f, o2p, ranges = lists_for(g, size, cfg)
  runs = ranges[:, 1] - ranges[:, 0]
  assert int(runs.min()) > 1024 and int(runs.max()) < 16384          # every tile is cut; nothing reaches the default threshold
  torch.manual_seed(1)
  G = (torch.rand(size[1], size[0], 3, device=DEV) + 0.5).contiguous()
  image, alpha, vis, gp, gf, heur, counts = split_forward_backward(lib, p, f, o2p, ranges, size, cfg, G, 512, 512)
  assert int(counts[2]) == 0 and int(counts[1]) == ranges.shape[0] and int(counts[0]) >= 3 * int(counts[1]), counts[:3]

  img_o, a_o, vis_o, gp_o, gf_o, heur_o = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert float(a_o.max()) < 0.999 and float(a_o.max()) > 0.05                      # every segment really blends
  assert (image.cpu().double() - img_o).abs().max().item() < TOL                    # every pixel
  assert (alpha.cpu().double() - a_o).abs().max().item() < TOL
  if visibility:
    assert (vis.cpu().double() - vis_o).abs().max().item() < TOL * float(vis_o.max())
  what = f"segments tile {tile}"
  report_rows(what + " d gaussians2d", gp, gp_o, p, ranges, o2p, size, cfg)
  report_rows(what + " d features", gf, gf_o, p, ranges, o2p, size, cfg)
  if heuristics:
    report_rows(what + " heuristics", heur, heur_o, p, ranges, o2p, size, cfg)


def test_segments_behind_an_opaque_surface_vs_oracle():
  """Thirty-two near-opaque layers in front of every pixel, then ~1400 splats per tile nothing can see: the transmittance at
  the start of the second and third segment is below 2^-66, so the visibility walk of those segments leaves its loop
  before it has staged a batch (csrc/raster_fast.hip, the spent-tile exit) and must commit nothing; the backward's
  saturation test drops every pair behind the first few layers.  Image, visibility and gradients against the oracle."""
  lib = _lib.load()
  tile, size = 16, (64, 48)
  hidden = confined_scene(1400, size, tile, seed=77)
  n_front = 32
  torch.manual_seed(5)
  # (alpha g stays below clamp_max_alpha: two clamped layers would leave T = 0.01^2, EXACTLY the saturation limit)
  front = random_2d_gaussians(n_front, size, scale_factor=1.0, alpha_range=(0.90, 0.95))
  front.position[:] = torch.tensor([[32.0, 24.0]]) + 2.0 * torch.rand(n_front, 2)
  front.log_scaling[:] = torch.log(torch.full((n_front, 2), 120.0))
  front.depths[:] = 0.001 * torch.rand(n_front, 1)                 # in front of everything (depths of the pool are U(0, 1))
  hidden.depths[:] = 0.1 + 0.9 * hidden.depths
  g = type(hidden).cat([front, hidden])
  cfg = cfg_for(tile, compute_visibility=True)
  p, f, o2p, ranges = lists_for(g, size, cfg)
  assert int((ranges[:, 1] - ranges[:, 0]).min()) > 1024
  torch.manual_seed(2)
  G = (torch.rand(size[1], size[0], 3, device=DEV) + 0.5).contiguous()
  image, alpha, vis, gp, gf, _, counts = split_forward_backward(lib, p, f, o2p, ranges, size, cfg, G, 512, 512)
  assert int(counts[2]) == 0 and int(counts[1]) == ranges.shape[0]
  img_o, a_o, vis_o, gp_o, gf_o, _ = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert float(a_o.min()) > 1.0 - 1e-15                                    # opaque everywhere
  assert bool(torch.isfinite(vis).all()) and bool(torch.isfinite(image).all())
  assert (image.cpu().double() - img_o).abs().max().item() < TOL
  assert (alpha.cpu().double() - a_o).abs().max().item() < TOL
  assert (vis.cpu().double() - vis_o).abs().max().item() < 1e-5 * float(vis_o.max())
  assert float(vis[n_front:].abs().max()) < 1e-12                          # nothing behind the surface is visible
  # (T falls by a factor ~10 per layer; a pair that sat on the saturation limit would toggle a weight of 1e-4 on one of
  # 3072 pixels of a front splat's row: report_rows lists such rows, none is excused)
  report_rows("segments behind an opaque surface, d gaussians2d", gp, gp_o, p, ranges, o2p, size, cfg)
  report_rows("segments behind an opaque surface, d features", gf, gf_o, p, ranges, o2p, size, cfg)


def test_split_plan_that_does_not_fit_falls_back_to_the_per_tile_kernels():
  """k_capacity far below the real overlap count (C-ABI misuse): the plan does not fit the capacities derived from it,
  is dropped as a whole (scratch word [2]) and every tile is rendered by its own workgroup — the image is bit for bit
  ms_raster_fwd's and matches the oracle, the gradients match the oracle.  Round 5 processed unwritten plan slots."""
  lib = _lib.load()
  tile, size = 16, (64, 48)
  g = confined_scene(1400, size, tile, seed=91)
  cfg = cfg_for(tile)
  p, f, o2p, ranges = lists_for(g, size, cfg)
  torch.manual_seed(3)
  G = (torch.rand(size[1], size[0], 3, device=DEV) + 0.5).contiguous()
  image, alpha, _, gp, gf, _, counts = split_forward_backward(lib, p, f, o2p, ranges, size, cfg, G, 512, 512, k_capacity=600)
  assert int(counts[2]) == 1
  plain = rasterize_with_tiles(p, f, o2p, ranges, size, cfg)
  assert torch.equal(image, plain.image) and torch.equal(alpha, plain.image_weight)
  img_o, a_o, _, gp_o, gf_o, _ = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert (image.cpu().double() - img_o).abs().max().item() < TOL
  report_rows("void split plan, d gaussians2d", gp, gp_o, p, ranges, o2p, size, cfg)
  report_rows("void split plan, d features", gf, gf_o, p, ranges, o2p, size, cfg)


def test_frame_executor_segments_vs_oracle():
  """rasterize() on the frame executor with the segment launches switched on for every frame and a 512-entry threshold
  (frame.set_split_policy): plan, segment forward, composition, segment backward inside the frame's fixed launch
  sequence — image and both 2D gradients against the oracle."""
  tile, size = 16, (64, 48)
  g = confined_scene(1400, size, tile, seed=101)
  cfg = cfg_for(tile)
  p, f, o2p, ranges = lists_for(g, size, cfg)
  depth = g.depths.reshape(-1, 1).to(DEV)
  torch.manual_seed(4)
  G = (torch.rand(size[1], size[0], 3, device=DEV) + 0.5).contiguous()
  states = []

  class Recording(frame.FrameState):
    def __init__(self):
      super().__init__()
      states.append(self)
  original = frame.FrameState
  frame.release_caches()
  frame.set_split_policy(min_run=512, seg_len=512, always=True)
  frame.FrameState = Recording
  try:
    pg, fg = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out = rasterize(pg, depth, fg, size, cfg)
    (out.image * G).sum().backward()
    torch.cuda.synchronize()
    st = states[-1]
    assert int(st.desc.split_long_runs) == 512 and int(st.desc.split_seg_len) == 512
    off = st.layout.split_scratch
    counts = st.keep_k[off:off + 16].view(torch.int32).cpu()
    assert int(counts[2]) == 0 and int(counts[1]) == ranges.shape[0] and int(counts[0]) >= 3 * int(counts[1]), counts[:3]
    assert torch.equal(st.overlap_to_point()[:o2p.shape[0]], o2p)          # the frame built the lists the oracle is given
  finally:
    frame.FrameState = original
    frame.set_split_policy()
    frame.release_caches()
  img_o, a_o, _, gp_o, gf_o, _ = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert (out.image.detach().cpu().double() - img_o).abs().max().item() < TOL
  assert (out.image_weight.cpu().double() - a_o).abs().max().item() < TOL
  report_rows("frame executor segments, d gaussians2d", pg.grad, gp_o, p, ranges, o2p, size, cfg)
  report_rows("frame executor segments, d features", fg.grad, gf_o, p, ranges, o2p, size, cfg)


def splat_rows_forward(lib, p, depth, f, o2p, ranges, size, cfg):
  """ms_splat_rows_pack + ms_raster_fwd_rows through the C-ABI: (rows, image, alpha, visibility)"""
  n, (w, h), tile = p.shape[0], size, cfg.tile_size
  cfg_c, stream = _lib.raster_config_c(cfg), _lib.current_stream(torch.device(DEV))
  th = (h + tile - 1) // tile
  rows = torch.full((n, _lib.SPLAT_ROW), float('nan'), device=DEV)
  _lib.check(lib.ms_splat_rows_pack(p.data_ptr(), depth.data_ptr(), f.data_ptr(), n, rows.data_ptr(), stream), "pack")
  image, alpha, vis = torch.empty((h, w, 3), device=DEV), torch.empty((h, w), device=DEV), torch.zeros(n, device=DEV)
  _lib.check(lib.ms_raster_fwd_rows(rows.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), w, h, cfg_c, image.data_ptr(),
                                    alpha.data_ptr(), vis.data_ptr(), 0, th, stream), "fwd rows")
  return rows, image, alpha, vis


def splat_rows_backward(lib, rows, o2p, ranges, image, G, size, cfg):
  """ms_raster_bwd_moments_rows through the C-ABI: (return code, moments)"""
  n, (w, h), tile = rows.shape[0], size, cfg.tile_size
  cfg_c, stream = _lib.raster_config_c(cfg), _lib.current_stream(torch.device(DEV))
  th = (h + tile - 1) // tile
  mom = torch.zeros((n, _lib.MOMENT_ROW), device=DEV)
  rc = lib.ms_raster_bwd_moments_rows(rows.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), image.data_ptr(), G.data_ptr(), w, h,
                                      cfg_c, mom.data_ptr(), 0, None, 0, th, stream)
  return rc, mom


@pytest.mark.parametrize('tile,heuristics', [(16, False), (16, True), (32, False), (8, False)])
def test_splat_row_entry_points_vs_oracle(tile, heuristics):
  """ms_splat_rows_pack -> ms_raster_fwd_rows -> ms_raster_bwd_moments_rows (one 64-byte row per splat gathered instead
  of two dense arrays) against the oracle at BASELINE config A's density (4 700 random 2D gaussians, 192 x 160),
  gate-stable: image, alpha, visibility, both gradients, heuristics.  Tile 8 offers the forward only."""
  lib = _lib.load()
  size = (192, 160)                  # (config A's density at 0.47 of its area: the oracle is most of this test's time)
  cfg = cfg_for(tile, compute_visibility=True, compute_point_heuristic=heuristics)
  torch.manual_seed(tile + (100 if heuristics else 0))
  g0 = random_2d_gaussians(4700, size)
  p0 = project_gaussians2d(g0)
  o2p0, ranges0 = map_to_tiles(p0.to(DEV), g0.depths.reshape(-1, 1).to(DEV), size, cfg)
  keep = orast.gate_margin(p0.double(), ranges0.cpu(), o2p0.cpu(), size, cfg) > 1e-4
  assert float(keep.float().mean()) > 0.7
  g = g0[keep]
  p, f, o2p, ranges = lists_for(g, size, cfg)
  (w, h) = size
  depth = g.depths.reshape(-1).to(DEV).contiguous()
  rows, image, alpha, vis = splat_rows_forward(lib, p, depth, f, o2p, ranges, size, cfg)
  torch.manual_seed(1)
  G = (torch.rand(h, w, 3, device=DEV) + 0.5).contiguous()
  img_o, a_o, vis_o, gp_o, gf_o, heur_o = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert (image.cpu().double() - img_o).abs().max().item() < TOL
  assert (alpha.cpu().double() - a_o).abs().max().item() < TOL
  assert (vis.cpu().double() - vis_o).abs().max().item() < TOL * float(vis_o.max())
  rc, mom = splat_rows_backward(lib, rows, o2p, ranges, image, G, size, cfg)
  if tile == 8:
    assert rc == -2                                                     # MS_ERR_UNSUPPORTED (measured slower: not offered)
    return
  _lib.check(rc, "bwd rows")
  gp, gf, heur = finalize(lib, p, mom, heuristics, _lib.current_stream(torch.device(DEV)))
  what = f"splat rows tile {tile}"
  report_rows(what + " d gaussians2d", gp, gp_o, p, ranges, o2p, size, cfg)
  report_rows(what + " d features", gf, gf_o, p, ranges, o2p, size, cfg)
  if heuristics:
    report_rows(what + " heuristics", heur, heur_o, p, ranges, o2p, size, cfg)


@pytest.mark.parametrize('per_tile', [268, 269, 530, 2300])
def test_backward_staging_cases_vs_oracle(per_tile):
  """The raster backward stages a tile's list in equal batches of <= 268 splats through a three-deep register pipeline
  whose last 12 slots travel one component per lane (csrc/raster_bwd_scan.hip): tile lists of EXACTLY 268 (one full
  batch), 269 (two batches of 135 / 134), 530 and 2300 entries against the float64 oracle — image and every gradient row
  (a dropped or misplaced slot loses a whole splat: an error of order 1 on its row)."""
  tile, size = 16, (64, 48)
  g = confined_scene(per_tile, size, tile, seed=per_tile, exact=True)
  cfg = cfg_for(tile)
  p, f, o2p, ranges = lists_for(g, size, cfg)
  runs = ranges[:, 1] - ranges[:, 0]
  assert int(runs.min()) == per_tile == int(runs.max())
  torch.manual_seed(1)
  G = (torch.rand(size[1], size[0], 3, device=DEV) + 0.5).contiguous()
  pg, fg = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
  out = rasterize_with_tiles(pg, fg, o2p, ranges, size, cfg)
  (out.image * G).sum().backward()
  img_o, a_o, _, gp_o, gf_o, _ = oracle_pair(p, f, ranges, o2p, size, cfg, G)
  assert float(a_o.max()) < 0.9999                                          # nothing saturates: every batch blends
  assert (out.image.detach().cpu().double() - img_o).abs().max().item() < TOL
  report_rows(f"staging {per_tile} d gaussians2d", pg.grad, gp_o, p, ranges, o2p, size, cfg)
  report_rows(f"staging {per_tile} d features", fg.grad, gf_o, p, ranges, o2p, size, cfg)
  # and every splat got its gradient: none lost most of its own row
  own = (pg.grad.cpu().double() - gp_o).abs().max(dim=1).values / gp_o.abs().max(dim=1).values.clamp_min(1e-3 * float(gp_o.abs().max()))
  assert int((own > 0.5).sum()) == 0


# ---- eager frames that look at their overlap total late (frame.LAZY_SETTLE) ----------------
def _train_scene(n=30000, size=(320, 240), seed=3):
  from taichi_splatting_amd.testing import random_3d_gaussians, random_camera
  torch.manual_seed(seed)
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(n, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  return g.replace(feature=torch.rand(n, 3)), cam


def test_lazily_settled_frames_equal_settled_frames_and_do_not_wait():
  """With frame.LAZY_SETTLE (opt-in), from the fifth frame of a scene shape on a frame that will be differentiated is not
  settled before it returns:
  its backward is enqueued without a look at the overlap total (frame.host_syncs stays put), the look happens at the
  next frame's entry.  Images and gradients are bit for bit those of frames settled the round-5 way (MS_STRICT-like:
  LAZY_SETTLE off) — the kernels and their launch order are the same, only the host's wait moved."""
  from taichi_splatting_amd import render_gaussians
  g, cam = _train_scene()
  cfg = RasterConfig()
  weight = torch.linspace(0.5, 1.5, 240 * 320 * 3, device=DEV).view(240, 320, 3)
  results = {}
  default = frame.LAZY_SETTLE
  for lazy in (False, True):
    frame.release_caches()
    frame.LAZY_SETTLE = lazy
    try:
      outs, waits = [], []
      for it in range(7):
        gd, camd = g.to(DEV), cam.to(device=DEV)
        gd.requires_grad_(True)
        before = frame.host_syncs
        r = render_gaussians(gd, camd, cfg, use_sh=False)
        pending = r.frame.pending is not None
        (r.image * weight).sum().backward()
        waits.append((frame.host_syncs - before, pending))
        outs.append((r.image.detach().clone(), gd.position.grad.clone(), gd.feature.grad.clone()))
      torch.cuda.synchronize()
      frame.settle_all()
      results[lazy] = (outs, waits)
    finally:
      frame.LAZY_SETTLE = default
      frame.release_caches()
  strict_waits, lazy_waits = results[False][1], results[True][1]
  assert all(w == (1, False) for w in strict_waits), strict_waits
  # (a lazily settled frame of this small scene may find its total already written when its backward is enqueued and
  # settle there, without waiting; what it never does is look before it returns)
  assert lazy_waits[:3] == [(1, False)] * 3 and all(w[1] for w in lazy_waits[4:]), lazy_waits
  for a, b in zip(results[False][0], results[True][0]):
    assert torch.equal(a[0], b[0])
    for x, y in zip(a[1:], b[1:]):                       # float atomics: arrival order
      assert float((x - y).abs().max()) <= 2e-5 * float(x.abs().max())


def test_an_overflow_found_late_is_raised_not_swallowed():
  """A lazily settled frame whose overlap total exceeds the remembered capacity (the splats grew threefold between two
  frames of one scene shape) has rendered the background and returned zero gradients by the time the host looks: the look
  (here: the next frame's entry) raises FrameOverflow, the capacity is raised, and the frame after that is right again.
  A frame rendered WITHOUT gradients is always settled before it returns and is re-run in place."""
  from taichi_splatting_amd import render_gaussians
  import math
  g, cam = _train_scene(seed=4)
  cfg = RasterConfig()
  frame.release_caches()
  default = frame.LAZY_SETTLE
  frame.LAZY_SETTLE = True
  try:
    for it in range(5):                                     # the shape settles: capacity known, stable
      gd = g.to(DEV).requires_grad_(True)
      render_gaussians(gd, cam.to(device=DEV), cfg, use_sh=False).image.sum().backward()
    big = g.replace(log_scaling=g.log_scaling + math.log(3.0))
    gd = big.to(DEV).requires_grad_(True)
    camd = cam.to(device=DEV)
    torch.cuda._sleep(400_000_000)                          # the GPU is busy (~0.2 s), as it is a frame behind in a training loop:
    r = render_gaussians(gd, camd, cfg, use_sh=False)       # the host enqueues forward AND backward before K exists
    assert r.frame.pending is not None
    r.image.sum().backward()                                # enqueued on the overflowed (empty) lists
    assert r.frame.consumed
    torch.cuda.synchronize()
    with pytest.raises(frame.FrameOverflow, match="zero gradients"):
      render_gaussians(big.to(DEV), cam.to(device=DEV), cfg, use_sh=False)
    assert float(gd.position.grad.abs().max()) == 0.0       # what the message says
    # the next frames of the shape have room, with or without gradients
    with torch.no_grad():
      want = render_gaussians(big.to(DEV), cam.to(device=DEV), cfg, use_sh=False).image
    gd = big.to(DEV).requires_grad_(True)
    r = render_gaussians(gd, cam.to(device=DEV), cfg, use_sh=False)
    r.image.sum().backward()
    frame.settle_all()
    assert torch.equal(r.image.detach(), want) and float(gd.position.grad.abs().max()) > 0
    assert float(want.max()) > 0.05
    # no gradients: settled before it returns, re-run in place when it does not fit
    frame.release_caches()
    for it in range(5):
      with torch.no_grad():
        render_gaussians(g.to(DEV), cam.to(device=DEV), cfg, use_sh=False)
    with torch.no_grad():
      r = render_gaussians(big.to(DEV), cam.to(device=DEV), cfg, use_sh=False)
    assert r.frame.pending is None and torch.equal(r.image, want)
  finally:
    frame.LAZY_SETTLE = default
    frame.release_caches()


# ---- scene shapes of the round-6 sweep (tools/sweep_scenes.py): half-culled, needle splats -------------------------
def _shape_scene(kind, n, size, seed):
  import math
  from taichi_splatting_amd.testing import random_3d_gaussians, random_camera
  torch.manual_seed(seed)
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(n, cam, scale_factor=0.7 if kind == 'needle' else 1.0, alpha_range=(0.1, 0.9),
                          margin=0.5 if kind == 'culled' else 0.0)
  if kind == 'needle':
    stretch = torch.zeros(n, 3)
    stretch[torch.arange(n), torch.randint(0, 3, (n,))] = math.log(10.0)
    g = g.replace(log_scaling=g.log_scaling + stretch)
  return g.replace(feature=torch.rand(n, 3)), cam


@pytest.mark.parametrize('kind', ['culled', 'needle'])
@pytest.mark.parametrize('tile', [8, 16, 32])
def test_new_sweep_shapes_lists_against_the_oracle(kind, tile):
  """Half-culled scenes (56 % of the gaussians outside the image: the compaction's int64 index list, N-sized buffers with
  V ~ N / 2 live rows) and needle splats (aspect ~10 at random orientations: the oriented-box test decides most tile
  candidates): the tile lists of both mapper sequences are identical to the numpy oracle's (tile, depth bits, point
  index) order, and the frame executor — which never compacts — renders the image of the modular operators (to float32
  rounding: its sort keys come from ndc depths evaluated in double inside the key kernel, torch's float32 ndc values can
  order two nearly coincident splats the other way round)."""
  from oracle import mapper as omap
  from taichi_splatting_amd import render_gaussians
  from taichi_splatting_amd.perspective.projection import project_to_image
  from taichi_splatting_amd.rendering import ndc_depth
  size = (400, 304)
  n = 30000
  g, cam = _shape_scene(kind, n, size, seed=tile + (50 if kind == 'needle' else 0))
  cfg = cfg_for(tile)
  gd, camd = g.to(DEV), cam.to(device=DEV)
  with torch.no_grad():
    g2d, depths, idx = project_to_image(gd, camd, cfg)
  v = g2d.shape[0]
  if kind == 'culled':
    assert 0.3 * n < v < 0.7 * n and idx.dtype == torch.int64, v
  else:
    sig = g2d[:, 4:6]
    assert float((sig.max(dim=1).values / sig.min(dim=1).values).median()) > 3.0        # needles on screen too
  ndc = ndc_depth(depths, cam.near_plane, cam.far_plane)
  want_o2p, want_ranges, _ = omap.map_to_tiles(g2d.cpu().numpy(), ndc.cpu().reshape(-1).numpy(), size, tile, cfg.alpha_threshold)
  for method in ('direct', 'presort'):
    o2p, ranges = map_to_tiles(g2d, ndc, size, cfg, method=method)
    assert o2p.shape[0] == want_o2p.shape[0], (method, o2p.shape[0], want_o2p.shape[0])
    assert torch.equal(ranges.view(-1, 2).cpu(), torch.from_numpy(want_ranges).view(-1, 2)), method
    assert torch.equal(o2p.cpu(), torch.from_numpy(want_o2p)), method
  # frame executor (gaussians stay in place, culled ones carry depth 0) against the modular operators on the compacted set
  frame.release_caches()
  try:
    with torch.no_grad():
      r = render_gaussians(gd, camd, cfg, use_sh=False)
      o2p, ranges = map_to_tiles(g2d, ndc, size, cfg)
      want = rasterize_with_tiles(g2d, gd.feature[idx], o2p, ranges.view(-1, 2), size, cfg)
    assert float((r.image - want.image).abs().max()) < 2e-6 and float((r.image_weight - want.image_weight).abs().max()) < 2e-6
    assert float(want.image.max()) > 0.05
    assert int(frame.frame_status(r)['overlaps']) == want_o2p.shape[0]
    assert torch.equal(r.points.idx, idx)
  finally:
    frame.release_caches()


def test_first_frame_of_a_shape_maps_with_the_presort_and_carries_the_segments():
  """The first frame of a scene shape knows nothing about how its overlaps are spread: it runs the sequence whose cost
  does not depend on that (pre-sort) with the long-run segments switched on, the next frames what the shape settled on.
  Same lists, same image either way."""
  from taichi_splatting_amd import render_gaussians
  g, cam = _shape_scene('plain', 30000, (320, 240), seed=9)
  cfg = RasterConfig()
  frame.release_caches()
  try:
    gd, camd = g.to(DEV), cam.to(device=DEV)
    with torch.no_grad():
      first = render_gaussians(gd, camd, cfg, use_sh=False)
      second = render_gaussians(gd, camd, cfg, use_sh=False)
    assert int(first.frame.desc.mapper) == _lib.MAPPER_PRESORT and int(first.frame.desc.split_long_runs) == 1
    assert int(second.frame.desc.mapper) == _lib.MAPPER_DIRECT and int(second.frame.desc.split_long_runs) == 0
    assert torch.equal(first.image, second.image)
    assert torch.equal(first.frame.overlap_to_point()[:first.frame.k], second.frame.overlap_to_point()[:second.frame.k])
  finally:
    frame.release_caches()


# ---- visibility of a frame that will be differentiated, from its backward pass (frame.VISIBILITY_FROM_BACKWARD, opt-in) --
def _vis_frames(cfg, deferred, det=False, read_early=False, n=30000, size=(320, 240)):
  from taichi_splatting_amd import render_gaussians
  from taichi_splatting_amd.rasterizer import function as raster_function
  g, cam = _train_scene(n=n, size=size)
  g, cam = g.to(DEV), cam.to(device=DEV)
  g.requires_grad_(True)
  weight = torch.linspace(0.5, 1.5, size[0] * size[1] * 3, device=DEV).view(size[1], size[0], 3)
  keep = frame.VISIBILITY_FROM_BACKWARD, raster_function.DETERMINISTIC_BACKWARD
  frame.VISIBILITY_FROM_BACKWARD, raster_function.DETERMINISTIC_BACKWARD = deferred, det
  try:
    r = render_gaussians(g, cam, cfg, use_sh=False)
    state = r.frame
    early = frame.point_outputs(r)['visibility'].clone() if read_early else None
    flags = (state.vis_deferred, state.vis_ready)
    (r.image * weight).sum().backward()
    out = frame.point_outputs(r)
    torch.cuda.synchronize()
  finally:
    frame.VISIBILITY_FROM_BACKWARD, raster_function.DETERMINISTIC_BACKWARD = keep
  return r, g, early, flags, out


@pytest.mark.parametrize('tile,det', [(16, False), (8, False), (32, False), (16, True)])
def test_visibility_written_by_the_backward_pass_vs_oracle(tile, det):
  """With frame.VISIBILITY_FROM_BACKWARD a frame that will be differentiated with point heuristics on runs its forward
  WITHOUT the visibility sums; the raster backward adds the blend weights of the pairs it visits as a twelfth column of the
  heuristics row and the per-gaussian pass writes them: oracle.raster.active_visibility — the reference's visibility minus
  the pairs behind a pixel's saturation point — in the float-row and in the fixed-point (deterministic) commit.  The
  default frame's visibility is the oracle's forward's; images, gradients and heuristics are the same either way."""
  cfg = cfg_for(tile, compute_visibility=True, compute_point_heuristic=True)
  assert frame.VISIBILITY_FROM_BACKWARD is False                       # opt-in
  passes = frame.visibility_passes
  rb, gb, _, flags_b, out_b = _vis_frames(cfg, True, det)
  rf, gf, _, flags_f, out_f = _vis_frames(cfg, False, det)
  assert flags_b == (True, False) and rb.frame.vis_ready and flags_f == (False, True)
  assert frame.visibility_passes == passes                     # read after the backward pass: no pass on demand
  vis_b, vis_f = out_b['visibility'].cpu().double(), out_f['visibility'].cpu().double()
  assert int((vis_f > 0).sum()) > 1000
  assert torch.equal(rb.image, rf.image)
  assert float((gb.position.grad - gf.position.grad).abs().max()) <= 2e-5 * float(gf.position.grad.abs().max())   # float atomics
  hb, hf = out_b['point_heuristic'], out_f['point_heuristic']
  assert float((hb - hf).abs().max()) <= 1e-4 * float(hf.abs().max())
  # the oracle on the frame's own lists
  state, _, points7, _, _, _, _, _, _ = object.__getattribute__(rf, 'points').args
  k = int(state.counters()[0])
  size = (320, 240)
  p64 = points7.detach().cpu().double()
  ranges, o2p = state.tile_ranges().reshape(-1, 2).cpu(), state.overlap_to_point()[:k].cpu()
  _, alpha_o, vis_o = orast.forward(p64, gf.feature.detach().cpu().double(), ranges, o2p, size, cfg)
  act_o = orast.active_visibility(p64, ranges, o2p, size, cfg)
  assert float(alpha_o.max()) > 0.9999                                   # the scene does saturate: the two differ
  assert float((vis_o - act_o).max()) > 5e-4 and float((vis_o - act_o).min()) >= 0.0
  tol = lambda want: 2e-5 + 1e-4 * want.abs()
  # a pair whose saturation test T_before <= 1 - saturate_threshold falls the other way in float32 toggles a weight of
  # <= alpha 1e-4: saturation_margin says which splats have a pair that close to the line (T is good to ~1e-4 relative
  # after a tile's few hundred factors); the others must agree like the forward's do
  margin, _ = orast.saturation_margin(p64, ranges, o2p, size, cfg)
  # (and the blend gate alpha > alpha_threshold, forward.py:99-101: a pair within float32's reach of it toggles alpha T)
  firm = (margin > 2e-3) & (orast.gate_margin(p64, ranges, o2p, size, cfg) > 1e-4)
  assert int(firm.sum()) > 0.8 * firm.numel()
  err = (vis_b - act_o).abs()
  assert bool((err[firm] <= tol(act_o[firm])).all()), float(err[firm].max())
  assert float(err.max()) < 5e-3                                          # a few toggled pixel pairs at most
  err_f = (vis_f - vis_o).abs()
  assert bool((err_f[firm] <= tol(vis_o[firm])).all()) and float(err_f.max()) < 5e-3


def test_visibility_read_before_the_backward_pass_is_computed_on_demand():
  """``point_outputs`` / ``rendering.points`` before ``backward()`` on a deferred frame: the forward's visibility kernel
  runs on the frame's kept lists (counted in frame.visibility_passes) and gives the forward's number.  Frames that will
  not be differentiated, or run without heuristics, are not deferred at all."""
  from taichi_splatting_amd import render_gaussians
  cfg = cfg_for(16, compute_visibility=True, compute_point_heuristic=True)
  passes = frame.visibility_passes
  r, g, early, flags, out = _vis_frames(cfg, True, read_early=True)
  assert flags == (True, True) and frame.visibility_passes == passes + 1
  _, _, _, _, want = _vis_frames(cfg, False)
  assert torch.allclose(early, want['visibility'], rtol=1e-4, atol=1e-5)
  keep = frame.VISIBILITY_FROM_BACKWARD
  frame.VISIBILITY_FROM_BACKWARD = True
  try:
    g3, cam = _train_scene()
    g3, cam = g3.to(DEV), cam.to(device=DEV)
    g3.requires_grad_(True)
    r3 = render_gaussians(g3, cam, cfg, use_sh=False)
    assert r3.frame.vis_deferred and not r3.frame.vis_ready
    pts = r3.points
    assert r3.frame.vis_ready and frame.visibility_passes == passes + 2
    assert torch.allclose(pts.visibility, want['visibility'][pts.idx], rtol=1e-4, atol=1e-5)
    with torch.no_grad():
      r4 = render_gaussians(g3, cam, cfg, use_sh=False)
    assert not r4.frame.vis_deferred
    r5 = render_gaussians(g3, cam, cfg_for(16, compute_visibility=True), use_sh=False)
    assert not r5.frame.vis_deferred
    assert torch.allclose(frame.point_outputs(r4)['visibility'], want['visibility'], rtol=1e-4, atol=1e-5)
    assert torch.allclose(frame.point_outputs(r5)['visibility'], want['visibility'], rtol=1e-4, atol=1e-5)
  finally:
    frame.VISIBILITY_FROM_BACKWARD = keep


def test_visibility_from_the_backward_pass_under_hip_graph_capture():
  """A captured training step with frame.VISIBILITY_FROM_BACKWARD: every replay's backward pass writes the visibility of
  the frame returned by the capture (same tensor, new values when the parameters moved), no pass on demand, no host wait."""
  from taichi_splatting_amd import render_gaussians
  cfg = cfg_for(16, compute_visibility=True, compute_point_heuristic=True)
  g, cam = _train_scene(n=20000, size=(256, 192))
  g, cam = g.to(DEV), cam.to(device=DEV)
  g.requires_grad_(True)
  leaves = [g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature]
  keep = frame.VISIBILITY_FROM_BACKWARD
  frame.VISIBILITY_FROM_BACKWARD = True
  try:
    def step():
      for t in leaves:
        t.grad = None
      r = render_gaussians(g, cam, cfg, use_sh=False)
      r.image.sum().backward()
      return r

    ref = step()
    want = frame.point_outputs(ref)['visibility'].clone()
    del ref
    graph = frame.FrameGraph(step, warmup=2)
    passes, syncs = frame.visibility_passes, frame.host_syncs
    for _ in range(2):
      r = graph.replay()
    vis = frame.point_outputs(r)['visibility']
    torch.cuda.synchronize()
    assert r.frame.vis_deferred and frame.visibility_passes == passes and frame.host_syncs == syncs
    assert torch.allclose(vis, want, rtol=1e-5, atol=1e-6) and int((vis > 0).sum()) > 1000
    with torch.no_grad():
      g.alpha_logit -= 1.0                       # fainter splats: more of each is seen
    graph.replay()
    torch.cuda.synchronize()
    moved = frame.point_outputs(r)['visibility']
    assert float((moved - want).abs().max()) > 1e-3
    eager = step()
    assert torch.allclose(moved, frame.point_outputs(eager)['visibility'], rtol=1e-5, atol=1e-6)
  finally:
    frame.VISIBILITY_FROM_BACKWARD = keep


def test_captured_frames_evaluate_their_sh_colours_on_a_second_stream():
  """Under HIP-graph capture the SH pass runs on the executor's second stream, beside the mapper's launches, and the raster
  forward waits for its event (ms_frame_sh_colours, ms_frame_inputs.colours_ready_event); eager frames keep one stream
  (between two queues the fork and the join cost more than the overlap returns).  Same image and gradients either way."""
  from taichi_splatting_amd import render_gaussians
  from taichi_splatting_amd.testing import random_3d_gaussians, random_camera
  torch.manual_seed(5)
  size = (256, 192)
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(20000, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  g = g.replace(feature=(torch.rand(20000, 3, 16) - 0.5) * 0.5).to(DEV)
  cam = cam.to(device=DEV)
  g.requires_grad_(True)
  leaves = [g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature]
  cfg = RasterConfig()

  def step():
    for t in leaves:
      t.grad = None
    r = render_gaussians(g, cam, cfg, use_sh=True)
    r.image.sum().backward()
    return r

  ref = step()
  assert ref.frame.colours_ready is None                      # eager: one stream
  ref_image, ref_grads = ref.image.detach().clone(), [t.grad.clone() for t in leaves]
  del ref
  results = {}
  keep = frame.SH_SIDE_STREAM
  try:
    for side in (True, False):
      frame.SH_SIDE_STREAM = side
      graph = frame.FrameGraph(step, warmup=1)
      for _ in range(2):
        r = graph.replay()
      torch.cuda.synchronize()
      assert (r.frame.colours_ready is not None) == side
      results[side] = (r.image.detach().clone(), [t.grad.clone() for t in leaves])
  finally:
    frame.SH_SIDE_STREAM = keep
  for side in (True, False):
    image, grads = results[side]
    assert torch.equal(image, ref_image)
    for got, want in zip(grads, ref_grads):                    # float atomics: arrival order
      assert float((got - want).abs().max()) <= 2e-5 * float(want.abs().max())


def test_visibility_from_the_backward_pass_is_the_colour_gradient_of_a_unit_loss():
  """The twelfth column sums the blend weights of exactly the pairs the colour gradient sums (d f_c = sum w dL/dC_c,
  backward.py:197): with loss = image.sum() the deferred visibility equals d feature[:, 0] bit for bit — same pairs, same
  order, same atomics."""
  from taichi_splatting_amd import render_gaussians
  cfg = cfg_for(16, compute_visibility=True, compute_point_heuristic=True)
  g, cam = _train_scene()
  g, cam = g.to(DEV), cam.to(device=DEV)
  g.requires_grad_(True)
  keep = frame.VISIBILITY_FROM_BACKWARD
  frame.VISIBILITY_FROM_BACKWARD = True
  try:
    r = render_gaussians(g, cam, cfg, use_sh=False)
    r.image.sum().backward()
    vis = frame.point_outputs(r)['visibility']
    torch.cuda.synchronize()
  finally:
    frame.VISIBILITY_FROM_BACKWARD = keep
  assert r.frame.vis_deferred and int((vis > 0).sum()) > 1000
  # (one commit per (patch, splat) carries both columns: whatever order the atomics arrive in, they arrive in it for both)
  assert torch.equal(vis, g.feature.grad[:, 0])
