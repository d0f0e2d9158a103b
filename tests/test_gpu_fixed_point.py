"""-m gpu: the fixed-point commits of the deterministic raster backward (``DETERMINISTIC_BACKWARD``; csrc/raster_bwd_scan.hip,
``commit_pass``) against float64 — the unit selection itself, the columns that carry their own unit (9: prune_cost's sum
of squares, 11: the blend weights), a dL/dimage with dynamic range, and the headroom of the int64 rows.

a. ``ms_fixed_point_exponents`` and ``ms_fixed_point_exponents_ranged`` equal a Python mirror built on ``math.frexp``
   (tests/moments_oracle.py), integer for integer, the +-100 clamps included.
b. Raw rows, deterministic against float atomics, with a DERIVED bound.  Both modes commit the same float32 per-(patch,
   splat) values; with V their real-number sum, |int 2^-e - V| <= P u / 2 (P commits, each rounded to nearest) and
   |float - V| <= (P - 1) 2^-24 A (P - 1 float additions of partial sums of magnitude <= A), so per row and column
       |int64 2^-e - float32| <= P[i] u_c / 2 + 1.01 P[i] 2^-24 A[i, c]
   with P and A from the float64 oracle of the rows (the 1.01 covers float32-against-float64 differences in A) and u_c the
   column's unit: main, the squared one for column 9, 2^-32 for column 11.  No measured constant enters.  A swapped or
   mis-scaled unit, a wrong exponent, truncation instead of rounding (it accumulates to P u) and a wrapped row all fail it.
   Scene A, tile 8 / 16 / 32, heuristics on, for a randn dL/dimage, the constant one of a mean-reduced loss, and one with
   30 bits of dynamic range (randn 2^-30 everywhere but for one 4 x 4 block of randn).
c. The same three dL/dimage through ``rasterize_with_tiles``, and one SH frame through ``render_gaussians`` (the FIXED
   per-gaussian pass reads the rows), against the float64 oracle at the project's tolerance.
d. Scaling dL/dimage by 2^k moves the exponents by exactly k and every step is linear in dL/dimage (quadratic for
   prune_cost), so the deterministic outputs for G 2^k are 2^k times those for G BIT FOR BIT (4^k for prune_cost),
   k in {-40, -13, 13, 40}; prune_cost at +-13 only: beyond, its per-pixel squares (dL/dalpha ~ 1e-2 |G| at the
   tails, squared and scaled by 4^-40 = 8e-25) leave the normal range of float32.  The visibility of a frame that takes it
   from the backward pass (column 11) is identical at every k; ``rasterize_with_tiles`` returns the FORWARD's visibility,
   which does not see dL/dimage and is summed with float atomics (not repeatable from run to run): not compared there.
e. The segment kernels (``ms_raster_bwd_moments_split``) with deterministic commits: rows bitwise repeatable, outputs
   against the oracle.
f. Headroom: a background splat over a 256 x 256 image with colours of 4000 (column 0 reaches 2^63.5 units of
   ``ms_fixed_point_exponents``) or of 100 at alpha 0.9 (column 9: 2^66.5), against the oracle.

CPU conditions on the units (tests/test_moments_oracle_host.py), scene A, quantisation P_max u_c / 2 over the largest
|sum| of the column, columns 0..10, P_max = 21 — identical for both forms, since the ranged form coarsens nothing where
the amax-only units fit (150 x 100 pixels, colours <= 1):
  randn dL/dimage (exponents 33, 30):  2.1e-10 2.7e-10 3.7e-10 4.3e-10 7.0e-10 4.0e-10 9.8e-11 1.0e-10 7.4e-11 3.0e-11 1.2e-10
  mean  dL/dimage (exponents 51, 66):  3.0e-12 1.2e-11 2.3e-11 4.5e-12 5.1e-11 4.6e-12 2.1e-12 2.1e-12 2.1e-12 7.5e-13 1.2e-11
against the 1e-6 the condition allows.

Observed on an MI355X (appended to the parity log by every run).  (b), largest error over its bound per column, the
largest over tile 8 / 16 / 32:
  randn (exponents 33, 30)   .39 .37 .35 .41 .41 .49 .23 .27 .28 .84 .63 .57
  mean  (exponents 51, 66)   .51 .44 .46 .56 .45 .52 .54 .54 .54 .56 .55 .57
  hdr   (exponents 34, 32)   .75 .81 .88 .98 .99 .97 .94 .79 .94 .18 .98 .57
(hdr: most rows are a few units long and are committed once, P = 1: their error is the rounding of that one commit, up to
u / 2 = the bound), and the largest row error against the float64 rows, of the column's largest entry: 9.7e-6 (hdr,
column 1), 2.2e-6 (randn, column 0), 8.7e-7 (mean, column 4).  (c), largest row error of the largest gradient:
d gaussians2d 1.3e-6 / 2.2e-7 / 3.0e-6 (randn / mean / hdr), d features 9.0e-8 / 8.7e-8 / 1.7e-7, heuristics
1.2e-7 / 2.8e-7 / 5.7e-8, visibility 1.2e-7; the SH frame 8.5e-7 and 1.9e-7.  (e) 3.5e-7 / 3.6e-7 / 4.5e-7.  (f), with
the ranged units: 2.7e-8 .. 1.1e-7; with the units of ``ms_fixed_point_exponents`` the three non-control cases wrap."""
import functools
import math

import numpy as np
import pytest
import torch

from oracle import mapper as omap, projection as oproj, raster as orast
from oracle.gate_excess import _record, check_pixels
from taichi_splatting_amd import RasterConfig, _lib, frame, map_to_tiles, rasterize_with_tiles, render_gaussians
from taichi_splatting_amd.rasterizer import function as raster_function

from . import moments_oracle as mo
from . import threshold_cases as tc
from .test_gpu_raster import gate_stable
from .test_gpu_round6 import SEG_SIZES, cfg_for, confined_scene, lists_for, report_rows, split_forward_backward

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
G_KINDS = ('randn', 'mean', 'hdr')


def grad_images(size, kind):
  """(H, W, 3) float32 on the CPU: a dL/dimage of kind 'randn', 'mean' or 'hdr' (module docstring)"""
  w, h = size
  if kind == 'randn':
    return tc.grad_image(size, 3).float()
  if kind == 'mean':
    return torch.full((h, w, 3), 1.0 / (h * w * 3), dtype=torch.float32)
  G = tc.grad_image(size, 3, seed=1).float() * 2.0 ** -30
  y, x = h // 2 + 3, w // 3 + 1                                     # (not aligned to a patch)
  G[y:y + 4, x:x + 4] = tc.grad_image((4, 4), 3, seed=2).float()
  return G


@functools.lru_cache(maxsize=None)
def scene(tile):
  """scene A, gate-stable, with heuristics and visibility on: (cfg, p, f, o2p, ranges, image of the GPU forward, its
  visibility)"""
  cfg = cfg_for(tile, compute_point_heuristic=True, compute_visibility=True)
  g = gate_stable(tc.scene_a('default'), tc.SIZE_A, cfg)
  p, f, o2p, ranges = lists_for(g, tc.SIZE_A, cfg)
  with torch.no_grad():
    out = rasterize_with_tiles(p, f, o2p, ranges, tc.SIZE_A, cfg)
  return cfg, p, f, o2p, ranges, out.image.contiguous(), out.visibility


@functools.lru_cache(maxsize=None)
def oracle(tile, kind):
  """float64, on the GPU mapper's lists: (image, alpha, visibility, grad_points, grad_features, heuristics), (M, A, P)"""
  cfg, p, f, o2p, ranges, _, _ = scene(tile)
  p64, f64, G = p.cpu().double(), f.cpu().double(), grad_images(tc.SIZE_A, kind).double()
  image, alpha, vis = orast.forward(p64, f64, ranges.cpu(), o2p.cpu(), tc.SIZE_A, cfg)
  gp, gf, heur = orast.backward(p64, f64, ranges.cpu(), o2p.cpu(), image, G, tc.SIZE_A, cfg)
  M, A, P, _ = mo.moment_rows(p64, f64, ranges, o2p, image, G, tc.SIZE_A, cfg)
  return (image, alpha, vis, gp, gf, heur), (M, A, P)


def ranged_exponents(G, p, f, size, cfg):
  return _lib.fixed_point_exponents_ranged(G, p, f, size[0] * size[1], cfg.alpha_threshold)


def raw_rows(p, f, o2p, ranges, image, G, size, cfg, deterministic, fixed_exp=None):
  """ms_raster_bwd_moments: the (V, 12) rows as they are committed, float32 or int64"""
  lib, (w, h) = _lib.load(), size
  mom = torch.zeros((p.shape[0], _lib.MOMENT_ROW), dtype=torch.int64 if deterministic else torch.float32, device=DEV)
  _lib.check(lib.ms_raster_bwd_moments(p.data_ptr(), f.data_ptr(), ranges.data_ptr(), o2p.data_ptr(), image.data_ptr(),
                                       G.data_ptr(), w, h, _lib.raster_config_c(cfg), mom.data_ptr(), deterministic,
                                       _lib.ptr(fixed_exp), 0, (h + cfg.tile_size - 1) // cfg.tile_size,
                                       _lib.current_stream(torch.device(DEV))), "raster backward (moments)")
  return mom[:, :12].cpu()


# ---- a. the exponent kernels, exact ---------------------------------------------------------------------------------------
def amax_values():
  vals = [0.0, 2.0 ** -149, 0.75, math.inf, math.nan]
  for k in (-70, -33, -32, -1, 0, 1, 40, 70):
    vals += [2.0 ** k, float(torch.nextafter(torch.tensor(2.0 ** k, dtype=torch.float32), torch.tensor(0.0)))]
  return vals


RANGED_LAUNCHES = [                                      # (max |feature|, smallest sigma, pixels, alpha_threshold)
  (1.0, 1.5, 150 * 100, 1 / 255.), (0.999, 0.7, 150 * 100, 0.02), (4000.0, 2.0, 256 * 256, 1 / 255.),
  (100.0, 2.0, 256 * 256, 1 / 255.), (16.0, 0.55, 4096 * 4096, 1 / 255.), (2.0, 0.3, 4096 * 4096 + 1, 1e-4),
  (0.0, 1.0, 1, 0.5), (3e-5, 0.01, 1 << 31, 1 / 256.), (math.inf, 1.0, 1000, 1 / 255.), (math.nan, math.inf, 1000, 0.05),
  (1.0, 0.0, 0, 0.0), (1.0, 2.0 ** -140, 640 * 480, 1.0), (3.0e38, 1e30, 7, 2.0),
]


def test_exponent_kernels_equal_their_frexp_mirror():
  lib, stream = _lib.load(), _lib.current_stream(torch.device(DEV))
  out = torch.zeros((2,), dtype=torch.int32, device=DEV)
  checked = 0
  for amax in amax_values():
    a = torch.tensor([amax], dtype=torch.float32, device=DEV)
    _lib.check(lib.ms_fixed_point_exponents(a.data_ptr(), out.data_ptr(), stream), "exponents")
    assert tuple(out.tolist()) == mo.exponents(amax), (amax, out.tolist(), mo.exponents(amax))
    for fmax, smin, pixels, thr in RANGED_LAUNCHES:
      stats = torch.tensor([amax, fmax, smin], dtype=torch.float32, device=DEV)
      _lib.check(lib.ms_fixed_point_exponents_ranged(stats.data_ptr(), pixels, thr, out.data_ptr(), stream), "ranged exponents")
      want = mo.exponents_ranged(amax, fmax, smin, pixels, thr)
      assert tuple(out.tolist()) == want, ((amax, fmax, smin, pixels, thr), out.tolist(), want)
      checked += 1
  # the clamps and the range-limited branch are among the cases
  assert mo.exponents(2.0 ** 70)[1] == -100 and mo.exponents(2.0 ** -70)[1] == 100 and mo.exponents(2.0 ** -70)[0] == 100
  assert mo.exponents_ranged(1.0, 4000.0, 2.0, 256 * 256, 1 / 255.) == (26, 13) and mo.exponents_ranged(1.0, 1.0, 1.5, 15000, 1 / 255.) == mo.exponents(1.0)
  assert checked == len(amax_values()) * len(RANGED_LAUNCHES)


def test_python_launch_statistics_reach_the_kernel():
  """``_lib.fixed_point_exponents_ranged`` reduces what the mirror is given: culled rows (NaN sigma, non-finite colours)
  stay out of the statistics"""
  cfg, p, f, _, _, _, _ = scene(16)
  G = grad_images(tc.SIZE_A, 'hdr').to(DEV)
  p2, f2 = p.clone(), f.clone() * 37.0
  p2[5, 4:6] = float('nan'); p2[6, 4] = 0.0; f2[5] = float('inf'); f2[7, 1] = float('nan')
  got = tuple(ranged_exponents(G, p2, f2, (4096, 4096), cfg).tolist())
  amax, fmax, smin = mo.launch_stats(p2.cpu(), f2.cpu(), G.cpu())
  assert math.isfinite(fmax) and fmax > 30 and 0 < smin < math.inf
  assert got == mo.exponents_ranged(amax, fmax, smin, 4096 * 4096, cfg.alpha_threshold) and got != mo.exponents(amax)


# ---- b. deterministic rows against float-atomic rows, derived bound ---------------------------------------------------------
@pytest.mark.parametrize('kind', G_KINDS)
@pytest.mark.parametrize('tile', [8, 16, 32])
def test_fixed_point_rows_against_float_rows_within_the_derived_bound(tile, kind):
  cfg, p, f, o2p, ranges, image, _ = scene(tile)
  _, (M, A, P) = oracle(tile, kind)
  G = grad_images(tc.SIZE_A, kind).to(DEV).contiguous()
  exps = ranged_exponents(G, p, f, tc.SIZE_A, cfg)
  e_main, e_h0 = exps.tolist()
  assert (e_main, e_h0) == mo.exponents_ranged(*mo.launch_stats(p.cpu(), f.cpu(), G.cpu()), tc.SIZE_A[0] * tc.SIZE_A[1], cfg.alpha_threshold)
  rows_f = raw_rows(p, f, o2p, ranges, image, G, tc.SIZE_A, cfg, 0).double()
  rows_i = raw_rows(p, f, o2p, ranges, image, G, tc.SIZE_A, cfg, 1, exps)
  assert int(rows_i.abs().max()) < 2 ** 53 and int(rows_i.abs().max()) > 2 ** 30          # exact as float64; a real sum
  u = mo.column_units(e_main, e_h0)
  err = (rows_i.double() * u[None] - rows_f).abs()
  Pd = P.double()[:, None]
  bound = Pd * u[None] / 2 + 1.01 * Pd * 2.0 ** -24 * A
  ratio = torch.where(bound > 0, err / bound.clamp_min(1e-300), torch.where(err > 0, torch.full_like(err, math.inf), torch.zeros_like(err)))
  row_err = (rows_i.double() * u[None] - M).abs() / M.abs().max(dim=0).values[None]
  entry = {"what": f"fixed-point rows vs float rows, tile {tile}, {kind} dL/dimage", "kind": "rows vs derived bound",
           "exponents": [e_main, e_h0], "largest_error_over_bound_per_column": [round(float(r), 4) for r in ratio.max(dim=0).values],
           "largest_row_error_vs_oracle_per_column": [float(f"{float(r):.3e}") for r in row_err.max(dim=0).values]}
  _record(entry)
  worst = torch.nonzero(ratio > 1.0)
  assert worst.numel() == 0, (entry, [(int(i), int(c), float(err[i, c]), float(bound[i, c])) for i, c in worst[:8]])


# ---- c. finalised outputs against the float64 oracle ----------------------------------------------------------------------
@pytest.mark.parametrize('kind', G_KINDS)
def test_deterministic_rasterize_against_the_oracle(kind, monkeypatch):
  tile = 16
  cfg, p, f, o2p, ranges, _, _ = scene(tile)
  (image_o, alpha_o, vis_o, gp_o, gf_o, heur_o), _ = oracle(tile, kind)
  G = grad_images(tc.SIZE_A, kind).to(DEV)
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)
  pg, fg = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
  out = rasterize_with_tiles(pg, fg, o2p, ranges, tc.SIZE_A, cfg)
  (out.image * G).sum().backward()
  what = f"deterministic rasterize, {kind} dL/dimage"
  flag, _, count = orast.near_gate(p.cpu().double(), ranges.cpu(), o2p.cpu(), tc.SIZE_A, cfg, 1e-5, return_counts=True)
  err = torch.maximum((out.image.detach().cpu().double() - image_o).abs().max(-1).values,
                      (out.image_weight.detach().cpu().double() - alpha_o).abs())
  check_pixels(err, flag, count, float(f.abs().max()), cfg.alpha_threshold, what, max_fraction=0.0)
  report_rows(what + " d gaussians2d", pg.grad, gp_o, p, ranges, o2p, tc.SIZE_A, cfg)
  report_rows(what + " d features", fg.grad, gf_o, p, ranges, o2p, tc.SIZE_A, cfg)
  report_rows(what + " heuristics", out.point_heuristic, heur_o, p, ranges, o2p, tc.SIZE_A, cfg)
  report_rows(what + " visibility", out.visibility.reshape(-1, 1), vis_o.reshape(-1, 1), p, ranges, o2p, tc.SIZE_A, cfg)


FRAME_SIZE = (128, 128)


@functools.lru_cache(maxsize=None)
def frame_scene():
  from .test_gpu_gaussian_bwd import _frame_scene
  return _frame_scene(3)


def frame_grad_image(kind='hdr'):
  return grad_images(FRAME_SIZE, kind)


def run_frame(G, cfg, vis_from_backward):
  """One SH frame with loss sum(image G) in deterministic mode: (leaves with .grad, rendering, full-size point outputs or
  None).  ``vis_from_backward``: the frame's visibility is column 11 of the rows (frame.VISIBILITY_FROM_BACKWARD); its
  points are then not looked at before the backward pass (that would compute the forward's visibility on demand), so the
  2D gradients are those of a frame without it."""
  g, cam = frame_scene()
  frame.release_caches()
  gd, cam_d = g.to(DEV).requires_grad_(True), cam.to(device=DEV)
  keep = frame.VISIBILITY_FROM_BACKWARD, raster_function.DETERMINISTIC_BACKWARD
  frame.VISIBILITY_FROM_BACKWARD, raster_function.DETERMINISTIC_BACKWARD = vis_from_backward, True
  try:
    r = render_gaussians(gd, cam_d, cfg, use_sh=True)
    if not vis_from_backward:
      r.points.gaussians2d.retain_grad()
      r.points.features.retain_grad()
    (r.image * G.to(DEV)).sum().backward()
    outs = None
    if vis_from_backward:
      outs = {k: v.detach().clone() for k, v in frame.point_outputs(r).items()}
    torch.cuda.synchronize()
  finally:
    frame.VISIBILITY_FROM_BACKWARD, raster_function.DETERMINISTIC_BACKWARD = keep
  return gd, r, outs


def test_deterministic_frame_against_the_oracle():
  """render_gaussians, SH degree 3, heuristics and visibility from the backward pass (column 11), the dL/dimage with 30 bits
  of dynamic range: the 2D gradients, heuristics and visibility against the oracle rasterizer on the kernels' own splats,
  the five leaves as test_moment_rows_frame_matches_oracle holds them"""
  from .test_gpu_configs import LEAVES, oracle_leaf_grads, oracle_leaf_grads_from_covariance
  from .test_gpu_projection_sh import assert_f32_gradient_as_accurate_as_reference
  cfg = RasterConfig(tile_size=16, pixel_stride=(2, 2), compute_point_heuristic=True, compute_visibility=True)
  g, cam = frame_scene()
  G = frame_grad_image()
  gd, r, _ = run_frame(G, cfg, False)
  size = cam.image_size
  idx = r.points.idx.cpu()
  p_h, f_h = r.points.gaussians2d.detach().cpu().double(), r.points.features.detach().cpu().double()
  ndc = oproj.ndc_depth(r.points.depths.detach().cpu().double(), *cam.depth_range)
  o2p_h, ranges_h = omap.map_to_tiles(p_h.numpy().astype(np.float32), ndc.numpy().astype(np.float32), size, cfg.tile_size,
                                      cfg.alpha_threshold)[:2]
  o2p_h, ranges_h = torch.from_numpy(o2p_h), torch.from_numpy(ranges_h).reshape(-1, 2)
  assert float(orast.gate_margin(p_h, ranges_h, o2p_h, size, cfg).min()) > 1e-4
  img_h, alpha_h, _ = orast.forward(p_h, f_h, ranges_h, o2p_h, size, cfg)
  gp_h, gf_h, heur_h = orast.backward(p_h, f_h, ranges_h, o2p_h, img_h, G.double(), size, cfg)
  act_h = orast.active_visibility(p_h, ranges_h, o2p_h, size, cfg)
  what = "deterministic frame, hdr dL/dimage"
  image_k = r.image.detach().clone()
  err = (image_k.cpu().double() - img_h).abs().max(-1).values
  check_pixels(err, torch.zeros_like(err, dtype=torch.bool), None, float(f_h.abs().max()), cfg.alpha_threshold, what, max_fraction=0.0)
  gp_k, gf_k = r.points.gaussians2d.grad.clone(), r.points.features.grad.clone()
  heur_k = torch.stack([r.points.prune_cost, r.points.split_score], dim=1).clone()
  leaves_k = [getattr(gd, k).grad.clone() for k in LEAVES]
  args = (p_h, ranges_h, o2p_h, size, cfg)
  report_rows(what + " d gaussians2d", gp_k, gp_h, *args)
  report_rows(what + " d features", gf_k, gf_h, *args)
  report_rows(what + " heuristics", heur_k, heur_h, *args)
  # the frame whose visibility is column 11: same image, bit for bit the same leaves, the same heuristics at full size
  gd_b, r_b, outs = run_frame(G, cfg, True)
  assert torch.equal(r_b.image, image_k) and torch.equal(r_b.points.idx.cpu(), idx)
  for k, want in zip(LEAVES, leaves_k):
    assert torch.equal(getattr(gd_b, k).grad, want), k
  report_rows(what + " heuristics (full size)", outs['point_heuristic'][idx.to(DEV)], heur_h, *args)
  report_rows(what + " visibility (backward pass)", outs['visibility'][idx.to(DEV)].reshape(-1, 1), act_h.reshape(-1, 1), *args)
  idx64, ref64 = oracle_leaf_grads_from_covariance(g, cam, cfg, p_h, gp_h, gf_h)
  idx32, ref32 = oracle_leaf_grads(g, cam, cfg, gp_k.cpu().double(), gf_k.cpu().double(), torch.float32)
  assert torch.equal(idx64, idx) and torch.equal(idx32, idx)
  for k, w64, w32 in zip(LEAVES, ref64, ref32):
    assert_f32_gradient_as_accurate_as_reference(leaves_k[LEAVES.index(k)].cpu(), w64, w32, (what, k))


# ---- d. power-of-two scale equivariance, bit for bit ----------------------------------------------------------------------
SCALES = (-40, -13, 13, 40)


def test_deterministic_rasterize_is_equivariant_to_powers_of_two(monkeypatch):
  cfg, p, f, o2p, ranges, _, _ = scene(16)
  G = grad_images(tc.SIZE_A, 'randn').to(DEV)
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)

  def run(k):
    pg, fg = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out = rasterize_with_tiles(pg, fg, o2p, ranges, tc.SIZE_A, cfg)
    (out.image * (G * 2.0 ** k)).sum().backward()
    return pg.grad, fg.grad, out.point_heuristic[:, 1].clone(), out.point_heuristic[:, 0].clone()
  base = run(0)
  assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in base)
  for k in SCALES:
    got = run(k)
    for name, a, b in zip(('d gaussians2d', 'd features', 'split_score'), got, base):
      assert torch.equal(a, b * 2.0 ** k), (k, name, float((a - b * 2.0 ** k).abs().max() / (b.abs().max() * 2.0 ** k)))
    if abs(k) == 13:
      assert torch.equal(got[3], base[3] * 4.0 ** k), (k, 'prune_cost')


def test_deterministic_frame_is_equivariant_to_powers_of_two():
  from .test_gpu_configs import LEAVES
  cfg = RasterConfig(tile_size=16, pixel_stride=(2, 2), compute_point_heuristic=True, compute_visibility=True)
  G = frame_grad_image('randn')

  def run(k):
    gd, r, outs = run_frame(G * 2.0 ** k, cfg, True)
    return [getattr(gd, name).grad.clone() for name in LEAVES] + [outs['point_heuristic'][:, 1], outs['point_heuristic'][:, 0], outs['visibility']]
  base = run(0)
  assert all(bool(torch.isfinite(t).all()) and float(t.abs().max()) > 0 for t in base)
  for k in SCALES:
    got = run(k)
    for name, a, b in zip(LEAVES + ('split_score',), got, base):
      assert torch.equal(a, b * 2.0 ** k), (k, name, float((a - b * 2.0 ** k).abs().max() / (b.abs().max() * 2.0 ** k)))
    if abs(k) == 13:
      assert torch.equal(got[6], base[6] * 4.0 ** k), (k, 'prune_cost')
    assert torch.equal(got[7], base[7]), (k, 'visibility')


# ---- e. segments in deterministic mode ------------------------------------------------------------------------------------
def test_segment_kernels_with_deterministic_commits():
  """test_segment_kernels_vs_oracle's tile-16 scene with heuristics on: ms_raster_bwd_moments_split with deterministic = 1"""
  lib, tile = _lib.load(), 16
  size = SEG_SIZES[tile]
  g = confined_scene(1400, size, tile, seed=60 + tile, inset=4.0, alpha_range=(0.01, 0.03))
  cfg = cfg_for(tile, compute_point_heuristic=True)
  p, f, o2p, ranges = lists_for(g, size, cfg)
  torch.manual_seed(1)
  G = (torch.rand(size[1], size[0], 3, device=DEV) + 0.5).contiguous()
  exps = ranged_exponents(G, p, f, size, cfg)
  rows, outs = [], []
  for _ in range(2):
    outs.append(split_forward_backward(lib, p, f, o2p, ranges, size, cfg, G, 512, 512, deterministic=1, fixed_exp=exps, rows_out=rows))
  counts = outs[0][6]
  assert int(counts[2]) == 0 and int(counts[1]) == ranges.shape[0] and int(counts[0]) >= 3 * int(counts[1]), counts[:3]
  assert rows[0].dtype == torch.int64 and torch.equal(rows[0], rows[1]) and int(rows[0].abs().max()) > 2 ** 30
  for a, b in zip(outs[0][3:6], outs[1][3:6]):
    assert torch.equal(a, b)
  img_o, _, _ = orast.forward(p.cpu().double(), f.cpu().double(), ranges.cpu(), o2p.cpu(), size, cfg)
  gp_o, gf_o, heur_o = orast.backward(p.cpu().double(), f.cpu().double(), ranges.cpu(), o2p.cpu(), img_o, G.cpu().double(), size, cfg)
  _, _, _, gp, gf, heur, _ = outs[0]
  what = "segments tile 16, deterministic"
  report_rows(what + " d gaussians2d", gp, gp_o, p, ranges, o2p, size, cfg)
  report_rows(what + " d features", gf, gf_o, p, ranges, o2p, size, cfg)
  report_rows(what + " heuristics", heur, heur_o, p, ranges, o2p, size, cfg)


# ---- f. headroom ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('case', list(mo.HEADROOM_CASES))
def test_rows_of_a_background_splat_with_large_colours_do_not_wrap(case, monkeypatch):
  colour, alpha, g_value, column = mo.HEADROOM_CASES[case]
  size = mo.HEADROOM_SIZE
  cfg = cfg_for(16, compute_point_heuristic=True)
  p, f, depth = (t.to(DEV).contiguous() for t in mo.headroom_scene(colour, alpha))
  o2p, ranges = map_to_tiles(p, depth.reshape(-1, 1), size, cfg)
  ranges = ranges.view(-1, 2).contiguous()
  p64, f64 = p.cpu().double(), f.cpu().double()
  assert float(orast.gate_margin(p64, ranges.cpu(), o2p.cpu(), size, cfg).min()) >= 1e-4
  G = torch.full((size[1], size[0], 3), g_value, device=DEV)
  img_o, _, _ = orast.forward(p64, f64, ranges.cpu(), o2p.cpu(), size, cfg)
  gp_o, gf_o, heur_o = orast.backward(p64, f64, ranges.cpu(), o2p.cpu(), img_o, G.cpu().double(), size, cfg)
  # the case tests something: in the units of ms_fixed_point_exponents its column passes 2^63
  M, _, _, _ = mo.moment_rows(p64, f64, ranges, o2p, img_o, G.cpu().double(), size, cfg)
  old_units = M.abs() / mo.column_units(*mo.exponents(abs(g_value)))
  if column is not None:
    assert float(old_units[:, column].max()) > 2.0 ** 63, (case, math.log2(float(old_units[:, column].max())))
  else:
    assert float(old_units.max()) < 2.0 ** 62

  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)

  def run():
    pg, fg = p.clone().requires_grad_(True), f.clone().requires_grad_(True)
    out = rasterize_with_tiles(pg, fg, o2p, ranges, size, cfg)
    (out.image * G).sum().backward()
    return pg.grad, fg.grad, out.point_heuristic.clone()
  first, second = run(), run()
  for a, b in zip(first, second):
    assert torch.equal(a, b)
  what = f"headroom {case}"
  report_rows(what + " d gaussians2d", first[0], gp_o, p, ranges, o2p, size, cfg)
  report_rows(what + " d features", first[1], gf_o, p, ranges, o2p, size, cfg)
  report_rows(what + " heuristics", first[2], heur_o, p, ranges, o2p, size, cfg)
