"""-m gpu: the raster, mapper and frame kernels at NON-DEFAULT blend thresholds (alpha_threshold, clamp_max_alpha,
saturate_threshold; clamp_margin and blur_cov in the 3D cases) against the float64 oracle.  The product kernels fold
these scalars into derived constants (csrc/raster_fast.hip: GATE, TSCALE, the exponent bias of the clamp; the cull
rectangles of write_records / make_scan_record; one_minus_saturate and the three levels of saturation early-out of
csrc/raster_bwd_scan.hip; obb_grid_query of csrc/mapper.hip; the frustum cull of csrc/splat_math.h), and at the default
config none of the foldings can be told from a wrong one: the clamp never engages, and a (pixel, splat) pair dropped for
saturation carries a weight of the size of the tolerance.

Configs, scene A and the two oracle-only conditions each case starts from are in tests/threshold_cases.py: the oracle at
the case's config differs from the oracle at the default config on at least 10 % of rows (the case tests something), and
at most 2 % of gradient rows have a pair within 1e-4 of the backward's saturation limit.  Those flagged rows are held,
element by element, to the interval between the oracle backward at limit (1 -+ 1e-4); every other row, and every pixel, to
the project's tolerances: float64 those of test_forward_backward_f64, float32 1e-4 absolute on pixels and 1e-4 of the
largest gradient on rows (BASELINE north star).  Scenes are gate-stable (test_gpu_raster.gate_stable at the case's
alpha_threshold).  Rows are listed through test_gpu_round6.report_rows into the parity log.

Observed on an MI355X, from the parity log (float32 cases; the largest pixel error of image and weight, absolute; the
largest row error of gradients, heuristics and visibility as a share of the largest entry; flagged rows.  The
deterministic backward gives the same figures to two digits):

  case                         pixels    rows      flagged rows
  2  T_hi    tile 16           3.5e-07   1.1e-06   -
  2  T_lo    tile 16           6.5e-07   1.5e-06   -
  2  C_half  tile 16           5.3e-07   7.4e-07   -
  2  C_80    tile 16           5.8e-07   1.5e-06   -
  2  S_half  tile 16           5.0e-07   1.2e-06   24 of 2966 (0.81 %)
  2  S_90    tile 16           5.0e-07   1.3e-06   34 of 2966 (1.15 %)
  2  ALL     tile 8 / 16 / 32  4.6e-07   8.7e-07   6 of 2971 (0.20 %)
  3  T_hi    antialias         4.2e-07   9.7e-07   -
  3  T_lo    antialias         6.6e-07   2.2e-06   -          (before the fix below: 4.8e-05, 1.3e-04 — failing)
  3  ALL     antialias         4.9e-07   9.4e-07   11 of 2982 (0.37 %)
  4  ALL     5 channels        4.6e-07   6.7e-07   6 of 2971 (0.20 %)
  5  S_half  segments 16 / 32  3.3e-07   7.5e-07   13 of 16800 (0.08 %) / 6 of 8400 (0.07 %)
  5  ALL     segments 16 / 32  5.2e-07   1.4e-06   2 of 16800 (0.01 %) / 1 of 8400 (0.01 %)
  6  ALL     splat rows        4.4e-07   6.8e-07   6 of 2971 (0.20 %)
  8  render, float32 forward   6.4e-06   -         -

No flagged row left its interval by more than 2e-5, no row of any case went beyond 2e-5: away from the defaults the 1e-4
contract has the same two orders of magnitude of room as at them.  Cases 1, 7, 8 (float64, both paths), 9, 10 and 11
passed at their exact or float64 tolerances: the 1/255 written out in csrc/gaussian_bwd.hip and csrc/projection.hip is
harmless (the backward passes never cull), and a shape record shared across alpha_thresholds re-runs the emission when
the learnt capacity (65 536) does not hold the other threshold's lists (70 447 overlaps) and reports no overflow.

The one finding: the float antialiased pdf of csrc/raster.hip took S(hi) - S(lo) of two sigmoids that are both
1 - O(alpha_threshold) in a splat's tail; the rounded difference was good to ~1e-7 / (S(hi) - S(lo)) only, 2e-2 relative
at alpha_threshold 1e-4 (1e-4 at 0.02 and 5e-5 at 0.05 in a float32 emulation on scene A: no deeper than the gate margin
of the scenes, which is why larger thresholds hid it), and moved (pixel, splat) pairs that are 1e-3 away from the blend
gate across it.  It now differences the exponentials instead (aa_edge_diff: 6e-6 relative).
"""
import functools
from collections import namedtuple

import pytest
import torch

from oracle import mapper as omap, raster as orast
from oracle.gate_excess import _record
from taichi_splatting_amd import RasterConfig, _lib, frame, map_to_tiles, rasterize_with_tiles, render_gaussians
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
from taichi_splatting_amd.rasterizer import function as raster_function
from taichi_splatting_amd.testing import random_2d_gaussians

from . import threshold_cases as tc
from .test_gpu_raster import gate_stable
from .test_gpu_round6 import (SEG_SIZES, TOL, confined_scene, finalize, lists_for, report_rows, split_forward_backward,
                              splat_rows_backward, splat_rows_forward)

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
SIZE = tc.SIZE_A

Reference = namedtuple('Reference', 'cfg p f depth o2p ranges G want saturation')


def saturates(name):
  return 'saturate_threshold' in tc.CONFIGS[name]


def oracle_reference(name, g, size, cfg, sensitive=True):
  """The float64 oracle on the GPU mapper's lists of ``g`` at ``cfg``, after the case's two preconditions (oracle only)"""
  p, f, o2p, ranges = lists_for(g, size, cfg)
  G = tc.grad_image(size, f.shape[1]).float().double()          # (the float32 kernels are given exactly this dL/dimage)
  want = tc.oracle_outputs(p, f, ranges, o2p, size, cfg, G)
  if sensitive:
    d = tc.default_of(cfg)
    _, _, o2p_d, ranges_d = lists_for(g, size, d)
    tc.assert_sensitive(name, want, tc.oracle_outputs(p, f, ranges_d, o2p_d, size, d, G))
  saturation = tc.saturation_rows(p, f, ranges, o2p, size, cfg, want['image'], G) if saturates(name) else None
  depth = g.depths.reshape(-1).to(DEV).contiguous()
  return Reference(cfg, p, f, depth, o2p, ranges, G, want, saturation)


def reference(name, tile=16, antialias=False, channels=3):
  """Scene A, gate-stable at the config, and its oracle: computed once, shared by the cases on the same lists"""
  return _reference(name, tile, antialias, channels)


@functools.lru_cache(maxsize=None)
def _reference(name, tile, antialias, channels):
  cfg = tc.config(name, tile, antialias=antialias, compute_visibility=True, compute_point_heuristic=True)
  g = gate_stable(tc.scene_a(name, channels), SIZE, cfg)
  return oracle_reference(name, g, SIZE, cfg)


def check_pixels(what, got, want, tol=TOL, relative=False):
  """every pixel (entry) within ``tol``, absolute or ``relative`` to the largest entry; the figure goes to the parity log"""
  err = float((got.detach().cpu().double() - want).abs().max()) / (float(want.abs().max()) if relative else 1.0)
  _record({"what": what, "kind": "entries vs oracle, of the largest" if relative else "pixels vs oracle", "largest": err})
  assert err < tol, (what, err)


def check_rows(what, ref, key, got, tol=TOL):
  flagged, interval = None, None
  if ref.saturation is not None:
    flagged, lo, hi = ref.saturation
    interval = (lo[key], hi[key])
  return report_rows(what, got, ref.want[key], ref.p, ref.ranges, ref.o2p, (ref.want['image'].shape[1], ref.want['image'].shape[0]),
                     ref.cfg, tol=tol, flagged=flagged, interval=interval)


def check_f32_outputs(what, ref, image, alpha, vis, gp, gf, heur):
  check_pixels(what + " image", image, ref.want['image'])
  check_pixels(what + " weight", alpha, ref.want['alpha'])
  if vis is not None:
    check_pixels(what + " visibility", vis, ref.want['visibility'], relative=True)
  check_rows(what + " d gaussians2d", ref, 'grad_points', gp)
  check_rows(what + " d features", ref, 'grad_features', gf)
  if heur is not None:
    check_rows(what + " heuristics", ref, 'heuristics', heur)


def rasterize_f32(ref, deterministic=False):
  keep = raster_function.DETERMINISTIC_BACKWARD
  raster_function.DETERMINISTIC_BACKWARD = deterministic
  try:
    pg, fg = ref.p.clone().requires_grad_(True), ref.f.clone().requires_grad_(True)
    out = rasterize_with_tiles(pg, fg, ref.o2p, ref.ranges, SIZE, ref.cfg)
    (out.image * ref.G.to(DEV, torch.float32)).sum().backward()
    torch.cuda.synchronize()
  finally:
    raster_function.DETERMINISTIC_BACKWARD = keep
  return out.image, out.image_weight, out.visibility, pg.grad, fg.grad, out.point_heuristic


# ---- case 1: the generic kernels (csrc/raster.hip) in float64 -------------------------------------------------------
F64_CASES = [(name, 16, False) for name in tc.CONFIGS] + [('ALL', 8, False), ('ALL', 32, False), ('ALL', 16, True)]


@pytest.mark.parametrize('name,tile,antialias', F64_CASES)
def test_generic_f64_vs_oracle(name, tile, antialias):
  """rasterize_with_tiles in float64: image, weight, visibility, gradients and heuristics at test_forward_backward_f64's
  tolerances — every row, flagged or not (a float64 T is within 1e-13 of the oracle's, the flags are 1e-4 wide)."""
  ref = reference(name, tile, antialias)
  want = ref.want
  pg, fg = ref.p.double().requires_grad_(True), ref.f.double().requires_grad_(True)
  out = rasterize_with_tiles(pg, fg, ref.o2p, ref.ranges, SIZE, ref.cfg)
  assert torch.allclose(out.image.cpu(), want['image'], atol=1e-9)
  assert torch.allclose(out.image_weight.cpu(), want['alpha'], atol=1e-9)
  assert torch.allclose(out.visibility.cpu(), want['visibility'], atol=1e-8)
  (out.image * ref.G.to(DEV)).sum().backward()
  gp_o, gf_o, h_o = want['grad_points'], want['grad_features'], want['heuristics']
  scale = max(1.0, gp_o.abs().max().item())
  assert torch.allclose(pg.grad.cpu(), gp_o, atol=1e-8 * scale, rtol=1e-7), (pg.grad.cpu() - gp_o).abs().max()
  assert torch.allclose(fg.grad.cpu(), gf_o, atol=1e-9, rtol=1e-7), (fg.grad.cpu() - gf_o).abs().max()
  assert torch.allclose(out.point_heuristic.cpu(), h_o, atol=1e-7 * max(1.0, h_o.abs().max().item()), rtol=1e-6)


# ---- case 2: the float32 RGB product kernels (csrc/raster_fast.hip forward, csrc/raster_bwd_scan.hip backward) ------
F32_CASES = [(name, 16) for name in tc.CONFIGS] + [('ALL', 8), ('ALL', 32)]


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('name,tile', F32_CASES)
def test_product_f32_rgb_vs_oracle(name, tile, deterministic):
  ref = reference(name, tile)
  what = f"thresholds {name} tile {tile}{' deterministic' if deterministic else ''}"
  check_f32_outputs(what, ref, *rasterize_f32(ref, deterministic))


# ---- case 3: float32 RGB with the antialiased pdf (pixel-per-lane backward, antialias cull of stage_batch) ----------
@pytest.mark.parametrize('name', ['T_hi', 'T_lo', 'ALL'])
def test_f32_antialias_vs_oracle(name):
  ref = reference(name, 16, True)
  check_f32_outputs(f"thresholds {name} antialias", ref, *rasterize_f32(ref))


# ---- case 4: float32, five channels (the generic float instantiation, channel chunks) -------------------------------
def test_f32_five_channels_vs_oracle():
  ref = reference('ALL', 16, False, 5)
  check_f32_outputs("thresholds ALL 5 channels", ref, *rasterize_f32(ref))


# ---- case 5: the segment kernels: start states composed across segments ---------------------------------------------
SEGMENT_ALPHA = {('S_half', 16): (0.01, 0.03), ('S_half', 32): (0.05, 0.12), ('ALL', 16): (0.03, 0.09), ('ALL', 32): (0.1, 0.25)}


@pytest.mark.parametrize('name,tile', list(SEGMENT_ALPHA))
def test_segment_kernels_vs_oracle(name, tile):
  """Tile lists of 1400 splats cut into three segments of 512 (test_gpu_round6.test_segment_kernels_vs_oracle) with
  opacities chosen so that, by the oracle, pixels first reach saturate_threshold BEHIND entry 512 of their list: the
  backward of the second and third segment starts from the composed transmittance and has to find the saturation limit
  from there; a limit crossed inside the first segment only would say nothing about the composed states."""
  lib = _lib.load()
  size = SEG_SIZES[tile]
  cfg = tc.config(name, tile, compute_visibility=True, compute_point_heuristic=True)
  g = confined_scene(1400, size, tile, seed=60 + tile, alpha_range=SEGMENT_ALPHA[name, tile], cfg=cfg)
  ref = oracle_reference(name, g, size, cfg)
  runs = ref.ranges[:, 1] - ref.ranges[:, 0]
  assert int(runs.min()) > 1024 and int(runs.max()) < 16384
  first = tc.first_saturated_entry(ref.p, ref.ranges, ref.o2p, size, cfg)
  behind = float((first >= 512).double().mean())
  print(f"segments {name} tile {tile}: {behind:.1%} of pixels saturate behind entry 512, {float((first >= 1024).double().mean()):.1%} behind 1024")
  assert behind > 0.02
  G = ref.G.to(DEV, torch.float32).contiguous()
  image, alpha, vis, gp, gf, heur, counts = split_forward_backward(lib, ref.p, ref.f, ref.o2p, ref.ranges, size, cfg, G, 512, 512)
  assert int(counts[2]) == 0 and int(counts[1]) == ref.ranges.shape[0] and int(counts[0]) >= 3 * int(counts[1]), counts[:3]
  check_f32_outputs(f"thresholds {name} segments tile {tile}", ref, image, alpha, vis, gp, gf, heur)


# ---- case 6: the splat-row entry points -------------------------------------------------------------------------------
def test_splat_row_entry_points_vs_oracle():
  lib = _lib.load()
  ref = reference('ALL')
  rows, image, alpha, vis = splat_rows_forward(lib, ref.p, ref.depth, ref.f, ref.o2p, ref.ranges, SIZE, ref.cfg)
  G = ref.G.to(DEV, torch.float32).contiguous()
  rc, mom = splat_rows_backward(lib, rows, ref.o2p, ref.ranges, image, G, SIZE, ref.cfg)
  _lib.check(rc, "bwd rows")
  gp, gf, heur = finalize(lib, ref.p, mom, True, _lib.current_stream(torch.device(DEV)))
  check_f32_outputs("thresholds ALL splat rows", ref, image, alpha, vis, gp, gf, heur)


# ---- case 7: the mapper ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('alpha_threshold', [0.05, 1e-4, 0.5])
@pytest.mark.parametrize('n,size,scale', [(1000, (320, 200), 0.5), (20000, (333, 210), 2.0)])
def test_mapper_vs_oracle(n, size, scale, alpha_threshold):
  """Both mapper sequences against the oracle mapper (test_gpu_mapper._check: identical lists, borderline pairs apart)
  with opacities over (0, 1): 0.5 culls half of the splats outright."""
  from .test_gpu_mapper import _check
  torch.manual_seed(n)
  g = random_2d_gaussians(n, size, scale_factor=scale, alpha_range=(0.0, 1.0), depth_range=(0.1, 100.0))
  p = project_gaussians2d(g)
  cfg = RasterConfig(alpha_threshold=alpha_threshold)
  count = lambda t: omap.map_to_tiles(p.numpy(), g.depths.numpy(), size, cfg.tile_size, t)
  k_case, k_default = count(alpha_threshold)[0].shape[0], count(RasterConfig().alpha_threshold)[0].shape[0]
  assert abs(k_case - k_default) > 0.25 * k_default, (k_case, k_default)        # the threshold reaches the lists
  if alpha_threshold == 0.5:
    listed = int((count(alpha_threshold)[2] > 0).sum())
    assert 0.4 * n < listed < 0.6 * n, listed
  _check(p, g.depths, size, cfg)


# ---- case 8: render_gaussians on a 3D scene -------------------------------------------------------------------------------
def render_config(**kw):
  return RasterConfig(**tc.CONFIGS['ALL'], clamp_margin=0.3, blur_cov=0.1, **kw)


def render_scene(dtype, alpha_range=(0.3, 1.0)):
  from .test_gpu_render import make_scene
  return make_scene(4000, (200, 120), seed=4, sh_degree=1, dtype=dtype, margin=0.6, alpha_range=alpha_range)


@functools.lru_cache(maxsize=None)
def render_reference():
  from .test_gpu_render import oracle_forward, oracle_render_with_grads
  size = (200, 120)
  g, cam = render_scene(torch.float64)
  cfg = render_config()
  torch.manual_seed(1)
  G = torch.randn(size[1], size[0], 3, dtype=torch.float64)
  image, alpha, idx, grads = oracle_render_with_grads(g, cam, cfg, True, G)
  assert 0.3 * 4000 < idx.shape[0] < 0.9 * 4000, idx.shape        # the frustum cull is active
  # the configured values reach the image and the visible set
  d = RasterConfig()
  default = oracle_forward(g, cam, d, True, blur_cov=d.blur_cov, clamp_margin=d.clamp_margin)
  share = tc.differing_rows(image, default['image'])
  print(f"render: the oracle image differs from the default config's on {share:.1%} of pixels; visible "
        f"{idx.shape[0]} against {default['indexes'].shape[0]}")
  assert share >= tc.SENSITIVE_ROWS and idx.shape[0] != default['indexes'].shape[0]
  return g, cam, cfg, G, image, alpha, idx, grads


@pytest.mark.parametrize('use_frame', [True, False])
def test_render_f64_vs_oracle(use_frame):
  """The frame executor and the modular operators in float64 against the oracle pipeline at test_gpu_render's tolerances:
  the visible set (frustum cull at the configured alpha_threshold), image, weight and all five leaf gradients — the
  per-gaussian backward passes re-project with alpha_threshold = 1/255 written out (csrc/gaussian_bwd.hip,
  csrc/projection.hip): harmless only if the backward never culls."""
  g, cam, cfg, G, image_o, alpha_o, idx_o, grads_o = render_reference()
  keep = frame.USE_FRAME
  frame.USE_FRAME = use_frame
  try:
    gd = g.to(DEV).requires_grad_(True)
    r = render_gaussians(gd, cam.to(device=DEV), cfg, use_sh=True)
    assert torch.equal(r.points.idx.cpu(), idx_o)
    assert torch.allclose(r.image.cpu(), image_o, atol=1e-9)
    assert torch.allclose(r.image_weight.cpu(), alpha_o, atol=1e-9)
    (r.image * G.to(DEV)).sum().backward()
  finally:
    frame.USE_FRAME = keep
  for what, got, want in zip(('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature'),
                             (gd.position.grad, gd.log_scaling.grad, gd.rotation.grad, gd.alpha_logit.grad, gd.feature.grad), grads_o):
    scale = max(1.0, want.abs().max().item())
    assert torch.allclose(got.cpu(), want, atol=1e-7 * scale, rtol=1e-6), (what, (got.cpu() - want).abs().max(), scale)


def test_render_f32_frame_equals_modular():
  from .test_gpu_frame import assert_grads_close, render_both
  g, cam = render_scene(torch.float32)
  g, cam = g.to(DEV), cam.to(device=DEV)
  cfg = render_config()
  torch.manual_seed(0)
  G = torch.randn(120, 200, 3, device=DEV)
  (rf, gf), (rl, gl) = render_both(g, cam, cfg, True, loss=lambda r: (r.image * G).sum())
  assert torch.equal(rf.image, rl.image) and torch.equal(rf.image_weight, rl.image_weight)
  assert torch.equal(rf.points.idx, rl.points.idx) and 0 < rf.points.idx.shape[0] < 4000
  assert torch.equal(rf.points.gaussians2d, rl.points.gaussians2d)
  assert_grads_close(gf, gl, modular_conditioning=True)


def test_render_f32_forward_within_1e4_of_the_oracle():
  """as test_render_f32_within_1e4_config_b_shape: the gaussians with a pair at the blend gate dropped by the float64
  pipeline, then every pixel of the float32 frame within 1e-4"""
  from .test_gpu_render import oracle_forward
  size = (200, 120)
  g, cam = render_scene(torch.float32)
  cfg = render_config()
  kw = dict(blur_cov=cfg.blur_cov, clamp_margin=cfg.clamp_margin)
  o = oracle_forward(g, cam, cfg, True, **kw)
  margin = orast.gate_margin(o['points'].detach(), o['ranges'], o['o2p'], size, cfg)
  keep = torch.ones(4000, dtype=torch.bool)
  keep[o['indexes'][margin < 1e-4]] = False
  assert float(keep.float().mean()) > 0.9
  g = g[keep]
  o = oracle_forward(g, cam, cfg, True, **kw)
  r = render_gaussians(g.to(DEV), cam.to(device=DEV), cfg, use_sh=True)
  assert torch.equal(r.points.idx.cpu(), o['indexes'])
  assert float(o['alpha'].max()) > 0.9
  check_pixels("thresholds render image", r.image, o['image'])
  check_pixels("thresholds render weight", r.image_weight, o['alpha'])


# ---- case 9: the shape record does not know the thresholds ----------------------------------------------------------------
@pytest.mark.parametrize('order', [('T_hi', 'T_lo', 'T_hi'), ('T_lo', 'T_hi', 'T_lo')])
def test_shape_record_across_alpha_thresholds(order):
  """frame._shape_key leaves the thresholds out: frames of one (n, size, tile) at alpha_threshold 0.05 and 1e-4 share a
  shape record, and the capacity learnt at 0.05 (one 65536-entry granule) does not hold the lists at 1e-4.  Each frame's
  image must be the modular path's bit for bit, its overlap total the mapper's, and no overflow may be left standing."""
  from .test_gpu_frame import make_scene
  from taichi_splatting_amd.perspective.projection import project_to_image
  from taichi_splatting_amd.rendering import ndc_depth
  size = (256, 256)
  g, cam = make_scene(16000, size, seed=3)
  totals, capacities = {}, []
  frame.release_caches()
  try:
    for name in order:
      cfg = tc.config(name)
      with torch.no_grad():
        r = render_gaussians(g, cam, cfg, use_sh=False)
        status = frame.frame_status(r)
        frame.USE_FRAME = False
        try:
          want = render_gaussians(g, cam, cfg, use_sh=False)
        finally:
          frame.USE_FRAME = True
        g2d, depths, idx = project_to_image(g, cam, cfg)
        o2p, ranges = map_to_tiles(g2d, ndc_depth(depths, cam.near_plane, cam.far_plane), size, cfg)
      assert torch.equal(r.image, want.image) and torch.equal(r.image_weight, want.image_weight), name
      assert torch.equal(r.points.idx, idx)
      assert float(want.image.max()) > 0.05
      assert status['overlaps'] == o2p.shape[0], (name, status, o2p.shape[0])
      assert not status['overflow'] and status['capacity'] >= status['overlaps'], (name, status)
      totals[name] = status['overlaps']
      capacities.append(status['capacity'])
  finally:
    frame.release_caches()
  # the case is the one it claims to be: the capacity a first frame at 0.05 learns is too small for the lists at 1e-4
  assert frame.round_capacity(totals['T_hi'] * frame.K_SLACK) < totals['T_lo'], totals
  print(f"shape record {order}: overlaps {totals}, capacities {capacities}")


# ---- case 10: median depth ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('use_frame', [True, False])
def test_median_depth_vs_quantile_oracle(use_frame):
  """render_median_depth with median_threshold 0.5 and alpha_threshold 0.02 against the oracle's quantile render of the
  depths; as in test_render_options_median_depth_and_visibility only pixels numerically on the quantile may differ."""
  from .test_gpu_render import make_scene, oracle_forward
  size = (160, 96)
  g, cam = make_scene(3000, size, seed=9)
  cfg = RasterConfig(median_threshold=0.5, alpha_threshold=0.02)
  o = oracle_forward(g, cam, cfg, False)
  quantile = lambda o, c: orast.forward(o['points'].detach(), o['depths'].detach(), o['ranges'], o['o2p'], size,
                                        orast.Cfg(use_alpha_blending=False, saturate_threshold=c.median_threshold,
                                                  alpha_threshold=c.alpha_threshold))[0][..., 0]
  med = quantile(o, cfg)
  d = RasterConfig()
  share = tc.differing_rows(med[..., None], quantile(oracle_forward(g, cam, d, False), d)[..., None])
  assert share >= tc.SENSITIVE_ROWS, share
  keep = frame.USE_FRAME
  frame.USE_FRAME = use_frame
  try:
    r = render_gaussians(g.to(DEV), cam.to(device=DEV), cfg, render_median_depth=True)
  finally:
    frame.USE_FRAME = keep
  assert torch.allclose(r.image.cpu(), o['image'], atol=1e-9)
  mism = (r.median_depth_image.cpu() - med).abs() > 1e-9
  print(f"median depth: {int(mism.sum())} of {mism.numel()} pixels differ; the default config's differs on {share:.1%}")
  assert mism.float().mean() < 1e-3
  assert float(med.max()) > 0


# ---- case 11: strips ------------------------------------------------------------------------------------------------------
def test_cropped_strips_equal_rows_of_full_frame():
  from .test_gpu_strips import check_cropped_strips
  cfg = tc.config('ALL')
  p, f, depths, size = check_cropped_strips(3, torch.float32, cfg)
  # (oracle only: the config reaches this scene's image)
  images = []
  for c in (cfg, tc.default_of(cfg)):
    o2p, ranges, _ = omap.map_to_tiles(p.cpu().numpy(), depths.cpu().numpy(), size, c.tile_size, c.alpha_threshold)
    images.append(orast.forward(p.cpu().double(), f.cpu().double(), torch.from_numpy(ranges), torch.from_numpy(o2p), size, c)[0])
  assert tc.differing_rows(*images) >= tc.SENSITIVE_ROWS
