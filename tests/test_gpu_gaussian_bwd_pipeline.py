"""-m gpu: the staged form of the moment-row kernels of csrc/gaussian_bwd.hip (gaussian_bwd_kernel<float, DEG, true,
FIXED>), reached through whole frames.

These kernels bring full blocks of 64 gaussians in by LDS-DMA, and where the grid-stride loop runs on (camera
gradients cap the grid at 2048 workgroups) one block ahead.  The edges are: a wave's first block (staged before the
loop), a next block that does not exist, the ragged last block (never staged: the lanes load for themselves), a loop
that runs more than once, culled rows and culled whole waves inside staged blocks, and caller tensors the 16-byte DMA
pieces cannot take.

Protocol and tolerances are Part B's of tests/test_gpu_gaussian_bwd.py (``_frame_backward``: the float64 oracle
rasterizer on the kernels' own splats, pushed through the float64 chain as a covariance gradient; criterion
``assert_f32_gradient_as_accurate_as_reference``), imported from there.  The long scene is compared with float64 from
the same inputs — the float64 generic rasterizer on the same splats and tile lists, then the float64 chain: code the
staging does not touch — under ``oracle.gate_excess.check_rows`` with pairs within 1e-5 of the blend gate flagged, the
criterion tests/test_gpu_configs.py applies to that pairing at full size.

The gradient arrays the frame allocates are handed out NaN-filled with a guard row behind them (``nan_guarded``)."""
import functools

import pytest
import torch

from oracle import projection as oproj, sh as osh
from oracle.gate_excess import check_rows
from taichi_splatting_amd import RasterConfig, map_to_tiles, render_gaussians
from taichi_splatting_amd.perspective.projection import project_to_image
from taichi_splatting_amd.rasterizer import function as raster_function
from taichi_splatting_amd.rendering import ndc_depth
from .gaussian_bwd_oracle import sh_features
from .test_gpu_configs import (LEAVES, MAX_ROWS_BEYOND, gate_stable, near_gate_gpu, oracle_leaf_grads,
                               oracle_leaf_grads_from_covariance, scene)
from .test_gpu_gaussian_bwd import DEV, _assert_moments_buffer_clean, _frame_backward
from .test_gpu_projection_sh import assert_f32_gradient_as_accurate_as_reference

pytestmark = pytest.mark.gpu

EDGE_SIZE, EDGE_TILE = (64, 48), 16
EDGE_NS = (1, 63, 64, 65, 255, 256, 257, 513)
POOL_N = 1400


def edge_cfg():
  return RasterConfig(tile_size=EDGE_TILE, pixel_stride=(2, 2))


@functools.lru_cache(maxsize=None)
def pool(degree):
  """gate-stable gaussians on the small image with saturating SH features; the tests take their rows from it"""
  g, cam = scene(POOL_N, EDGE_SIZE, seed=5, sh_degree=max(degree, 0))
  torch.manual_seed(70 + degree)
  g = g.replace(feature=sh_features(POOL_N, 3, degree))
  return gate_stable(g, cam, edge_cfg()), cam


def rows(g, first, n):
  keep = torch.zeros(g.position.shape[0], dtype=torch.bool)
  keep[first:first + n] = True
  return g[keep]


def saturated_share(g, cam, cfg):
  """share of the visible colours outside (0, 1), by the float64 oracle; None when nothing is visible"""
  g64, cam64 = g.to(dtype=torch.float64), cam.to(dtype=torch.float64)
  _, _, idx = oproj.apply(g64.position, g64.log_scaling, g64.rotation, g64.alpha_logit, cam64.T_camera_world,
                          cam64.projection, cam64.image_size, cam64.depth_range, cfg.blur_cov, cfg.clamp_margin,
                          cfg.alpha_threshold)
  if idx.numel() == 0:
    return None
  f = osh.evaluate_sh_at(g64.feature, g64.position, idx, torch.inverse(cam64.T_camera_world)[0:3, 3])
  return float(((f <= 0) | (f >= 1)).double().mean())


def edge_scene(degree, n):
  """n consecutive rows of the pool whose visible colours are partly saturated (Part B asserts 10 % .. 75 %; a single
  gaussian has only 0, 1/3, 2/3 or 1 to offer and degree 0 sits near 11 %, so the window slides until the share is
  inside)"""
  g, cam = pool(degree)
  for first in range(0, g.position.shape[0] - n):
    sub = rows(g, first, n)
    share = saturated_share(sub, cam, edge_cfg())
    if share is not None and 0.11 <= share <= 0.74:
      return sub, cam
  raise AssertionError("no window of the pool has partly saturated colours")


class nan_guarded:
  """While active, torch.empty_like on the GPU returns the first rows of a NaN-filled buffer one row longer: what the
  frame writes its gradients into.  ``check()``: the guard rows are still NaN."""

  def __init__(self, monkeypatch):
    self.buffers, self.real = [], torch.empty_like
    monkeypatch.setattr(torch, 'empty_like', self.make)

  def make(self, t, *args, **kwargs):
    if args or kwargs or t.dim() < 1 or not t.is_cuda or not t.is_floating_point() or not t.is_contiguous():
      return self.real(t, *args, **kwargs)
    big = torch.full((t.shape[0] + 1,) + tuple(t.shape[1:]), float('nan'), dtype=t.dtype, device=t.device)
    self.buffers.append(big)
    return big[:t.shape[0]]

  def check(self):
    assert self.buffers, "the frame allocated no gradient array through torch.empty_like"
    for big in self.buffers:
      assert bool(torch.isnan(big[-1]).all()), "a guard row behind a gradient array was written"


def assert_leaves(gd, g, cam, cfg, p_h, gp_h, gf_h, gp_k, gf_k, idx, what):
  idx64, ref64 = oracle_leaf_grads_from_covariance(g, cam, cfg, p_h, gp_h, gf_h)
  idx32, ref32 = oracle_leaf_grads(g, cam, cfg, gp_k, gf_k, torch.float32)
  assert torch.equal(idx64, idx) and torch.equal(idx32, idx)
  for k, w64, w32 in zip(LEAVES, ref64, ref32):
    got = getattr(gd, k).grad.cpu()
    assert bool(torch.isfinite(got).all()), (what, k, 'a gradient row was not written')
    assert_f32_gradient_as_accurate_as_reference(got, w64, w32, what + (k,))


@pytest.mark.parametrize('deterministic', [False, True])
@pytest.mark.parametrize('degree', [0, 1, 2, 3])
@pytest.mark.parametrize('n', EDGE_NS)
def test_wave_and_workgroup_edges(n, degree, deterministic, monkeypatch):
  """one lane, one short of a wave, a wave, a wave and a lane, a workgroup less / exactly / plus a lane, two workgroups
  and a lane: gradients of the five leaves against the float64 oracle, moment rows clean afterwards"""
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', deterministic)
  cfg = edge_cfg()
  g, cam = edge_scene(degree, n)
  torch.manual_seed(2)
  G = torch.rand(EDGE_SIZE[1], EDGE_SIZE[0], 3, dtype=torch.float64) + 0.5
  guard = nan_guarded(monkeypatch)
  gd, _, idx, p_h, (gp_h, gf_h), (gp_k, gf_k) = _frame_backward(g, cam, cfg, G)
  guard.check()
  _assert_moments_buffer_clean(n, deterministic)
  assert_leaves(gd, g, cam, cfg, p_h, gp_h, gf_h, gp_k, gf_k, idx, (n, degree, deterministic))


CULL_N = 4 * 256 + 1


@functools.lru_cache(maxsize=None)
def culled_scene():
  """about half of the gaussians mirrored through the camera centre (depth < 0: culled), among them a whole wave
  (rows 128 .. 191) and the last row, which sits alone in the ragged last block"""
  g, cam = pool(3)
  g = rows(g, 0, CULL_N)
  assert g.position.shape[0] == CULL_N
  gen = torch.Generator().manual_seed(9)
  behind = torch.rand(CULL_N, generator=gen) < 0.5
  behind[128:192] = True
  behind[-1] = True
  behind[0:64] = False                  # and a wave with no culled row
  centre = torch.inverse(cam.T_camera_world)[0:3, 3]
  position = torch.where(behind[:, None], 2 * centre[None, :] - g.position, g.position)
  return g.replace(position=position), cam, behind


@pytest.mark.parametrize('deterministic', [False, True])
def test_culled_rows_inside_waves(deterministic, monkeypatch):
  """culled rows inside staged blocks, a culled wave, a culled last row: exact zero rows, guard rows untouched, moment
  rows (all 16 columns, culled and tail rows included) zero afterwards; two deterministic frames agree bit for bit"""
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', deterministic)
  cfg = edge_cfg()
  g, cam, behind = culled_scene()
  torch.manual_seed(4)
  G = torch.rand(EDGE_SIZE[1], EDGE_SIZE[0], 3, dtype=torch.float64) + 0.5
  guard = nan_guarded(monkeypatch)
  gd, _, idx, p_h, (gp_h, gf_h), (gp_k, gf_k) = _frame_backward(g, cam, cfg, G)
  guard.check()
  _assert_moments_buffer_clean(CULL_N, deterministic)
  visible = torch.zeros(CULL_N, dtype=torch.bool)
  visible[idx] = True
  assert not bool((visible & behind).any()) and 0.3 < float(visible.float().mean()) < 0.6
  for k in LEAVES:
    got = getattr(gd, k).grad.cpu()
    assert int(got[~visible].ne(0).sum()) == 0 and not bool(torch.isnan(got).any()), (k, 'culled rows are not exact zeros')
  assert_leaves(gd, g, cam, cfg, p_h, gp_h, gf_h, gp_k, gf_k, idx, ('culled', deterministic))
  if deterministic:
    again = _frame_backward(g, cam, cfg, G)[0]
    _assert_moments_buffer_clean(CULL_N, True)
    for k in LEAVES:
      assert torch.equal(getattr(gd, k).grad, getattr(again, k).grad), (k, 'two deterministic frames differ')


def leaf_grads(leaves, g, cam, cfg, G, camera_grads=False):
  from dataclasses import replace
  gd = g.to(DEV).replace(**{k: t.requires_grad_(True) for k, t in zip(LEAVES, leaves)})
  cam_d = cam.to(device=DEV)
  if camera_grads:
    cam_d = replace(cam_d, T_camera_world=cam_d.T_camera_world.clone().requires_grad_(True),
                    projection=cam_d.projection.clone().requires_grad_(True))
  r = render_gaussians(gd, cam_d, cfg, use_sh=True)
  (r.image * G).sum().backward()
  torch.cuda.synchronize()
  grads = [t.grad.clone() for t in leaves]
  return grads + [cam_d.T_camera_world.grad.clone(), cam_d.projection.grad.clone()] if camera_grads else grads


def offset_view(t, floats):
  """a copy of t that starts `floats` floats into a larger NaN-filled allocation"""
  flat = torch.full((t.numel() + floats,), float('nan'), dtype=t.dtype, device=t.device)
  v = flat[floats:].view(t.shape)
  v.copy_(t)
  return v


@pytest.mark.parametrize('offset', ['row', 'float'])
def test_unaligned_leaves(offset, monkeypatch):
  """the five leaves as views one row into a larger allocation ('row': position and log-scaling 12 bytes, alpha logit
  4 bytes off a 16-byte boundary, rotation and features still on one: the 4- and 12-byte DMA pieces take them), and
  with the rotation one float in instead ('float': the 16-byte pieces cannot take it, the whole scene goes by the
  lanes' own loads): deterministic gradients bit-identical to the aligned copy's"""
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)
  cfg = edge_cfg()
  g, cam = pool(3)
  g = rows(g, 0, CULL_N)
  torch.manual_seed(6)
  G = (torch.rand(EDGE_SIZE[1], EDGE_SIZE[0], 3) + 0.5).to(DEV)
  aligned = [getattr(g, k).to(DEV).clone() for k in LEAVES]
  assert all(t.data_ptr() % 16 == 0 for t in aligned)
  shifted = [offset_view(t, 1 if offset == 'float' and k == 'rotation' else t[0].numel()) for k, t in zip(LEAVES, aligned)]
  assert shifted[0].data_ptr() % 16 != 0 and (shifted[2].data_ptr() % 16 != 0) == (offset == 'float')
  want = leaf_grads(aligned, g, cam, cfg, G)
  got = leaf_grads(shifted, g, cam, cfg, G)
  for k, a, b in zip(LEAVES, got, want):
    assert float(b.abs().max()) > 0
    assert torch.equal(a, b), (k, offset, float((a - b).abs().max()))


def test_loop_runs_at_least_twice_with_ragged_tail(monkeypatch):
  """n = 3 x 256 x 8 x (compute units) + 257 with camera gradients asked for, which cap the grid at 2048 workgroups:
  every wave takes at least two blocks (three on 256 compute units), each but the first staged while its predecessor
  is worked on, and the last block is ragged.  Tiny splats on 256 x 192, 32 of them per pixel.

  Truth in float64 from the same inputs, paired the way tests/test_gpu_configs.py pairs float32 and float64 at full
  size: the float64 generic rasterizer on the SAME splats and tile lists gives the 2D-boundary gradients, the float64
  projection / SH chain (oracle_leaf_grads_from_covariance) carries them to the five leaves; every row beyond 1e-4 of
  the largest gradient must have a (pixel, splat) pair within 1e-5 of the blend gate under it, counted and bounded
  (check_rows, MAX_ROWS_BEYOND).  (A float64 frame that maps for itself orders splats of nearly equal depth
  differently from the float32 one; at this density that moved 152 position rows by up to 9 % of the largest gradient,
  on the kernels before the staging as well: tile lists are shared for that reason.)

  The camera gradients are asked for only to cap the grid: sums of 1.5 M float32 terms whose cancellation this scene
  does not control; Part B of test_gpu_gaussian_bwd.py holds them to the oracle, here they must be finite."""
  from taichi_splatting_amd import rasterize_with_tiles
  from taichi_splatting_amd.spherical_harmonics import evaluate_sh_at
  cus = torch.cuda.get_device_properties(0).multi_processor_count
  n, size = 3 * 256 * 8 * cus + 257, (256, 192)
  assert n >= 2 * 2048 * 256
  cfg = RasterConfig(tile_size=16, pixel_stride=(2, 2))
  g, cam = scene(n, size, seed=3)
  torch.manual_seed(8)
  G = torch.rand(size[1], size[0], 3, dtype=torch.float64, device=DEV) + 0.5
  guard = nan_guarded(monkeypatch)
  got = leaf_grads([getattr(g, k).to(DEV).clone() for k in LEAVES], g, cam, cfg, G.float(), camera_grads=True)
  guard.check()
  monkeypatch.undo()
  _assert_moments_buffer_clean(n, raster_function.DETERMINISTIC_BACKWARD)

  gd, cam_d = g.to(DEV), cam.to(device=DEV)
  with torch.no_grad():
    p, depth, idx = project_to_image(gd, cam_d, cfg)
    o2p, ranges = map_to_tiles(p, ndc_depth(depth, cam.near_plane, cam.far_plane), cam.image_size, cfg)
    feats = evaluate_sh_at(gd.feature, gd.position, idx, cam_d.camera_position)
    _, splat_flag = near_gate_gpu(p, o2p, ranges, cam.image_size, cfg, 1e-5)
  pp, ff = p.double().requires_grad_(True), feats.double().requires_grad_(True)
  out = rasterize_with_tiles(pp, ff, o2p, ranges.view(-1, 2), cam.image_size, cfg)
  (out.image * G).sum().backward()
  idx64, want = oracle_leaf_grads_from_covariance(gd, cam_d, cfg, p.double(), pp.grad, ff.grad)
  assert torch.equal(idx64, idx.long()) and idx.shape[0] > 0.3 * n
  flag = torch.zeros(n, dtype=torch.bool, device=DEV)
  flag[idx.long()] = splat_flag
  print(f"grid-stride loop: {idx.shape[0]} of {n} visible, {float(flag.float().mean()):.4f} of the rows flagged")
  assert float(flag.float().mean()) < 0.05          # as test_config_c_full_size asks of its flagged share
  for k, a, b in zip(LEAVES, got, want):
    assert bool(torch.isfinite(a).all()), (k, 'a gradient row was not written')
    check_rows(a.reshape(n, -1), b.reshape(n, -1), flag, f"grid-stride loop, d{k}", max_fraction=MAX_ROWS_BEYOND)
  for name, a in zip(('T_camera_world', 'projection'), got[5:]):
    assert bool(torch.isfinite(a).all()), name
