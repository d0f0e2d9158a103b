"""GPU tests of the geometry kernels (csrc/geometry.hip through taichi_splatting_amd/geometry.py) against the float64
oracle on the CPU (tests/geometry_oracle.py), within error bounds that come from the number format and not from the
kernels.  With eps the unit roundoff of the dtype under test and K = 16 roundings behind a value:

  normals           |d| <= K eps per component (a unit vector): an entry of q / |q| carries three roundings, a column
                    entry is a sum of products of two of them, 2 (2 x 3 + 1) + 2 = 16 at worst
  rotation gradient |d| <= 8 K eps |g| / |q| per component: every entry is a handful of products of unit-quaternion
                    entries with g, projected off q and divided by |q|
  consistency       the bounds of tests/geometry_oracle.py's docstring: K eps cond per component of n_d with
                    cond = |a| |b| / |a x b| times the cancellation of the two differences, the loss and the gradients
                    from the same quantity.  Pixels with cond > 1e4 are left out; the cases keep them under 1 % (0 here)

The float32 composition of the same formulas in torch on the CPU, an independent implementation, is asserted to sit at
<= 0.1 of the consistency bounds (measured: <= 0.03, as the kernels; float64 kernels <= 0.006).  For the normals, where
the count above is the worst case of a dozen operations and not a loose one, it is asserted at <= 0.75 (measured on two
hosts: forward <= 0.57, rotation gradient <= 0.09; the kernels: forward <= 0.57, rotation gradient <= 0.10, in both
dtypes).  float64 on the GPU against the float64 oracle is the sharp test.

Which shape runs which path (a workgroup owns 64 x 16 pixels; the backward stages tile + 2 and evaluates the centres of
tile + 1):
  (1, 1) (2, 5) (3, 2)   no interior pixel: loss and gradients exactly 0, one workgroup
  (3, 3)                 one interior pixel
  (19, 200)              4 x 2 workgroups, ragged in x (8 of 64 columns) and y (3 of 16 rows); stencils across tile edges
  (37, 53)               1 x 3 workgroups, ragged in both
  (33, 130)              3 x 3 workgroups; pixels (63..64, 15..16), (127..128, 31..32): the radius-2 diamond crosses a tile
                         corner and the last tiles hold one row and two columns
  (256, 256)             4 x 16 whole tiles
"""
import functools

import pytest
import torch

from tests import geometry_oracle as go

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
K = go.K

NORMAL_SIZES = [1, 63, 64, 65, 1000]
SHAPES = [(1, 1), (2, 5), (3, 2), (3, 3), (19, 200), (37, 53), (33, 130), (256, 256)]
LAYOUTS = [(5, (0, 1, 2)), (5, (4, 3, 0)), (6, (5, 3, 0)), (6, (1, 0, 3))]      # F, (depth, alpha, normal) offsets
GRAD_LOSS = 0.7


# ---- per-gaussian normals ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def normal_case(n, dtype):
  """inputs in ``dtype``, the float64 oracle on those values (normals, rotation gradient for the upstream g): shared"""
  pos, ls, rot, cam, planted = (t.to(dtype) if isinstance(t, torch.Tensor) else t for t in go.make_gaussians(n))
  g = torch.randn((n, 3), generator=torch.Generator().manual_seed(5 + n), dtype=torch.float64).to(dtype)
  q = rot.double().clone().requires_grad_(True)
  want = go.normals(pos.double(), ls.double(), q, cam.double())
  want.backward(g.double())
  margin, gap = go.normal_margins(pos.double(), ls.double(), rot.double(), cam.double())
  return pos, ls, rot, cam, g, planted, want.detach(), q.grad, margin, gap


def fused_normals(pos, ls, rot, cam, g, dtype, grads=(False, False, True, False)):
  from taichi_splatting_amd import gaussian_normals, Gaussians3D
  n = pos.shape[0]
  leaves = [t.to(DEV, dtype).requires_grad_(r) for t, r in zip((pos, ls, rot, cam), grads)]
  scene = Gaussians3D(position=leaves[0], log_scaling=leaves[1], rotation=leaves[2],
                      alpha_logit=torch.zeros((n, 1), device=DEV, dtype=dtype),
                      feature=torch.zeros((n, 3), device=DEV, dtype=dtype), batch_size=(n,))
  out = gaussian_normals(scene, leaves[3])
  if any(grads):
    out.backward(g.to(DEV, dtype))
  torch.cuda.synchronize()
  return out.detach().cpu(), [None if t.grad is None else t.grad.cpu() for t in leaves]


@pytest.mark.parametrize('dtype', [torch.float32, torch.float64])
@pytest.mark.parametrize('n', NORMAL_SIZES)
def test_gaussian_normals_hold_the_bounds(n, dtype):
  pos, ls, rot, cam, g, planted, want, want_grad, margin, gap = normal_case(n, dtype)
  eps = go.unit_roundoff(dtype)
  # no random row is excluded: the sign and the axis of every one are well-posed
  assert bool((margin >= 1e-3).all()) and bool((gap[planted:] >= 1e-3).all())
  if n >= 63:
    assert gap[0] == 0 and gap[1] == 0                               # the planted ties
    flipped = (go.rotation_columns(rot.double() / rot.double().norm(dim=1, keepdim=True))[
      torch.arange(n), go.smallest_axis(ls.double())] * want).sum(1) < 0
    assert bool(flipped[4]) and bool(flipped.any()) and not bool(flipped.all())
  got, grads = fused_normals(pos, ls, rot, cam, g, dtype, grads=(True, True, True, True))
  bound_grad = 8 * K * eps * g.double().norm(dim=1, keepdim=True) / rot.double().norm(dim=1, keepdim=True)
  e_fwd, e_bwd = go.excess(got, want, K * eps), go.excess(grads[2], want_grad, bound_grad)
  print(f"normals n = {n} {dtype}: error / bound: forward {e_fwd:.3f}, rotation gradient {e_bwd:.3f}")
  assert e_fwd <= 1 and e_bwd <= 1
  assert grads[0] is None and grads[1] is None and grads[3] is None   # position, log_scaling, camera_position: none
  if n >= 63:
    assert float((got[2] - got[3]).abs().max()) <= 2 * K * eps        # q and -0.01 q are one rotation
  if dtype == torch.float32:
    # an independent float32 implementation (the oracle's formulas in float32 on the CPU) sits well inside
    q = rot.clone().requires_grad_(True)
    mine = go.normals(pos, ls, q, cam)
    mine.backward(g)
    s_fwd, s_bwd = go.excess(mine.detach(), want, K * eps), go.excess(q.grad, want_grad, bound_grad)
    print(f"float32 torch composition on the CPU: forward {s_fwd:.3f}, rotation gradient {s_bwd:.3f}")
    assert s_fwd <= 0.75 and s_bwd <= 0.75


def test_gaussian_normals_launch_no_backward_without_a_rotation_gradient():
  pos, ls, rot, cam, g, *_ = normal_case(65, torch.float32)
  out, grads = fused_normals(pos, ls, rot, cam, g, torch.float32, grads=(True, True, False, False))
  assert all(t is None for t in grads)
  from taichi_splatting_amd import geometry
  calls = []
  original = geometry.gaussian_normals_backward
  geometry.gaussian_normals_backward = lambda *a: calls.append(1) or original(*a)
  try:
    fused_normals(pos, ls, rot, cam, g, torch.float32, grads=(True, False, False, False))
    assert calls == []
    fused_normals(pos, ls, rot, cam, g, torch.float32, grads=(False, False, True, False))
    assert calls == [1]
  finally:
    geometry.gaussian_normals_backward = original
  a, _ = fused_normals(pos, ls, rot, cam, g, torch.float32)
  b, _ = fused_normals(pos, ls, rot, cam, g, torch.float32)
  assert torch.equal(a, b) and torch.equal(a, out)


# ---- normal consistency -----------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def case(shape, layout, dtype, weighted):
  """(accum, projection, pixel_weight | None) in ``dtype``, the float64 oracle ON THOSE VALUES and the bounds for ``dtype``:
  computed once, shared, never written to"""
  f, offsets = layout
  accum, proj, weight = (t.to(dtype) for t in go.make_image(*shape, f, offsets))
  weight = weight if weighted else None
  want = go.reference(accum.double(), offsets, proj.double(), None if weight is None else weight.double(), 0.5, GRAD_LOSS)
  return accum, proj, weight, want, go.bounds(accum, offsets, proj, weight, 0.5, go.unit_roundoff(dtype), GRAD_LOSS)


def fused(accum, offsets, proj, weight, dtype, grad_loss=GRAD_LOSS):
  from taichi_splatting_amd import normal_consistency
  x = accum.to(DEV, dtype).requires_grad_(True)
  loss, nd = normal_consistency(x, *offsets, proj.to(DEV, dtype), pixel_weight=None if weight is None else weight.to(DEV, dtype),
                                return_normals=True)
  (loss * grad_loss).backward()
  torch.cuda.synchronize()
  assert not nd.requires_grad
  return loss.detach().cpu(), nd.cpu(), x.grad.cpu()


def excesses(got, want, b, offsets):
  oz, oa, on = offsets
  return (abs(float(got[0]) - float(want[0])) / b['loss'] if b['loss'] > 0 else float(got[0] != want[0]),
          go.excess(got[1], want[1], b['nd'][..., None], b['covered_nd'][..., None]),
          go.excess(got[2][..., on:on + 3], want[2][..., on:on + 3], b['grad'][..., on:on + 3], b['covered_grad'][..., None]),
          go.excess(got[2][..., oz], want[2][..., oz], b['grad'][..., oz], b['covered_depth_grad']),
          go.excess(got[2][..., oa], want[2][..., oa], b['grad'][..., oa], b['covered_depth_grad']))


def check(shape, layout, dtype, weighted):
  f, offsets = layout
  accum, proj, weight, want, b = case(shape, layout, dtype, weighted)
  got = fused(accum, offsets, proj, weight, dtype)
  e = excesses(got, want, b, offsets)
  cond = float(b['cond'].max()) if b['cond'].numel() else 0.0
  print(f"{dtype} {shape} F = {f} offsets {offsets} weight {'given' if weighted else 'alpha'}: loss {float(want[0]):.6f}; "
        f"error / bound: loss {e[0]:.3f}, n_d {e[1]:.3f}, normal grad {e[2]:.3f}, depth grad {e[3]:.3f}, alpha grad {e[4]:.3f}; "
        f"largest cond {cond:.1f}, excluded {b['excluded']:.5f}")
  assert cond <= go.CAP and b['excluded'] <= 0.01
  assert all(bool(torch.isfinite(t).all()) for t in got)
  assert max(e) <= 1
  unused = [c for c in range(f) if c not in (offsets[0], offsets[1], offsets[2], offsets[2] + 1, offsets[2] + 2)]
  assert bool((got[2][..., unused] == 0).all())
  if shape[0] < 3 or shape[1] < 3:
    assert float(got[0]) == 0.0 and bool((got[2] == 0).all()) and bool((got[1] == 0).all())
  elif not weighted:
    assert float(want[0]) > 0
  return got


@pytest.mark.parametrize('shape', SHAPES)
def test_float32_consistency_holds_the_bounds(shape):
  layout = LAYOUTS[SHAPES.index(shape) % len(LAYOUTS)]
  for weighted in (False, True):
    check(shape, layout, torch.float32, weighted)
    # an independent float32 implementation holds a tenth of the same bounds
    accum, proj, weight, want, b = case(shape, layout, torch.float32, weighted)
    e = excesses(go.reference(accum, layout[1], proj, weight, 0.5, GRAD_LOSS), want, b, layout[1])
    print(f"float32 torch composition on the CPU: error / bound {tuple(round(v, 4) for v in e)}")
    assert max(e) <= 0.1


@pytest.mark.parametrize('shape', SHAPES)
def test_float64_consistency_holds_the_bounds(shape):
  for layout in (LAYOUTS[SHAPES.index(shape) % len(LAYOUTS)], LAYOUTS[(SHAPES.index(shape) + 2) % len(LAYOUTS)]):
    for weighted in (False, True):
      check(shape, layout, torch.float64, weighted)


@pytest.mark.parametrize('layout', LAYOUTS)
def test_every_channel_layout(layout):
  check((37, 53), layout, torch.float32, False)
  check((33, 130), layout, torch.float64, True)


def test_two_channels_have_no_normals():
  from taichi_splatting_amd import normal_consistency, normal_consistency_loss, GeometryImages, CameraParams
  accum = torch.ones((8, 8, 2), device=DEV)
  proj = torch.tensor([10., 10., 4., 4.], device=DEV)
  camera = CameraParams(projection=proj, T_camera_world=torch.eye(4, device=DEV), near_plane=0.1, far_plane=10., image_size=(8, 8))
  with pytest.raises(ValueError):
    normal_consistency_loss(GeometryImages(accum=accum, camera=camera))
  with pytest.raises(ValueError):
    normal_consistency(accum, 0, 1, 2, proj)


def test_two_runs_are_bitwise_equal():
  accum, proj, weight, _, _ = case((33, 130), LAYOUTS[2], torch.float32, True)
  a = fused(accum, LAYOUTS[2][1], proj, weight, torch.float32)
  b = fused(accum, LAYOUTS[2][1], proj, weight, torch.float32)
  assert all(torch.equal(x, y) for x, y in zip(a, b))


def test_graph_replay_follows_projection_and_accum():
  """one capture of forward + backward; projection and accum are then rewritten in place: the replay equals eager"""
  from taichi_splatting_amd import normal_consistency
  layout = LAYOUTS[1]
  accum, proj, _, _, _ = case((37, 53), layout, torch.float32, False)
  other = go.make_image(37, 53, *layout, seed=3)[0].float()
  x = accum.to(DEV).requires_grad_(True)
  p = proj.to(DEV)

  def step():
    loss, nd = normal_consistency(x, *layout[1], p, return_normals=True)
    return loss, nd, torch.autograd.grad(loss, x)[0]

  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    step()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured = step()
  with torch.no_grad():
    x.copy_(other.to(DEV))
    p.copy_(torch.tensor([61.0, 57.0, 25.1, 19.4], device=DEV))
  graph.replay()
  torch.cuda.synchronize()
  eager = step()
  torch.cuda.synchronize()
  first = fused(accum, layout[1], proj, None, torch.float32, grad_loss=1.0)
  assert all(torch.equal(a, b) for a, b in zip(captured, eager))
  assert not torch.equal(eager[2].cpu(), first[2])                   # and the new values are not the old ones


# ---- integration with the frame ---------------------------------------------------------------------------------------

def frame_scene(n=300, size=(64, 48), seed=11):
  from taichi_splatting_amd.testing import random_3d_gaussians, random_camera
  torch.manual_seed(seed)
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(n, cam, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=0.1)
  return g.to(dtype=torch.float32).to(DEV), cam.to(dtype=torch.float32).to(device=DEV)


def test_render_geometry_is_render_features_of_the_stated_rows():
  """accum against render_features of rows [z, 1, z^2, n_cam].  With the normals of gaussian_normals the whole image is
  bitwise equal.  With the ORACLE's normals (float64 on the CPU, rounded to float32) the depth, alpha and z^2 channels
  are bitwise equal and the normal channels differ by what K eps per component of a unit normal can do: n_cam moves by
  at most sqrt(3) (K + 3) eps (the 3 x 3 product adds three roundings), blended with weights that sum to alpha.

  alpha against Rendering.image_weight: two kernels sum the same weights w_i = a_i prod_{j<i} (1 - a_j) in float32.  With
  L the longest tile list, a weight carries at most L + 3 roundings in each kernel and a sum of L terms L - 1 more:
  |d| <= 2 (2 L + 2) eps alpha; a pixel at the saturation threshold may stop one splat apart, which is at most the
  transmittance left, 1 - saturate_threshold."""
  from taichi_splatting_amd import RasterConfig, render_gaussians, render_geometry, render_features, gaussian_normals
  g, cam = frame_scene()
  config = RasterConfig(tile_size=16)
  r = render_gaussians(g, cam, config, use_sh=False)
  geo = render_geometry(r, g, depth_variance=True)
  assert geo.accum.shape == (48, 64, 6) and (geo.depth_offset, geo.alpha_offset, geo.depth_sq_offset, geo.normal_offset) == (0, 1, 2, 3)
  T = cam.T_camera_world
  z = g.position @ T[2, :3] + T[2, 3]
  centre = cam.camera_position
  mine = gaussian_normals(g, centre) @ T[:3, :3].T
  rows = torch.cat([z[:, None], torch.ones_like(z)[:, None], z.square()[:, None], mine], 1)
  assert torch.equal(geo.accum, render_features(r, rows))
  oracle = go.normals(g.position.cpu().double(), g.log_scaling.cpu().double(), g.rotation.cpu().double(), centre.cpu().double())
  rows_o = torch.cat([rows[:, :3], oracle.float().to(DEV) @ T[:3, :3].T], 1)
  accum_o = render_features(r, rows_o)
  assert torch.equal(geo.accum[..., :3], accum_o[..., :3])
  eps = go.unit_roundoff(torch.float32)
  bound = (3 ** 0.5 * (K + 3) * eps * geo.alpha + 4 * eps).unsqueeze(-1)
  e = go.excess(geo.accum[..., 3:].cpu(), accum_o[..., 3:].cpu(), bound.cpu())
  print(f"normal channels against the oracle's normals: error / bound {e:.3f}")
  assert e <= 1
  ranges = r.frame.tile_ranges().view(-1, 2)
  longest = int((ranges[:, 1] - ranges[:, 0]).max())
  alpha, weight = geo.alpha.cpu().double(), r.image_weight.cpu().double()
  bound = 2 * (2 * longest + 2) * eps * weight + (1 - config.saturate_threshold) * (weight >= config.saturate_threshold - 1e-3)
  e = go.excess(alpha, weight, bound)
  print(f"alpha against image_weight: longest list {longest}, largest difference {float((alpha - weight).abs().max()):.3e}, "
        f"error / bound {e:.3f}")
  assert e <= 1
  assert geo.alpha.requires_grad is False and not r.image_weight.requires_grad
  assert torch.isfinite(geo.depth).all() and torch.isfinite(geo.normal).all() and torch.isfinite(geo.depth_variance).all()
  two = render_geometry(r, g, normals=False)
  assert two.accum.shape == (48, 64, 2) and torch.equal(two.accum, geo.accum[..., :2])
  with pytest.raises(ValueError):
    from taichi_splatting_amd import normal_consistency_loss
    normal_consistency_loss(two)


def test_one_backward_reaches_every_parameter_and_the_pose():
  from taichi_splatting_amd import RasterConfig, render_gaussians, render_geometry, normal_consistency_loss, l1_ssim_loss
  from dataclasses import replace
  g, cam = frame_scene()
  g = g.clone().requires_grad_(True)
  pose = cam.T_camera_world.clone().requires_grad_(True)
  cam = replace(cam, T_camera_world=pose)
  r = render_gaussians(g, cam, RasterConfig(tile_size=16), use_sh=False)
  geo = render_geometry(r, g)
  gen = torch.Generator().manual_seed(2)
  target = torch.rand((48, 64, 3), generator=gen).to(DEV)
  depth_target = (torch.rand((48, 64), generator=gen) * 5 + 1).to(DEV)
  loss = l1_ssim_loss(r.image, target) + normal_consistency_loss(geo) + (geo.depth - depth_target).abs().mean()
  loss.backward()
  for name, t in (('position', g.position), ('log_scaling', g.log_scaling), ('rotation', g.rotation),
                  ('alpha_logit', g.alpha_logit), ('feature', g.feature), ('T_camera_world', pose)):
    assert t.grad is not None and bool(torch.isfinite(t.grad).all()), name
    assert float(t.grad.abs().max()) > 0, name
    print(f"{name}: largest gradient entry {float(t.grad.abs().max()):.3e}")


def test_adam_on_rotations_lowers_the_consistency_loss():
  """a planar sheet of flat gaussians facing the camera, rotations perturbed: thirty Adam steps on rotation alone"""
  from taichi_splatting_amd import (CameraParams, Gaussians3D, RasterConfig, render_gaussians, render_geometry,
                                    normal_consistency_loss)
  gen = torch.Generator().manual_seed(4)
  xs, ys = torch.meshgrid(torch.linspace(-2.6, 2.6, 20), torch.linspace(-1.9, 1.9, 15), indexing='xy')
  n = xs.numel()
  position = torch.stack([xs.flatten(), ys.flatten(), torch.full((n,), 5.0)], 1)
  rotation = torch.tensor([0., 0., 0., 1.]).expand(n, 4) + 0.15 * torch.randn((n, 4), generator=gen)
  scene = Gaussians3D(position=position, log_scaling=torch.tensor([-1.6, -1.6, -5.0]).expand(n, 3).contiguous(),
                      rotation=rotation.contiguous(), alpha_logit=torch.full((n, 1), 2.0),
                      feature=torch.rand((n, 3), generator=gen), batch_size=(n,)).to(DEV)
  camera = CameraParams(projection=torch.tensor([60., 60., 32., 24.]), T_camera_world=torch.eye(4), near_plane=0.1,
                        far_plane=100., image_size=(64, 48)).to(device=DEV)
  q = scene.rotation.clone().requires_grad_(True)
  optimiser = torch.optim.Adam([q], lr=0.02)
  values = []
  for _ in range(31):
    g = scene.replace(rotation=q)
    r = render_gaussians(g, camera, RasterConfig(tile_size=16), use_sh=False)
    loss = normal_consistency_loss(render_geometry(r, g))
    values.append(float(loss.detach()))
    if len(values) <= 30:
      optimiser.zero_grad()
      loss.backward()
      optimiser.step()
  print(f"consistency loss: {values[0]:.6f} before, {values[-1]:.6f} after thirty Adam steps on rotation")
  assert values[0] > 0 and values[-1] < values[0]
