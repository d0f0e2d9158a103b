"""-m gpu: the active SH degree (``evaluate_sh_at(active_degree=d)``, ``render_gaussians(sh_degree=d)``) of a scene
stored at degree D, for all ten pairs 0 <= d <= D <= 3.

The definition of the feature is the slice: everything is compared with ``oracle.sh.evaluate_sh_at`` in float64 on
``params[:, :, :(d + 1)**2]`` (or with the library itself run on the sliced scene), and the gradient of the other
coefficients must be exactly zero — written, not left over: right before every backward pass a tensor of the
gradient's size is filled with NaN and freed, so that a row the kernel did not write comes back from the caching
allocator as NaN instead of as an accidental zero.

Shapes are the smallest that reach every branch: n = 300 gaussians (one full 256-thread block and a last wave of 44),
index lists of 229 unique (v < n), 300 unique (v == n: the ``torch.empty`` gradient of ``_SHFunction.backward``) and 400
with repeats (atomics), K = 1, 3 (128-bit pieces), 4 (SH_MAX_F) and 5 (``sh_bwd_kernel``'s atomics)."""
import functools
from dataclasses import replace

import pytest
import torch

from oracle import sh as osh
from taichi_splatting_amd import RasterConfig, evaluate_sh_at, frame, render_gaussians
from taichi_splatting_amd.testing import random_camera, random_3d_gaussians

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
N = 300
PAIRS = [(d, D) for D in range(4) for d in range(D + 1)]
DTYPES = [torch.float32, torch.float64]
SEED = {1: 0, 3: 0, 4: 0, 5: 0}        # per K; (seed 2, K = 5, d = 1) is the one case of seeds 0..3 that fails the margin check


def nd(d):
  return (d + 1) ** 2


@functools.lru_cache(maxsize=None)
def sh_inputs(k, dtype):
  """(params (N, K, 16), points, camera position) on the CPU in ``dtype``; a scene stored at degree D is the first
  (D + 1)^2 coefficients of params.  Shared by every case: never modified."""
  gen = torch.Generator().manual_seed(SEED[k])
  params = 0.5 * torch.randn(N, k, 16, generator=gen, dtype=torch.float64)
  points = 2.0 * torch.randn(N, 3, generator=gen, dtype=torch.float64)
  cam = torch.tensor([0.3, -0.2, 6.0], dtype=torch.float64)
  return params.to(dtype), points.to(dtype), cam.to(dtype)


@functools.lru_cache(maxsize=None)
def index_lists():
  gen = torch.Generator().manual_seed(11)
  return {'u229': (torch.randperm(N, generator=gen)[:229], True),
          'u300': (torch.randperm(N, generator=gen), True),
          'r400': (torch.randint(0, N, (400,), generator=gen), False)}


@functools.lru_cache(maxsize=None)
def oracle(k, d, dtype, which):
  """float64 oracle on the slice, on the (float32 or float64) input VALUES of the kernel run: (out, d params,
  d positions, d camera, upstream gradient).  No pre-clamp value may sit within 1e-5 of 0 or 1, so that no gradient
  depends on the side of the clamp a rounding lands on."""
  params, points, cam = (t.double() for t in sh_inputs(k, dtype))
  idx, _ = index_lists()[which]
  sliced = params[:, :, :nd(d)].clone().requires_grad_(True)
  points, cam = points.clone().requires_grad_(True), cam.clone().requires_grad_(True)
  dirs = points.detach()[idx] - cam.detach()
  dirs = dirs / dirs.norm(dim=1, keepdim=True)
  pre = (osh.rsh_cart(dirs, d).unsqueeze(1) * sliced.detach()[idx]).sum(-1) + 0.5
  margin = torch.minimum(pre.abs(), (pre - 1).abs()).min().item()
  assert margin > 1e-5, (k, d, which, margin)
  out = osh.evaluate_sh_at(sliced, points, idx, cam)
  g_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(5), dtype=torch.float64)
  out.backward(g_out)
  zero_if_none = lambda t: t.grad if t.grad is not None else torch.zeros_like(t)     # degree 0 does not see the direction
  return out.detach(), sliced.grad, zero_if_none(points), zero_if_none(cam), g_out


def poison(like):
  """A freed block of NaNs where the next allocation of this size will land."""
  t = torch.full_like(like, float('nan'))
  del t


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('k', [1, 3, 4, 5])
@pytest.mark.parametrize('d,D', PAIRS)
def test_modular_forward_is_the_sliced_scene(d, D, k, dtype):
  params, points, cam = (t.to(DEV) for t in sh_inputs(k, dtype))
  stored = params[:, :, :nd(D)].contiguous()
  sliced = params[:, :, :nd(d)].contiguous()
  atol = 1e-12 if dtype == torch.float64 else 1e-5
  for which, (idx, unique) in index_lists().items():
    got = evaluate_sh_at(stored, points, idx.to(DEV), cam, unique, active_degree=d)
    same = evaluate_sh_at(sliced, points, idx.to(DEV), cam, unique)
    assert torch.equal(got, same), (which, (got - same).abs().max().item())
    want = oracle(k, d, dtype, which)[0]
    err = (got.cpu().double() - want).abs().max().item()
    print(f"forward d={d} D={D} K={k} {dtype} {which}: max err {err:.3e}, clamped {(want <= 0).sum() + (want >= 1).sum()}/{want.numel()}")
    assert err <= atol, (which, err)
  if d == D:
    assert torch.equal(evaluate_sh_at(stored, points, idx.to(DEV), cam, active_degree=None),
                       evaluate_sh_at(stored, points, idx.to(DEV), cam, active_degree=D))


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('k', [1, 3, 4, 5])
@pytest.mark.parametrize('d,D', PAIRS)
def test_modular_backward_active_bands_vs_oracle_inactive_exactly_zero(d, D, k, dtype):
  params, points, cam = (t.to(DEV) for t in sh_inputs(k, dtype))
  atol = 1e-10 if dtype == torch.float64 else 1e-5
  for which, (idx, unique) in index_lists().items():
    _, w_params, w_points, w_cam, g_out = oracle(k, d, dtype, which)
    g_out = g_out.to(dtype).to(DEV)
    # all three gradients (streamed parameter rows + the direction kernel), then the parameters alone (for 'u300' the
    # kernel owns every row of a torch.empty gradient)
    for only_params in (False, True):
      p = params[:, :, :nd(D)].contiguous().requires_grad_(True)
      x, c = points.clone().requires_grad_(not only_params), cam.clone().requires_grad_(not only_params)
      out = evaluate_sh_at(p, x, idx.to(DEV), c, unique, active_degree=d)
      poison(p)
      out.backward(g_out)
      g = p.grad.cpu().double()
      what = (d, D, k, dtype, which, only_params)
      assert g.shape == (N, k, nd(D)) and bool(torch.isfinite(g).all()), what
      assert bool((g[:, :, nd(d):] == 0).all()), (what, 'inactive bands', g[:, :, nd(d):].abs().max().item())
      errs = [(g[:, :, :nd(d)] - w_params).abs().max().item()]
      if not only_params:
        errs += [(x.grad.cpu().double() - w_points).abs().max().item(), (c.grad.cpu().double() - w_cam).abs().max().item()]
      print(f"backward d={d} D={D} K={k} {dtype} {which} only_params={only_params}: max errs {errs}")
      assert max(errs) <= atol, (what, errs)


# ---- frame executor ---------------------------------------------------------------------------------------------

SIZE = (64, 48)


@functools.lru_cache(maxsize=None)
def frame_scene(dtype):
  """300 gaussians in front of a 64 x 48 camera, ten of them moved behind it (culled by the near plane); degree-3
  coefficients 0.5 randn.  (scene, camera) on the GPU; never modified."""
  torch.manual_seed(3)
  cam = random_camera(image_size=SIZE)
  g = random_3d_gaussians(N, cam, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=0.3)
  pose = torch.inverse(cam.T_camera_world)                 # camera -> world: column 2 looks forward
  position = g.position.clone()
  position[5:15] = pose[:3, 3] - pose[:3, 2] * torch.linspace(0.5, 3.0, 10).unsqueeze(1) + 0.1 * torch.randn(10, 3)
  g = g.replace(position=position, feature=0.5 * torch.randn(N, 3, 16))
  return g.to(dtype=dtype).to(DEV), cam.to(dtype=dtype).to(device=DEV)


def stored_at(g, D):
  return g.replace(feature=g.feature[:, :, :nd(D)].contiguous())


LEAVES = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


def render_with_grads(g, cam, g_image, **kw):
  gd = g.clone().requires_grad_(True)
  cam = replace(cam, T_camera_world=cam.T_camera_world.clone().requires_grad_(True),
                projection=cam.projection.clone().requires_grad_(True))
  r = render_gaussians(gd, cam, RasterConfig(tile_size=16), use_sh=True, **kw)
  poison(gd.feature)
  r.image.backward(g_image)
  grads = {name: getattr(gd, name).grad for name in LEAVES}
  grads['T_camera_world'], grads['projection'] = cam.T_camera_world.grad, cam.projection.grad
  return r, grads


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('d,D', PAIRS)
def test_frame_at_active_degree_is_the_sliced_scene(d, D, dtype, monkeypatch):
  from taichi_splatting_amd.rasterizer import function as raster_function
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)
  assert frame.USE_FRAME
  g, cam = frame_scene(dtype)
  g_image = torch.randn(SIZE[1], SIZE[0], 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype).to(DEV)
  ra, ga = render_with_grads(stored_at(g, D), cam, g_image, sh_degree=d)
  rb, gb = render_with_grads(stored_at(g, d), cam, g_image)
  assert hasattr(ra, 'frame') and ra.frame.desc.sh_active_bands == d + 1 and rb.frame.desc.sh_active_bands == 0

  assert (ra.image - rb.image).abs().max().item() <= 2e-5
  assert (ra.image_weight - rb.image_weight).abs().max().item() <= 2e-5
  assert ra.image_weight.max().item() <= 1.0 and rb.image_weight.max().item() <= 1.0

  cam_pos = torch.inverse(cam.T_camera_world.cpu().double())[:3, 3]
  culled = None
  for r in (ra, rb):
    idx = r.points.idx.cpu()
    visible = torch.zeros(N, dtype=torch.bool)
    visible[idx] = True
    culled = ~visible
    assert 5 <= int(culled.sum()) < N // 2 and bool(culled[5:15].all())
    want = osh.evaluate_sh_at(g.feature.cpu().double()[:, :, :nd(d)], g.position.cpu().double(), idx, cam_pos)
    err = (r.points.features.detach().cpu().double() - want).abs().max().item()
    print(f"frame colours d={d} D={D} {dtype}: max err {err:.3e}")
    assert err <= 1e-5

  gfa = ga['feature'].cpu()
  assert gfa.shape == (N, 3, nd(D)) and bool(torch.isfinite(gfa).all())
  assert bool((gfa[:, :, nd(d):] == 0).all()), gfa[:, :, nd(d):].abs().max().item()
  for name in ga:
    a = ga[name].cpu().double()
    b = gb[name].cpu().double()
    if name == 'feature':
      a = a[:, :, :nd(d)]
    assert a.shape == b.shape and bool(torch.isfinite(a).all()), name
    scale = b.abs().max().item()
    err = (a - b).abs().max().item()
    print(f"frame grads d={d} D={D} {dtype} {name}: max err {err:.3e} of scale {scale:.3e}")
    assert scale > 0 and err <= 1e-4 * scale, (name, err, scale)
    if name in LEAVES:
      assert bool((ga[name].cpu()[culled] == 0).all()), (name, 'culled rows')


@pytest.mark.parametrize('dtype', DTYPES, ids=['f32', 'f64'])
@pytest.mark.parametrize('D', range(4))
def test_default_and_full_degree_are_bit_identical(D, dtype, monkeypatch):
  """sh_degree=None and sh_degree=D launch the same kernels: bit-identical images, and bit-identical gradients wherever
  the backward pass is deterministic at all."""
  from taichi_splatting_amd.rasterizer import function as raster_function
  monkeypatch.setattr(raster_function, 'DETERMINISTIC_BACKWARD', True)
  g, cam = frame_scene(dtype)
  g_image = torch.randn(SIZE[1], SIZE[0], 3, generator=torch.Generator().manual_seed(9), dtype=torch.float64).to(dtype).to(DEV)
  ra, ga = render_with_grads(stored_at(g, D), cam, g_image, sh_degree=None)
  rb, gb = render_with_grads(stored_at(g, D), cam, g_image, sh_degree=D)
  assert ra.frame.desc.sh_active_bands == 0 and rb.frame.desc.sh_active_bands == D + 1
  assert torch.equal(ra.image, rb.image) and torch.equal(ra.image_weight, rb.image_weight)
  moments_path, det = frame.backward_mode(ra.frame.desc)
  assert det and moments_path == (dtype == torch.float32)
  for name in ga:
    if moments_path:
      assert torch.equal(ga[name], gb[name]), name
    else:
      # deterministic commits exist on the float32 RGB moments path only: the float64 raster backward adds with atomics
      # in whatever order the waves arrive, so two runs of the SAME launch sequence agree to float64 rounding
      assert (ga[name] - gb[name]).abs().max().item() <= 1e-12 * gb[name].abs().max().item(), name


def test_captured_step_at_active_degree_replays_the_eager_image():
  """Under capture the SH colours are evaluated by ms_frame_sh_colours on the executor's side stream: it must honour the
  descriptor field too."""
  assert frame.SH_SIDE_STREAM
  g, cam = frame_scene(torch.float32)
  gd = g.clone().requires_grad_(True)
  leaves = [gd.position, gd.log_scaling, gd.rotation, gd.alpha_logit, gd.feature]
  cfg = RasterConfig(tile_size=16)

  def step():
    for t in leaves:
      t.grad = None
    r = render_gaussians(gd, cam, cfg, use_sh=True, sh_degree=1)
    r.image.sum().backward()
    return r

  def eager_image():
    with torch.no_grad():
      return render_gaussians(gd, cam, cfg, use_sh=True, sh_degree=1).image.clone()

  want = eager_image()
  full = render_gaussians(g, cam, cfg, use_sh=True).image
  assert (want - full).abs().max().item() > 1e-3            # the higher bands do show in this scene
  graph = frame.FrameGraph(step, warmup=2)
  r = graph.replay()
  torch.cuda.synchronize()
  assert r.frame.colours_ready is not None                  # the side-stream route was taken
  assert torch.equal(r.image, want)
  assert bool((gd.feature.grad[:, :, 4:] == 0).all()) and float(gd.feature.grad[:, :, :4].abs().max()) > 0
  with torch.no_grad():
    gd.feature.mul_(-0.7)
  r = graph.replay()
  torch.cuda.synchronize()
  moved = eager_image()
  assert (moved - want).abs().max().item() > 1e-3
  assert torch.equal(r.image, moved)
  assert not frame.frame_status(r)['overflow']


def test_training_step_at_degree_1_leaves_the_higher_bands_alone():
  """render -> loss -> backward -> VisibilityAwareAdam dense step at sh_degree=1 on a degree-3 scene whose higher bands
  hold values: they and their optimiser moments are bit-unchanged, the active coefficients move."""
  from taichi_splatting_amd.optim import VisibilityAwareAdam
  g, cam = frame_scene(torch.float32)
  feature = g.feature.clone().requires_grad_(True)
  gd = g.replace(feature=feature)
  before = feature.detach().clone()
  assert float(before[:, :, 4:].abs().min()) > 0
  opt = VisibilityAwareAdam([dict(params=[feature], lr=0.01, name='feature', type='scalar')])
  cfg = RasterConfig(tile_size=16, compute_visibility=True, compute_point_heuristic=True)
  r = render_gaussians(gd, cam, cfg, use_sh=True, sh_degree=1)
  target = torch.rand(SIZE[1], SIZE[0], 3, generator=torch.Generator().manual_seed(2)).to(DEV)
  poison(feature)
  (r.image - target).abs().mean().backward()
  visibility = frame.point_outputs(r)['visibility']
  opt.step(None, visibility)
  torch.cuda.synchronize()
  after = feature.detach()
  assert torch.equal(after[:, :, 4:], before[:, :, 4:])
  seen = visibility > 1e-8
  assert int(seen.sum()) > 100
  moved = (after[:, :, :4] != before[:, :, :4]).flatten(1).any(dim=1)
  assert int(moved.sum()) > 100 and not bool((moved & ~seen).any())      # visible gaussians moved, and only they
  state = opt.state[feature]
  for key in ('v', 'm'):
    moment = state[key].view(N, 3, 16)
    assert bool((moment[:, :, 4:] == 0).all()), key
    assert float(moment[:, :, :4].abs().max()) > 0, key
