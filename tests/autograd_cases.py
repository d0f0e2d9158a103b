"""Scenes, float64 truth and comparison helpers of tests/test_gpu_autograd_contract.py (nothing here needs a GPU;
tests/test_autograd_cases_host.py checks the scenes with the oracle alone).

What is under test is the layer ABOVE the kernels: the ``torch.autograd.Function`` wrappers decide which buffers are
``torch.empty`` and which ``torch.zeros``, which pointers are NULL, what a ``None`` or an expanded upstream gradient
becomes and what a second backward over one graph does.  So everything here is phrased as autograd: a loss is a
function of an ``out`` namespace (image, image_weight, gaussians2d, depths, features, idx), evaluated once on the
kernels' outputs and once on the oracle's, and truth is float64 torch autograd through ``oracle.projection``,
``oracle.sh``, ``oracle.mapper`` and the oracle rasterizer.  The rasterizer enters autograd as ONE node made of
``oracle.raster.forward`` / ``oracle.raster.backward`` — the pair tests/test_gpu_render.py::oracle_render_with_grads
and tests/test_gpu_configs.py::oracle_frame chain by hand, which also yields the point heuristics — and the host test
holds that node to ``oracle.raster.rasterize_autograd`` and to ``oracle_render_with_grads`` on these scenes.

Shapes: n = 300 gaussians (one full 256-thread block and a last wave of 44) in front of a 64 x 48 camera at tile 16
(12 tiles, the bottom row partial).  Scene 'culled' scatters them with margin 0.6 (48 of the 300 rows are
culled), scene 'all' with margin 0 (every row visible: the ``empty_like`` branch of the projection backward and
``all_rows_written`` of the SH backward).  Every value is float32-representable, so the float32 and the float64 kernels
and the oracle see the same inputs.  A pool of 400 gaussians is drawn and the ones with a (pixel, splat) pair within
1e-4 of the blend gate — plain or antialiased — are dropped before the first 300 are taken (the gate margin of a splat
does not depend on the other splats), as tests/test_gpu_raster.py::gate_stable does."""
import functools
import types

import numpy as np
import torch

from oracle import mapper as omap, projection as oproj, raster as orast, sh as osh
from taichi_splatting_amd import RasterConfig
from taichi_splatting_amd.testing import random_camera, random_3d_gaussians

N, POOL = 300, 400
SIZE = (64, 48)
TILE = 16
GATE_MARGIN = 1e-4
LEAVES = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')
CAMERA_LEAVES = ('T_camera_world', 'projection')
ALL_LEAVES = LEAVES + CAMERA_LEAVES
PROJECTION_LEAVES = LEAVES[:4] + CAMERA_LEAVES
SH_LEAVES = ('feature', 'position', 'camera_position')
RASTER_LEAVES = ('gaussians2d', 'features')
ILL_CONDITIONED_F32 = ('position', 'log_scaling', 'rotation') + CAMERA_LEAVES   # behind a float32 projection backward
# (margin of random_3d_gaussians, seed): picked so that the conditions of tests/test_autograd_cases_host.py hold
SCENES = {'culled': (0.6, 3), 'all': (0.0, 4)}
FEATURES = {'rgb': 3, 'c4': 4, 'c9': 9, 'sh3': 3}


def config(antialias=False, heuristic=False, visibility=False):
  return RasterConfig(tile_size=TILE, antialias=antialias, compute_point_heuristic=heuristic, compute_visibility=visibility)


def tile_lists(points, depths, camera, cfg):
  """(overlap_to_point, tile_ranges) of the oracle mapper, float32 keys like the kernels'"""
  ndc = oproj.ndc_depth(depths.detach().double(), *camera.depth_range)
  o2p, ranges, _ = omap.map_to_tiles(points.detach().numpy().astype(np.float32), ndc.numpy().astype(np.float32), SIZE,
                                     cfg.tile_size, cfg.alpha_threshold)
  return torch.from_numpy(o2p), torch.from_numpy(ranges)


def project(g, camera, cfg):
  return oproj.apply(g.position, g.log_scaling, g.rotation, g.alpha_logit, camera.T_camera_world, camera.projection, SIZE,
                     camera.depth_range, cfg.blur_cov, cfg.clamp_margin, cfg.alpha_threshold)


@functools.lru_cache(maxsize=None)
def geometry(kind):
  """(the 300 gate-stable gaussians with their RGB colours, camera, share of the pool's splats that survived): float32
  on the CPU, never modified."""
  margin, seed = SCENES[kind]
  torch.manual_seed(seed)
  camera = random_camera(image_size=SIZE)
  pool = random_3d_gaussians(POOL, camera, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=margin)
  g64, cam64 = pool.to(dtype=torch.float64), camera.to(dtype=torch.float64)
  keep = torch.ones(POOL, dtype=torch.bool)
  survived = []
  for antialias in (False, True):
    cfg = config(antialias=antialias)
    points, depths, idx = project(g64, cam64, cfg)
    o2p, ranges = tile_lists(points, depths, cam64, cfg)
    stable = orast.gate_margin(points, ranges, o2p, SIZE, cfg) > GATE_MARGIN
    keep[idx[~stable]] = False
    survived.append(float(stable.double().mean()))
  assert int(keep.sum()) >= N, (kind, int(keep.sum()))
  return pool[keep][:N], camera, min(survived)


@functools.lru_cache(maxsize=None)
def scene(kind, features='rgb', dtype=torch.float64):
  """(Gaussians3D, CameraParams) on the CPU in ``dtype``; 'rgb' / 'c4' / 'c9': plain colours of 3 / 4 / 9 channels,
  'sh3': RGB coefficients of degree 3, 0.5 randn (some colours clamp)."""
  g, camera, _ = geometry(kind)
  gen = torch.Generator().manual_seed(17)
  if features == 'sh3':
    g = g.replace(feature=0.5 * torch.randn(N, 3, 16, generator=gen))
  elif features != 'rgb':
    g = g.replace(feature=torch.rand(N, FEATURES[features], generator=gen))
  return g.to(dtype=dtype), camera.to(dtype=dtype)


@functools.lru_cache(maxsize=None)
def culled_rows(kind):
  """(N,) bool on the CPU, never modified: the rows the float64 oracle culls"""
  g, camera = scene(kind)
  visible = torch.zeros(N, dtype=torch.bool)
  visible[project(g, camera, config())[2]] = True
  return ~visible


def sh_clamp_margin(kind):
  """smallest distance of a pre-clamp SH colour of the visible gaussians from 0 and from 1"""
  g, camera = scene(kind, 'sh3')
  idx = project(g, camera, config())[2]
  dirs = g.position[idx] - torch.inverse(camera.T_camera_world)[:3, 3]
  dirs = dirs / dirs.norm(dim=1, keepdim=True)
  pre = (osh.rsh_cart(dirs, 3).unsqueeze(1) * g.feature[idx]).sum(-1) + 0.5
  return torch.minimum(pre.abs(), (pre - 1).abs()).min().item()


# ---- constants of the losses ---------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def constants(channels, dtype=torch.float64, device='cpu'):
  """Weights of the losses: G (H, W, C) on the image, M a 0/1 mask that splits it, target an image in [0, 1], and one
  row per GAUSSIAN for the losses on ``points`` (D depth, P gaussians2d, F features), indexed by ``out.idx``."""
  gen = torch.Generator().manual_seed(23)
  w, h = SIZE
  rand = lambda *s: torch.rand(*s, generator=gen, dtype=torch.float64)
  k = dict(G=rand(h, w, channels) + 0.5, M=(rand(h, w, 1) < 0.5).double(), target=rand(h, w, channels),
           D=rand(N, 1) + 0.5, P=rand(N, 7) + 0.5, F=rand(N, channels) + 0.5, ones=torch.ones(h, w, channels, dtype=torch.float64),
           O=rand(400, 3) + 0.5)
  return types.SimpleNamespace(**{name: t.to(dtype=dtype, device=device) for name, t in k.items()})


def _k(out):
  return constants(out.image.shape[-1], out.image.dtype, str(out.image.device))


LOSSES = {
  'weighted': lambda o: (o.image * _k(o).G).sum(),
  'sum': lambda o: o.image.sum(),                                           # an expanded scalar reaches the backward
  'ones': lambda o: (o.image * _k(o).ones).sum(),                           # the same loss, materialised upstream
  'permuted': lambda o: (o.image.permute(2, 0, 1)[1] * _k(o).G[:, :, 1]).sum(),     # non-contiguous dL/dimage
  'strided': lambda o: (o.image[::2, ::3] * _k(o).G[::2, ::3]).sum(),
  'half_a': lambda o: (o.image * _k(o).G * _k(o).M).sum(),                  # half_a + half_b = weighted
  'half_b': lambda o: (o.image * _k(o).G * (1 - _k(o).M)).sum(),
  'depths': lambda o: (o.depths * _k(o).D[o.idx]).sum(),                    # g_image is None from here on
  'gaussians2d': lambda o: (o.gaussians2d * _k(o).P[o.idx]).sum(),
  'features': lambda o: (o.features * _k(o).F[o.idx]).sum(),
  'mixed': lambda o: (o.image * _k(o).G).sum() + (o.depths * _k(o).D[o.idx]).sum() + (o.gaussians2d * _k(o).P[o.idx]).sum(),
}


def photometric_truth_loss(o):
  from .photometric_oracle import loss_terms
  return loss_terms(o.image, _k(o).target)[0]


# ---- float64 truth -------------------------------------------------------------------------------------------------------

class OracleRaster(torch.autograd.Function):
  """``oracle.raster.forward`` / ``backward`` as one autograd node.  ``record['heuristic']`` holds the (V, 2) point
  heuristics of the most recent backward pass."""

  @staticmethod
  def forward(ctx, points, feats, ranges, o2p, cfg, record):
    image, alpha, visibility = orast.forward(points.detach(), feats.detach(), ranges, o2p, SIZE, cfg)
    ctx.set_materialize_grads(False)
    ctx.args = (ranges, o2p, cfg, record)
    ctx.save_for_backward(points.detach(), feats.detach(), image)
    ctx.mark_non_differentiable(alpha, visibility)
    return image, alpha, visibility

  @staticmethod
  def backward(ctx, g_image, g_alpha, g_visibility):
    if g_image is None:
      return (None,) * 6
    points, feats, image = ctx.saved_tensors
    ranges, o2p, cfg, record = ctx.args
    grad_points, grad_feats, record['heuristic'] = orast.backward(points, feats, ranges, o2p, image, g_image.contiguous(),
                                                                  SIZE, cfg)
    return grad_points, grad_feats, None, None, None, None


def oracle_raster(points, feats, ranges, o2p, cfg):
  record = {}
  image, alpha, visibility = OracleRaster.apply(points, feats, ranges, o2p, cfg, record)
  return types.SimpleNamespace(image=image, image_weight=alpha, visibility=visibility, record=record)


def oracle_frame(leaves, depth_range, cfg, use_sh):
  """The render path of the oracle on a dict of the seven leaves, differentiable in all of them (renderer.py:23-108: the
  SH direction sees the gaussians' positions detached, the camera's not)."""
  pos, T = leaves['position'], leaves['T_camera_world']
  points, depths, idx = oproj.apply(pos, leaves['log_scaling'], leaves['rotation'], leaves['alpha_logit'], T,
                                    leaves['projection'], SIZE, depth_range, cfg.blur_cov, cfg.clamp_margin, cfg.alpha_threshold)
  feature = leaves['feature']
  feats = osh.evaluate_sh_at(feature, pos.detach(), idx, torch.inverse(T)[0:3, 3]) if use_sh else feature[idx]
  camera = types.SimpleNamespace(depth_range=depth_range)
  o2p, ranges = tile_lists(points, depths, camera, cfg)
  out = oracle_raster(points, feats, ranges, o2p, cfg)
  out.gaussians2d, out.depths, out.features, out.idx, out.o2p, out.ranges = points, depths, feats, idx, o2p, ranges
  return out


def scene_leaves(kind, features, dtype=torch.float64, device='cpu', requires=ALL_LEAVES):
  """fresh copies of the seven leaves of a scene; ``requires``: the names that require grad"""
  g, camera = scene(kind, features, dtype)
  values = dict(position=g.position, log_scaling=g.log_scaling, rotation=g.rotation, alpha_logit=g.alpha_logit,
                feature=g.feature, T_camera_world=camera.T_camera_world, projection=camera.projection)
  return {name: t.detach().clone().to(device).requires_grad_(name in requires) for name, t in values.items()}


def grads_of(leaves, names=None):
  return {name: (t.grad if t.grad is not None else torch.zeros_like(t)).detach().clone()
          for name, t in leaves.items() if (names is None or name in names)}


def _loss_fn(loss):
  return photometric_truth_loss if loss == 'photometric' else LOSSES[loss]


@functools.lru_cache(maxsize=None)
def frame_truth(kind, features, loss, antialias=False):
  """float64 oracle of a whole frame under ``loss``: image, image_weight, visibility, idx, the seven gradients, the point
  heuristics of ONE backward pass scattered to (N, 2), and the gradients in front of the projection / SH backward
  (``upstream``: points, depths, feats or None).  One backward per (scene, features, loss), shared by every subset."""
  _, camera = scene(kind, features)
  cfg = config(antialias=antialias)
  leaves = scene_leaves(kind, features)
  out = oracle_frame(leaves, camera.depth_range, cfg, features == 'sh3')
  boundary = [out.gaussians2d, out.depths] + ([out.features] if features == 'sh3' else [])
  for t in boundary:
    t.retain_grad()
  _loss_fn(loss)(out).backward()
  heuristic = torch.zeros(N, 2, dtype=torch.float64)
  if 'heuristic' in out.record:
    heuristic[out.idx] = out.record['heuristic']
  visibility = torch.zeros(N, dtype=torch.float64)
  visibility[out.idx] = out.visibility
  return types.SimpleNamespace(image=out.image.detach(), image_weight=out.image_weight, visibility=visibility, idx=out.idx,
                               grads=grads_of(leaves), heuristic=heuristic, gaussians2d=out.gaussians2d.detach(),
                               depths=out.depths.detach(), features=out.features.detach(), o2p=out.o2p, ranges=out.ranges,
                               upstream=[t.grad for t in boundary] + ([None] if features != 'sh3' else []))


def chain_grads(kind, features, dtype, upstream):
  """The oracle's projection (and SH) backward alone, in ``dtype`` (torch on the CPU), for GIVEN gradients of its outputs
  ``upstream`` = (d gaussians2d (V, 7), d depths (V, 1), d colours (V, 3) of an SH scene), each possibly None: float64 =
  the exact chain behind those gradients, float32 = what the reference's arithmetic reaches at the product's precision
  (tests/test_gpu_configs.py::oracle_leaf_grads).  The modular float32 projection backward is judged on ITS inputs this
  way, as tests/test_gpu_projection_sh.py::test_projection_f32_backward_vs_oracle judges it.  Dict of the seven gradients
  as float64."""
  _, camera = scene(kind, features)
  cfg = config()
  leaves = scene_leaves(kind, features, dtype)
  pos, T = leaves['position'], leaves['T_camera_world']
  points, depths, idx = oproj.apply(pos, leaves['log_scaling'], leaves['rotation'], leaves['alpha_logit'], T,
                                    leaves['projection'], SIZE, camera.depth_range, cfg.blur_cov, cfg.clamp_margin,
                                    cfg.alpha_threshold)
  assert idx.shape[0] == frame_truth(kind, features, 'weighted').idx.shape[0], (kind, dtype, 'other rows culled')
  outputs = [points, depths]
  if features == 'sh3':
    outputs.append(osh.evaluate_sh_at(leaves['feature'], pos.detach(), idx, torch.inverse(T)[0:3, 3]))
  pairs = [(o, u.detach().cpu().to(dtype)) for o, u in zip(outputs, upstream) if u is not None]
  if pairs:
    torch.autograd.backward([o for o, _ in pairs], [u for _, u in pairs])
  return {name: g.double() for name, g in grads_of(leaves).items()}


@functools.lru_cache(maxsize=None)
def raster_inputs(kind, features):
  """What the 2D operators are given: the oracle's projected splats rounded to float32 (as float64 tensors), their
  colours, the NDC depths the tile lists are sorted by, and the oracle mapper's lists for exactly those values."""
  g, camera = scene(kind, features)
  cfg = config()
  with torch.no_grad():
    out = oracle_frame(scene_leaves(kind, features, requires=()), camera.depth_range, cfg, features == 'sh3')
  points, feats = out.gaussians2d.float().double(), out.features.float().double()
  ndc = oproj.ndc_depth(out.depths, *camera.depth_range).float().double()
  o2p, ranges, _ = omap.map_to_tiles(points.numpy().astype(np.float32), ndc.numpy().astype(np.float32), SIZE, TILE,
                                     cfg.alpha_threshold)
  return types.SimpleNamespace(gaussians2d=points, features=feats, depth=ndc, o2p=torch.from_numpy(o2p),
                               ranges=torch.from_numpy(ranges).view(-1, 2))


@functools.lru_cache(maxsize=None)
def raster_truth(kind, features, loss, antialias=False):
  """float64 oracle of the 2D operators on ``raster_inputs``: image, image_weight, visibility, the two gradients and the
  (V, 2) heuristics of one backward pass"""
  x = raster_inputs(kind, features)
  leaves = dict(gaussians2d=x.gaussians2d.clone().requires_grad_(True), features=x.features.clone().requires_grad_(True))
  out = oracle_raster(leaves['gaussians2d'], leaves['features'], x.ranges, x.o2p, config(antialias=antialias))
  _loss_fn(loss)(out).backward()
  return types.SimpleNamespace(image=out.image.detach(), image_weight=out.image_weight, visibility=out.visibility,
                               grads=grads_of(leaves), heuristic=out.record['heuristic'])


@functools.lru_cache(maxsize=None)
def projection_truth(kind, upstream, dtype=torch.float64):
  """The oracle projection in ``dtype`` under a loss on ``upstream`` in ('both', 'points', 'depth'): (points, depth, idx,
  dict of the six gradients as float64)"""
  _, camera = scene(kind)
  cfg = config()
  leaves = {k: v for k, v in scene_leaves(kind, 'rgb', dtype).items() if k in PROJECTION_LEAVES}
  points, depth, idx = oproj.apply(*[leaves[k] for k in PROJECTION_LEAVES], SIZE, camera.depth_range, cfg.blur_cov,
                                   cfg.clamp_margin, cfg.alpha_threshold)
  projection_loss(points, depth, idx, upstream).backward()
  return points.detach(), depth.detach(), idx, {k: g.double() for k, g in grads_of(leaves).items()}


def projection_loss(points, depth, idx, upstream):
  k = constants(3, points.dtype, str(points.device))
  terms = []
  if upstream in ('both', 'points'):
    terms.append((points * k.P[idx]).sum())
  if upstream in ('both', 'depth'):
    terms.append((depth * k.D[idx]).sum())
  return sum(terms)


@functools.lru_cache(maxsize=None)
def sh_indexes(kind, which):
  """'unique': the visible gaussians of the scene in storage order (all 300 on scene 'all'); 'repeated': 400 draws"""
  if which == 'unique':
    g, camera = scene(kind)
    return project(g, camera, config())[2]
  return torch.randint(0, N, (400,), generator=torch.Generator().manual_seed(31))


def sh_camera_position(kind):
  """the camera position of the scene rounded to float32 (float64 tensor): one value for both dtypes and the oracle"""
  return torch.inverse(scene(kind)[1].T_camera_world)[:3, 3].float().double()


def sh_loss(out, loss):
  """sum(out * O), or one of its two halves (even / odd rows)"""
  k = constants(3, out.dtype, str(out.device))
  weighted = out * k.O[:out.shape[0]]
  return {'weighted': weighted, 'half_a': weighted[0::2], 'half_b': weighted[1::2]}[loss].sum()


@functools.lru_cache(maxsize=None)
def sh_truth(kind, which, loss='weighted'):
  """oracle.sh.evaluate_sh_at on the degree-3 scene under ``sh_loss``: (out, dict of the three gradients)"""
  g, camera = scene(kind, 'sh3')
  idx = sh_indexes(kind, which)
  leaves = dict(feature=g.feature.clone().requires_grad_(True), position=g.position.clone().requires_grad_(True),
                camera_position=sh_camera_position(kind).requires_grad_(True))
  out = osh.evaluate_sh_at(leaves['feature'], leaves['position'], idx, leaves['camera_position'])
  sh_loss(out, loss).backward()
  return out.detach(), grads_of(leaves)


# ---- comparisons (the project's own tolerances; none is new) ---------------------------------------------------------------

def assert_f64_gradient(got, want, what, atol=1e-8):
  """tests/test_gpu_raster.py::test_forward_backward_f64: 1e-8 of max(1, largest) + 1e-7 relative for the gaussians'
  gradients, 1e-9 absolute for the colours'"""
  got = got.detach().cpu().double()
  scale = max(1.0, want.abs().max().item()) if atol == 1e-8 else 1.0
  err = (got - want).abs().max().item()
  assert got.shape == want.shape and torch.allclose(got, want, atol=atol * scale, rtol=1e-7), (what, err, scale)


def assert_f64_heuristic(got, want, what):
  got = got.detach().cpu().double()
  scale = max(1.0, want.abs().max().item())
  assert torch.allclose(got, want, atol=1e-7 * scale, rtol=1e-6), (what, (got - want).abs().max().item(), scale)


def assert_gradient(name, got, want, dtype, what, w32=None, w64=None):
  """One returned gradient against the float64 oracle's, by the tolerance its dtype and its leaf have."""
  from .test_gpu_raster import assert_within
  from .test_gpu_projection_sh import assert_f32_gradient_as_accurate_as_reference
  assert got is not None, (what, name, 'no gradient')
  assert got.shape == want.shape and bool(torch.isfinite(got).all()), (what, name, 'shape / finite')
  err = (got.detach().cpu().double() - want).abs().max().item()
  print(f"{what} {name}: max err {err:.3e} of scale {want.abs().max().item():.3e}")
  if float(want.abs().max()) == 0.0:
    assert float(got.abs().max()) == 0.0, (what, name, 'the loss does not depend on this leaf', err)
  elif dtype == torch.float64:
    assert_f64_gradient(got, want, (what, name), atol=1e-9 if name in ('features',) else 1e-8)
  elif w32 is not None and name in w32:
    exact = want if w64 is None else w64[name]           # (the exact chain behind the upstream gradients w32 was given)
    assert_f32_gradient_as_accurate_as_reference(got.detach().cpu(), exact, w32[name], (what, name))
  else:
    assert_within(got.detach(), want, 1e-4, (what, name))


def assert_same_gradient(name, got, full, dtype, exact, what):
  """A subset's gradient against the all-leaves backward of the same forward: bit for bit where no float atomic is
  involved, else by the atomic-noise criterion of tests/test_gpu_frame.py::assert_grads_close."""
  from .test_gpu_frame import assert_grads_close
  if exact:
    assert torch.equal(got, full), (what, name, 'not bit-identical', (got - full).abs().max().item())
  else:
    assert_grads_close([got], [full], tol=1e-9 if dtype == torch.float64 else 2e-5)


def poison(*tensors):
  """freed NaN blocks where the next allocations of these sizes will land (tests/test_gpu_sh_active.py::poison)"""
  from .test_gpu_sh_active import poison as poison_one
  for t in tensors:
    poison_one(t)


def subsets(names):
  """every single leaf, and all but one leaf"""
  singles = [(n,) for n in names]
  if len(names) <= 2:
    return singles
  return singles + [tuple(m for m in names if m != n) for n in names]
