"""-m gpu: the wide-feature rasteriser (csrc/raster_wide.hip, rasterize_wide / render_features) against the float64
oracle, the chunked path and the modular composition.

Tolerances are those of tests/test_gpu_raster.py for float32 raster kernels: 1e-4 absolute on pixels and image_weight,
1e-4 of the largest gradient entry on gradients, for EVERY pixel and EVERY splat, on gate-stable scenes (splats with a
(pixel, splat) pair within 1e-4 relative of the blend gate are removed beforehand, more than 70 % must remain)."""
import pytest
import torch

from oracle import mapper as omap, raster as orast
from taichi_splatting_amd import (RasterConfig, frame, rasterize_wide, rasterize_with_tiles, render_features,
                                  render_gaussians)
from taichi_splatting_amd.mapper.tile_mapper import map_to_tiles_strip
from taichi_splatting_amd.misc.renderer2d import project_gaussians2d
from taichi_splatting_amd.testing import random_2d_gaussians, random_3d_gaussians, random_camera

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CFG = RasterConfig(tile_size=16)
TOL = 1e-4


def gate_stable(g, size, cfg, rel_margin=1e-4):
  """The 2D gaussians of ``g`` that have no (pixel, splat) pair within ``rel_margin`` of the blend gate."""
  p = project_gaussians2d(g)
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), g.depths.numpy(), size, cfg.tile_size)
  margin = orast.gate_margin(p.double(), torch.from_numpy(ranges), torch.from_numpy(o2p), size, cfg)
  keep = margin > rel_margin
  assert keep.float().mean() > 0.7
  return g[keep]


def scene(n, size, seed, scale=1.0, alpha=(0.1, 0.9)):
  """gate-stable (points7, depths, overlap_to_point, tile_ranges) on the CPU, lists from the oracle mapper"""
  torch.manual_seed(seed)
  g = gate_stable(random_2d_gaussians(n, size, scale_factor=scale, alpha_range=alpha), size, CFG)
  p = project_gaussians2d(g)
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), g.depths.numpy(), size, CFG.tile_size)
  return p, g.depths, torch.from_numpy(o2p), torch.from_numpy(ranges)


def features_for(n, f, seed=0):
  return torch.rand((n, f), generator=torch.Generator().manual_seed(1000 + seed + f))


def assert_within(got, want, tol, what, rows=None):
  got, want = got.cpu().double(), want.cpu().double()
  scale = want.abs().max().item()
  if rows is not None:
    got, want = got[rows], want[rows]
  err = (got - want).abs().max().item() if want.numel() else 0.0
  print(f"{what}: max error {err:.3e}, largest entry {scale:.3e}, ratio {err / max(scale, 1e-30):.3e}")
  assert err < tol * max(scale, 1e-30), (what, err, scale)


def run_wide(p, f, o2p, ranges, size, G=None, grad_p=True, grad_f=True):
  pg, fg = p.to(DEV).requires_grad_(grad_p), f.to(DEV).requires_grad_(grad_f)
  out = rasterize_wide(pg, fg, o2p.to(DEV), ranges.to(DEV).view(-1, 2), size, CFG)
  if G is not None and (grad_p or grad_f):
    (out.image * G.to(DEV)).sum().backward()
  return out, pg.grad, fg.grad


def check_against_oracle(p, f, o2p, ranges, size, seed=0, rows=None):
  w, h = size
  img_o, a_o, _ = orast.forward(p.double(), f.double(), ranges, o2p, size, CFG)
  G = torch.randn(img_o.shape, generator=torch.Generator().manual_seed(seed), dtype=torch.float64)
  gp_o, gf_o, _ = orast.backward(p.double(), f.double(), ranges, o2p, img_o, G, size, CFG)
  out, gp, gf = run_wide(p, f, o2p, ranges, size, G.float())
  assert out.image.shape == (h, w, f.shape[1]) and out.image_weight.shape == (h, w)
  assert out.point_heuristic.shape == (0, 2) and out.visibility.shape == (0,)
  err_i = (out.image.cpu().double() - img_o).abs().max().item()
  err_a = (out.image_weight.cpu().double() - a_o).abs().max().item()
  print(f"F = {f.shape[1]}: image max error {err_i:.3e}, image_weight max error {err_a:.3e}")
  assert err_i < TOL and err_a < TOL
  assert_within(gp, gp_o, TOL, 'd gaussians2d', rows)
  assert_within(gf, gf_o, TOL, 'd features', rows)
  return out


_scenes = {}
def shared_scene(*key, **kw):
  """built once, shared by the tests that need it, never modified"""
  k = (key, tuple(sorted(kw.items())))
  if k not in _scenes:
    _scenes[k] = scene(*key, **kw)
  return _scenes[k]


# ---- 1. widths: every channel-block count, widths that are no multiple of 32, an image that is no multiple of 16
@pytest.mark.parametrize('f', [5, 32, 33, 40, 64, 128])
def test_widths_against_the_oracle(f):
  if f == 128:
    size, (p, d, o2p, ranges) = (70, 50), shared_scene(600, (70, 50), 3, scale=1.5)
  else:
    size, (p, d, o2p, ranges) = (150, 100), shared_scene(1500, (150, 100), 2, scale=1.5)
  check_against_oracle(p, features_for(p.shape[0], f), o2p, ranges, size, seed=f)


# ---- 2. long runs and saturation: several staged batches per tile, the odd-hit tail, the backward's saturation drop
def test_long_runs_and_saturation():
  size = (64, 64)
  p, d, o2p, ranges = shared_scene(6000, size, 11, scale=6.0, alpha=(0.6, 1.0))
  runs = ranges.view(-1, 2)
  assert int((runs[:, 1] - runs[:, 0]).min()) > 500
  margin, _ = orast.saturation_margin(p.double(), ranges, o2p, size, CFG)
  rows = margin >= 1e-4            # a float32 T may fall on the other side of the saturation test within that margin
  left_out = 1.0 - rows.float().mean().item()
  print(f"rows left out of the gradient comparison: {100 * left_out:.3f} %")
  assert left_out <= 0.01
  out = check_against_oracle(p, features_for(p.shape[0], 40), o2p, ranges, size, seed=1, rows=rows)
  assert float(out.image_weight.min()) > 0.99


# ---- 3. tiny lists
def one_splat(x, y, alpha=0.7):
  return torch.tensor([x, y, 1.0, 0.0, 2.5, 1.5, alpha])


@pytest.mark.parametrize('f', [32, 7])
def test_tiny_lists(f):
  # one splat on a (20, 9) image: two tiles with one entry each
  p = one_splat(15.6, 4.2)[None]
  o2p = torch.tensor([0, 0], dtype=torch.int32)
  ranges = torch.tensor([[0, 1], [1, 2]], dtype=torch.int32)
  check_against_oracle(p, features_for(1, f), o2p, ranges, (20, 9), seed=1)
  # three splats in one (16, 16) tile: an odd hit count
  p = torch.stack([one_splat(4.3, 5.1, 0.5), one_splat(9.7, 8.2, 0.8), one_splat(7.1, 11.4, 0.3)])
  o2p = torch.tensor([0, 1, 2], dtype=torch.int32)
  ranges = torch.tensor([[0, 3]], dtype=torch.int32)
  check_against_oracle(p, features_for(3, f), o2p, ranges, (16, 16), seed=2)
  # mostly empty tile ranges
  size = (160, 128)
  centres = [(10.3, 12.7), (11.9, 14.2), (75.2, 40.6), (140.4, 100.9), (141.7, 99.3), (30.5, 110.1)]
  p = torch.stack([one_splat(x, y, 0.3 + 0.1 * i) for i, (x, y) in enumerate(centres)])
  depths = torch.linspace(0.1, 0.9, len(centres))
  o2p, ranges, _ = omap.map_to_tiles(p.numpy(), depths.numpy(), size, 16)
  o2p, ranges = torch.from_numpy(o2p), torch.from_numpy(ranges)
  assert float(orast.gate_margin(p.double(), ranges, o2p, size, CFG).min()) > 1e-4          # gate-stable as it stands
  assert ((ranges.view(-1, 2)[:, 1] - ranges.view(-1, 2)[:, 0]) == 0).float().mean() > 0.5
  check_against_oracle(p, features_for(p.shape[0], f), o2p, ranges, size, seed=3)


@pytest.mark.parametrize('v', [0, 5])
def test_empty_inputs_render_zeros(v):
  size = (40, 24)
  p = torch.stack([one_splat(5.0 + i, 6.0) for i in range(v)]) if v else torch.zeros((0, 7))
  f = features_for(v, 7)
  o2p = torch.zeros((0,), dtype=torch.int32)
  ranges = torch.zeros((6, 2), dtype=torch.int32)
  out, gp, gf = run_wide(p, f, o2p, ranges, size, torch.ones((24, 40, 7)))
  assert float(out.image.abs().max()) == 0.0 and float(out.image_weight.abs().max()) == 0.0
  assert gp.shape == (v, 7) and gf.shape == (v, 7)
  assert float(gp.abs().sum()) == 0.0 and float(gf.abs().sum()) == 0.0


# ---- 4. the forward is bitwise reproducible, and channel blocks are independent MFMA tiles
def test_forward_is_bitwise_reproducible():
  size = (150, 100)
  p, d, o2p, ranges = shared_scene(1500, size, 2, scale=1.5)
  f33 = features_for(p.shape[0], 33)
  a, _, _ = run_wide(p, f33, o2p, ranges, size)
  b, _, _ = run_wide(p, f33, o2p, ranges, size)
  assert torch.equal(a.image, b.image) and torch.equal(a.image_weight, b.image_weight)
  c, _, _ = run_wide(p, f33[:, :32].contiguous(), o2p, ranges, size)
  assert torch.equal(a.image[:, :, :32], c.image) and torch.equal(a.image_weight, c.image_weight)
  f32 = torch.zeros((p.shape[0], 32))
  f32[:, :5] = f33[:, :5]
  e, _, _ = run_wide(p, f32, o2p, ranges, size)
  g, _, _ = run_wide(p, f33[:, :5].contiguous(), o2p, ranges, size)
  assert torch.equal(e.image[:, :, :5], g.image)
  assert float(e.image[:, :, 5:].abs().max()) == 0.0


# ---- 5. agreement with the chunked path
@pytest.mark.parametrize('f', [8, 64])
def test_agrees_with_the_chunked_path(f):
  size = (150, 100)
  p, d, o2p, ranges = shared_scene(1500, size, 2, scale=1.5)
  feats = features_for(p.shape[0], f)
  G = torch.randn((100, 150, f), generator=torch.Generator().manual_seed(f))
  wide, gp_w, gf_w = run_wide(p, feats, o2p, ranges, size, G)
  pg, fg = p.to(DEV).requires_grad_(True), feats.to(DEV).requires_grad_(True)
  chunked = rasterize_with_tiles(pg, fg, o2p.to(DEV), ranges.to(DEV).view(-1, 2), size, CFG)
  (chunked.image * G.to(DEV)).sum().backward()
  assert float((wide.image - chunked.image).abs().max()) < TOL
  assert float((wide.image_weight - chunked.image_weight).abs().max()) < TOL
  assert_within(gp_w, pg.grad, TOL, 'd gaussians2d')
  assert_within(gf_w, fg.grad, TOL, 'd features')


# ---- 6. autograd contract
def test_autograd_contract():
  size = (150, 100)
  p, d, o2p, ranges = shared_scene(1500, size, 2, scale=1.5)
  f = features_for(p.shape[0], 40)
  G = torch.randn((100, 150, 40), generator=torch.Generator().manual_seed(7))
  _, gp, gf = run_wide(p, f, o2p, ranges, size, G)

  _, none_p, only_f = run_wide(p, f, o2p, ranges, size, G, grad_p=False)       # the geometry part is skipped
  assert none_p is None
  assert_within(only_f, gf, 1e-5, 'd features (features only)')
  only_p, none_f = run_wide(p, f, o2p, ranges, size, G, grad_f=False)[1:]
  assert none_f is None
  assert_within(only_p, gp, 1e-5, 'd gaussians2d (gaussians2d only)')
  out, a, b = run_wide(p, f, o2p, ranges, size, G, grad_p=False, grad_f=False)
  assert a is None and b is None and not out.image.requires_grad

  # two backward passes over one graph: the same gradients within the atomics' noise
  pg, fg = p.to(DEV).requires_grad_(True), f.to(DEV).requires_grad_(True)
  out = rasterize_wide(pg, fg, o2p.to(DEV), ranges.to(DEV).view(-1, 2), size, CFG)
  loss = (out.image * G.to(DEV)).sum()
  first = torch.autograd.grad(loss, (pg, fg), retain_graph=True)
  second = torch.autograd.grad(loss, (pg, fg), retain_graph=True)
  assert_within(second[0], first[0], 1e-5, 'd gaussians2d (second backward)')
  assert_within(second[1], first[1], 1e-5, 'd features (second backward)')

  # a non-contiguous dL/dimage
  Gt = G.to(DEV).permute(2, 0, 1).contiguous().permute(1, 2, 0)
  assert not Gt.is_contiguous()
  third = torch.autograd.grad(out.image, (pg, fg), grad_outputs=Gt)
  assert_within(third[0], first[0], 1e-5, 'd gaussians2d (non-contiguous grad)')
  assert_within(third[1], first[1], 1e-5, 'd features (non-contiguous grad)')


# ---- 7. render_features: a frame's own lists and weights, one frame backward for colour + features
def make_scene3d(n, size, seed):
  torch.manual_seed(seed)
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(n, cam, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=0.1)
  return g.to(dtype=torch.float32).to(DEV), cam.to(dtype=torch.float32).to(device=DEV)


def assert_grads_close(names, a, b, tol=2e-5):
  """tests/test_gpu_frame.py assert_grads_close(modular_conditioning=True): the modular float32 chain behind the
  projection backward is compared by quantiles, everything else entry by entry"""
  for name, x, y in zip(names, a, b):
    scale = max(float(y.abs().max()), 1e-12)
    err = ((x - y).abs() / scale).flatten()
    worst = float(err.max())
    print(f"{name}: worst {worst:.3e} of the largest entry")
    if err.numel() <= 1000:
      assert worst < tol, f"{name}: {worst:.3e} of the largest entry"
      continue
    quantile = lambda q: float(err.float().kthvalue(int(err.numel() * q))[0])
    if name in ('position', 'log_scaling', 'rotation'):
      assert quantile(0.99) < tol, f"{name}: 99 % quantile {quantile(0.99):.3e} of the largest entry"
      assert quantile(0.999) < 50 * tol, f"{name}: 99.9 % quantile {quantile(0.999):.3e}"
    else:
      assert quantile(0.999) < tol, f"{name}: 99.9 % quantile {quantile(0.999):.3e} of the largest entry"
      assert worst < 50 * tol, f"{name}: {worst:.3e} of the largest entry"


@pytest.mark.parametrize('touch', ['before', 'after'])
def test_render_features_equals_the_modular_composition(touch):
  size, n, f = (160, 96), 2000, 32
  g, cam = make_scene3d(n, size, seed=4)
  feats = features_for(n, f).to(DEV)
  gen = torch.Generator().manual_seed(9)
  A, B = torch.randn((96, 160, 3), generator=gen).to(DEV), torch.randn((96, 160, f), generator=gen).to(DEV)
  names = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature', 'features')

  def leaves(gd, fd):
    return [t.grad for t in (gd.position, gd.log_scaling, gd.rotation, gd.alpha_logit, gd.feature, fd)]

  # frame executor + render_features
  gd, fd = g.clone().requires_grad_(True), feats.clone().requires_grad_(True)
  r = render_gaussians(gd, cam, CFG, use_sh=False)
  assert hasattr(r, 'frame')
  if touch == 'before':
    assert r.points.gaussians2d.shape[1] == 7
  image_f = render_features(r, fd)
  if touch == 'after':
    assert r.points.gaussians2d.shape[1] == 7
  assert image_f.shape == (96, 160, f)
  ((r.image * A).sum() + (image_f * B).sum()).backward()
  got = leaves(gd, fd)

  # modular composition: project -> map_to_tiles -> rasterize_with_tiles, colours and features[idx]
  frame.USE_FRAME = False
  try:
    gm, fm = g.clone().requires_grad_(True), feats.clone().requires_grad_(True)
    rm = render_gaussians(gm, cam, CFG, use_sh=False)
    pts = rm.points
    o2p, ranges = map_to_tiles_strip(pts.gaussians2d, pts.depths.detach(), image_size=cam.image_size, config=CFG,
                                     ndc_range=(cam.near_plane, cam.far_plane))       # as render_projected maps
    image_m = rasterize_with_tiles(pts.gaussians2d, fm[pts.idx], o2p, ranges.view(-1, 2), size, CFG).image
    ((rm.image * A).sum() + (image_m * B).sum()).backward()
    want = leaves(gm, fm)
  finally:
    frame.USE_FRAME = True

  assert torch.equal(r.image, rm.image)
  err = float((image_f - image_m).abs().max())
  print(f"feature image: max difference {err:.3e}")
  assert err <= 2e-6
  assert_grads_close(names, got, want)
