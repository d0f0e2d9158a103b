"""GPU tests of the bilateral-grid slice (csrc/bilagrid.hip through taichi_splatting_amd/appearance.py) against the float64
oracle on the CPU (tests/bilagrid_oracle.py), within error bounds that come from the number format and not from the
kernels: with eps the unit roundoff of the dtype and G = max(L, Gy, Gx),

  output          |d| <= 16 eps G max|grid| (|r| + |g| + |b| + 1)                              per pixel
  grid gradient   |d| <= 16 eps G S[c, j, yv, xv],  S = the unweighted sum of |g_c| |p1_j| over the pixels of the vertex's
                  xy footprint; where S = 0 the gradient is exactly 0
  image gradient  |d| <= 16 eps G max(L - 1, 1) max|grid| sum_c|g_c| (|r| + |g| + |b| + 1)    per pixel, leaving out the
                  pixels whose unclamped lum (L - 1) is within 1e-4 of an integer in 0..L-1 (the guide term jumps there)

(about a dozen roundings per term; the rounding of a coordinate scales with G).  The float32 grid_sample composition on
the CPU, an independent implementation, is asserted to sit at <= 0.1 of the same bounds.

Which shape runs which path (a forward / image-gradient workgroup owns 64 x 16 pixels and stages the vertices its tile
touches in LDS when their L x 12 coefficients number <= 4096; the grid gradient cuts a vertex's footprint into 64 x 64
chunks and walks the luminance bins in groups of 2 (L <= 2) or 8):

  (37, 53, 8, 16, 16)    global fallback in all three row tiles (16 x 8 vertices = 12288 coefficients); ragged in x and y
  (5, 7, 8, 16, 16)      global fallback (256 vertices); most vertices have an empty footprint: exactly 0
  (64, 64, 1, 1, 1)      staged, one vertex; all three axes of size 1; whole tiles
  (19, 200, 4, 3, 5)     staged; ragged last tile in x (8 of 64 columns) and y (3 of 16 rows); 2 chunks per vertex
  (130, 70, 2, 2, 2)     staged; 3 x 2 chunks per vertex, the last ones ragged; bins in one group of 2
  (256, 256, 8, 16, 16)  staged, 10 to 18 vertices per tile; one chunk per vertex
  (256, 256, 2, 2, 2)    staged, a cell wider than any tile; 16 chunks per vertex
  (33, 65, 16, 2, 3)     staged; two groups of 8 bins; one column in the second tile
  (1, 1, 8, 16, 16)      staged, one pixel
  (100, 150, 5, 2, 3)    added: several chunks per vertex together with a group of 8 bins of which 5 exist
"""
import functools

import pytest
import torch

from tests import bilagrid_oracle as bo

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'

SHAPES = [(37, 53, 8, 16, 16), (5, 7, 8, 16, 16), (64, 64, 1, 1, 1), (19, 200, 4, 3, 5), (130, 70, 2, 2, 2),
          (256, 256, 8, 16, 16), (256, 256, 2, 2, 2), (33, 65, 16, 2, 3), (1, 1, 8, 16, 16), (100, 150, 5, 2, 3)]


@functools.lru_cache(maxsize=None)
def case(shape, dtype=torch.float64):
  """(image, grid, grad_out) of one shape in ``dtype``, the float64 oracle ON THOSE VALUES and the bounds for ``dtype``:
  computed once, shared, never written to"""
  image, grid, grad_out = (t.to(dtype) for t in bo.make_case(*shape))
  want = bo.reference(image.double(), grid.double(), grad_out.double())
  return image, grid, grad_out, want, bo.bounds(image, grid, grad_out, bo.unit_roundoff(dtype))


@functools.lru_cache(maxsize=None)
def composed32(shape):
  """the float32 grid_sample composition and its autograd on the CPU"""
  image, grid, grad_out, _, _ = case(shape, torch.float32)
  return bo.reference(image, grid, grad_out)


def fused(image, grid, grad_out, dtype, image_grad=True, grid_grad=True):
  from taichi_splatting_amd import apply_bilateral_grid
  x = image.to(DEV, dtype).requires_grad_(image_grad)
  g = grid.to(DEV, dtype).requires_grad_(grid_grad)
  out = apply_bilateral_grid(x, g)
  out.backward(grad_out.to(DEV, dtype))
  torch.cuda.synchronize()
  return out.detach().cpu(), None if x.grad is None else x.grad.cpu(), None if g.grad is None else g.grad.cpu()


def excesses(got, want, b):
  """error / bound of (out, grad_image, grad_grid), the largest of each"""
  return (bo.excess(got[0], want[0], b['out'][..., None]),
          bo.excess(got[1], want[1], b['grad_image'][..., None], b['covered']),
          bo.excess(got[2], want[2], b['grad_grid']))


def check(shape, dtype, what):
  x, g, go, reference, b = case(shape, dtype)
  lum = bo.luminance(x.double())
  below, above = float((lum < 0).double().mean()), float((lum > 1).double().mean())
  excluded = 1 - float(b['covered'].double().mean())
  got = fused(x, g, go, dtype)
  e = excesses(got, reference, b)
  print(f"{what} {shape}: error / bound: out {e[0]:.3f}, image gradient {e[1]:.3f}, grid gradient {e[2]:.3f}; "
        f"luminance below 0: {below:.3f}, above 1: {above:.3f}; excluded {excluded:.5f}")
  if shape[0] * shape[1] > 1:               # (a single pixel cannot lie on both sides)
    assert below >= 0.01 and above >= 0.01
  assert excluded <= 0.01
  assert all(torch.isfinite(t).all() for t in got)
  assert e[0] <= 1 and e[1] <= 1 and e[2] <= 1
  zero = b['grad_grid'] == 0
  assert bool((got[2][zero] == 0).all())


@pytest.mark.parametrize('shape', SHAPES)
def test_float32_kernels_hold_the_bounds(shape):
  check(shape, torch.float32, 'float32')
  # an independent float32 implementation holds a tenth of the same bounds
  _, _, _, reference, b = case(shape, torch.float32)
  e = excesses(composed32(shape), reference, b)
  print(f"float32 torch composition on the CPU: error / bound: out {e[0]:.3f}, image gradient {e[1]:.3f}, grid gradient {e[2]:.3f}")
  assert max(e) <= 0.1


@pytest.mark.parametrize('shape', SHAPES)
def test_float64_kernels_hold_the_bounds(shape):
  check(shape, torch.float64, 'float64')


def test_most_vertices_of_a_fine_grid_receive_exactly_zero():
  image, grid, grad_out, _, _ = case((5, 7, 8, 16, 16))
  S = bo.footprint_abs_sum(image, grad_out, 16, 16)
  assert 0.3 < float((S == 0).double().mean()) < 1.0
  _, _, grad_grid = fused(image, grid, grad_out, torch.float32)
  assert bool((grad_grid[(S == 0).reshape(12, 1, 16, 16).expand(12, 8, 16, 16)] == 0).all())


@pytest.mark.parametrize('level', [0.0, 1.0, 1.0 + 2.0 ** -20])
def test_black_and_white_images(level):
  """luminance exactly 0 and at or just above 1: the clamped ends, where the guide has no gradient.  At 0 and just above 1
  no pixel is left out of the image-gradient bound: the kernels must put these on the flat side.  At level 1 the
  luminance itself rounds to 1 in float32 and to 1 - 1.1e-16 in the float64 oracle, the two sides of the jump: there
  the bound's own rule applies (lum (L - 1) within 1e-4 of an integer) and the output and the grid gradient are checked."""
  shape = (19, 200, 4, 3, 5)
  _, g, go, _, _ = case(shape, torch.float32)
  x = torch.full((shape[0], shape[1], 3), level, dtype=torch.float32)
  reference = bo.reference(x.double(), g.double(), go.double())
  b = bo.bounds(x, g, go, bo.unit_roundoff(torch.float32))
  if level != 1.0:
    b['covered'] = torch.ones_like(b['covered'])
  e = excesses(fused(x, g, go, torch.float32), reference, b)
  print(f"level {level}: error / bound {e}")
  assert max(e) <= 1


def test_one_nan_pixel_stays_one_pixel():
  from taichi_splatting_amd import apply_bilateral_grid
  for shape in ((37, 53, 8, 16, 16), (256, 256, 8, 16, 16)):          # global fallback and staged
    x, grid, _, (reference, _, _), b = case(shape, torch.float32)
    for bad in (float('nan'), float('inf'), -float('inf')):
      y = x.clone()
      y[shape[0] // 2, shape[1] // 3, 1] = bad
      with torch.no_grad():
        out = apply_bilateral_grid(y.to(DEV), grid.to(DEV)).cpu()
      others = torch.ones(shape[:2], dtype=torch.bool)
      others[shape[0] // 2, shape[1] // 3] = False
      assert torch.isfinite(out[others]).all()
      assert bo.excess(out, reference, b['out'][..., None], others) <= 1


def test_non_contiguous_inputs():
  from taichi_splatting_amd import apply_bilateral_grid
  shape = (33, 65, 16, 2, 3)
  image, grid, grad_out, _, _ = case(shape)
  want = fused(image, grid, grad_out, torch.float32)
  wide = torch.zeros((33, 65, 4), device=DEV)
  wide[..., :3] = image.float().to(DEV)
  x = wide[..., :3].requires_grad_(True)                               # pixel stride 4
  g = grid.float().to(DEV).permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2).requires_grad_(True)   # coefficient-innermost storage
  assert not x.is_contiguous() and not g.is_contiguous()
  out = apply_bilateral_grid(x, g)
  out.backward(grad_out.float().to(DEV))
  assert torch.equal(out.detach().cpu(), want[0]) and torch.equal(x.grad.cpu(), want[1]) and torch.equal(g.grad.cpu(), want[2])


def test_only_the_needed_gradient_is_computed():
  shape = (130, 70, 2, 2, 2)
  image, grid, grad_out, _, _ = case(shape)
  both = fused(image, grid, grad_out, torch.float32)
  out, gi, gg = fused(image, grid, grad_out, torch.float32, grid_grad=False)
  assert gg is None and torch.equal(gi, both[1]) and torch.equal(out, both[0])
  out, gi, gg = fused(image, grid, grad_out, torch.float32, image_grad=False)
  assert gi is None and torch.equal(gg, both[2]) and torch.equal(out, both[0])


@pytest.mark.parametrize('shape', [(37, 53, 8, 16, 16), (64, 64, 1, 1, 1), (256, 256, 8, 16, 16)])
def test_identity_grid_returns_the_image(shape):
  from taichi_splatting_amd import apply_bilateral_grid, identity_bilateral_grid
  image, _, grad_out, _, _ = case(shape)
  x = image.float()
  grid = identity_bilateral_grid(*shape[2:], device=DEV)
  out = apply_bilateral_grid(x.to(DEV), grid).cpu()
  b = bo.bounds(x, grid.cpu(), grad_out.float(), bo.unit_roundoff(torch.float32))
  assert bo.excess(out, x, b['out'][..., None]) <= 1


def test_two_runs_are_bit_identical():
  for shape in ((256, 256, 2, 2, 2), (37, 53, 8, 16, 16)):
    image, grid, grad_out, _, _ = case(shape)
    a, b = fused(image, grid, grad_out, torch.float32), fused(image, grid, grad_out, torch.float32)
    assert all(torch.equal(s, t) for s, t in zip(a, b))


def capture(step):
  side = torch.cuda.Stream()
  side.wait_stream(torch.cuda.current_stream())
  with torch.cuda.stream(side):
    for _ in range(2):
      step()
  torch.cuda.current_stream().wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    result = step()
  return graph, result


def test_forward_and_backward_capture_into_a_graph():
  from taichi_splatting_amd import apply_bilateral_grid
  shape = (130, 70, 2, 2, 2)
  image, grid, grad_out, _, _ = case(shape)
  eager = fused(image, grid, grad_out, torch.float32)
  x = torch.zeros(shape[0], shape[1], 3, device=DEV).requires_grad_(True)
  g = grid.float().to(DEV).requires_grad_(True)
  go = grad_out.float().to(DEV)

  def step():
    out = apply_bilateral_grid(x, g)
    return (out,) + torch.autograd.grad(out, (x, g), go)

  graph, result = capture(step)
  with torch.no_grad():
    x.copy_(image.float().to(DEV))               # the capture saw another image: the replay must read this one
  graph.replay()
  torch.cuda.synchronize()
  assert all(torch.equal(r.detach().cpu(), e) for r, e in zip(result, eager))


def test_device_index_selects_the_grid_in_a_replay():
  from taichi_splatting_amd import BilateralGrids
  shape = (19, 200, 4, 3, 5)
  image, grid, grad_out, _, _ = case(shape)
  grids = BilateralGrids(2, grid_shape=(5, 3, 4), device=DEV)
  with torch.no_grad():
    grids.grids[0].copy_(grid.float().to(DEV))
    grids.grids[1].copy_(grid.float().flip(1).to(DEV))
  x, go = image.float().to(DEV), grad_out.float().to(DEV)

  def eager_step(i):
    out = grids(x, i)
    return out.detach().clone(), torch.autograd.grad(out, grids.grids, go)[0].clone()

  # (no autograd graph of these eager steps may outlive them: one that is alive at the capture keeps the parameter's
  # gradient accumulator on the default stream, and the captured backward would fork onto it and never join)
  eager = [eager_step(i) for i in range(2)]
  assert not torch.equal(eager[0][0], eager[1][0])
  assert float(eager[0][1][1].abs().max()) == 0 and float(eager[1][1][0].abs().max()) == 0
  index = torch.zeros((), dtype=torch.int64, device=DEV)

  def step():
    out = grids(x, index)
    return out, torch.autograd.grad(out, grids.grids, go)[0]

  graph, (out, grad) = capture(step)
  for i in (1, 0, 1):
    index.fill_(i)
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(out.detach(), eager[i][0]) and torch.equal(grad, eager[i][1])


def test_render_slice_loss_backward():
  """render_gaussians(...).image -> apply_bilateral_grid -> l1_ssim_loss -> backward: dL/dimage agrees with the same chain
  built from float32 grid_sample on the GPU within the image-gradient bound, and every gaussian parameter receives a
  finite, non-zero gradient"""
  from taichi_splatting_amd import RasterConfig, apply_bilateral_grid, l1_ssim_loss, render_gaussians
  from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
  torch.manual_seed(3)
  size = (96, 64)
  cam = random_camera(image_size=size)
  scene = random_3d_gaussians(600, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  scene = scene.replace(feature=(torch.rand(600, 3, 16) - 0.5) * 0.5)
  target = torch.rand((size[1], size[0], 3)).to(DEV)
  _, grid, _ = bo.make_case(size[1], size[0], 8, 16, 16, seed=5)
  grid = grid.float().to(DEV)
  fields = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')

  def chain(slice_fn):
    gd = scene.to(DEV).requires_grad_(True)
    r = render_gaussians(gd, cam.to(device=DEV), RasterConfig(), use_sh=True)
    r.image.retain_grad()
    out = slice_fn(r.image, grid)
    out.retain_grad()
    l1_ssim_loss(out, target).backward()
    return r.image.detach(), r.image.grad, out.grad, [getattr(gd, k).grad for k in fields]

  image, got, upstream, grads = chain(apply_bilateral_grid)
  image_t, want, _, _ = chain(bo.slice_grid_sample)
  assert torch.equal(image, image_t)
  b = bo.bounds(image.cpu(), grid.cpu(), upstream.cpu(), bo.unit_roundoff(torch.float32))
  e = bo.excess(got.cpu(), want.cpu(), b['grad_image'][..., None], b['covered'])
  print(f"dL/dimage, fused against the float32 grid_sample chain: error / bound {e:.3f}; "
        f"excluded {1 - float(b['covered'].double().mean()):.5f}")
  assert float(want.abs().max()) > 0 and e <= 1
  for k, t in zip(fields, grads):
    assert t is not None and torch.isfinite(t).all() and float(t.abs().max()) > 0, k


def test_the_example_fits_the_photographs():
  """the training loop of examples/fit_appearance.py at 64 x 64, 3 views, 150 steps"""
  from taichi_splatting_amd.examples.fit_appearance import fit
  result = fit(size=(64, 64), views=3, steps=150)
  print(f"loss {result['initial_loss']:.5f} -> {result['final_loss']:.5f} in {result['steps_taken']} steps")
  assert result['final_loss'] < 0.5 * result['initial_loss']
  assert result['steps_taken'] == 150          # the stopping rule is for a finished fit: it does not cut this one short


def test_the_example_leaves_the_grids_alone_on_identity_targets():
  """Targets equal to the renders: the loss starts at rounding level (4e-10 in float32), the loop's stopping rule (mean
  photometric loss <= 1e-6) ends it before Adam can turn the SSIM gradient's rounding noise into steps, and the grids stay
  where they are.  (Without the rule, tol = 0, they wander 8.6e-3 from the identity in 150 steps and the loss rises to
  9e-4: examples/fit_appearance.py says why.)"""
  from taichi_splatting_amd import identity_bilateral_grid
  from taichi_splatting_amd.examples.fit_appearance import fit
  result = fit(size=(64, 64), views=3, steps=150, identity_targets=True)
  drift = float((result['grids'].grids.detach() - identity_bilateral_grid(8, 16, 16, device=DEV)).abs().max())
  print(f"loss {result['initial_loss']:.3e} -> {result['final_loss']:.3e} in {result['steps_taken']} steps; "
        f"largest departure from the identity {drift:.3e}")
  assert drift <= 1e-6
