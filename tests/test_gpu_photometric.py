"""-m gpu: the fused photometric loss (csrc/loss.hip, taichi_splatting_amd/loss.py) against the float64 oracle of
tests/photometric_oracle.py: float64 kernels to 1e-11 of the largest value, float32 kernels inside the error model
(four times the float32 torch composition's own deviation on the same input, plus the rounding floor), and the
behaviour of the interface (rendered input, upstream gradient, determinism, graph capture, views, errors, the demo)."""
import functools

import pytest
import torch

from tests import photometric_oracle as po

pytestmark = pytest.mark.gpu
DEV = 'cuda:0'
CASES = [(s, p) for s in po.SHAPES for p in po.paddings(s[0], s[1])]


@functools.lru_cache(maxsize=None)
def oracle(kind, shape, padding):
  """(x, y, analytic parts) on the CPU in float64, once per input"""
  x, y = po.make_pair(kind, *shape)
  return x, y, po.analytic(x, y, padding)


def run_kernels(x, y, lam, padding, dtype):
  from taichi_splatting_amd.loss import photometric_forward, photometric_backward
  xd, yd = x.to(DEV, dtype), y.to(DEV, dtype)
  out, maps = photometric_forward(xd, yd, lam, padding, want_maps=True)
  grad = photometric_backward(xd, yd, maps, torch.ones((1,), device=DEV, dtype=dtype), lam, padding)
  return out.cpu().double(), maps.cpu().double(), grad.cpu().double()


def close(got, want, rel, what):
  scale = max(float(want.abs().max()), 1e-300)
  err = float((got - want).abs().max())
  assert torch.isfinite(got).all() and err <= rel * scale, f"{what}: off by {err:.3e}, {err / scale:.3e} of the largest value"


@pytest.mark.parametrize('shape,padding', CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{p}" for s, p in CASES])
def test_float64_kernels_equal_the_oracle(shape, padding):
  x, y, parts = oracle('random', shape, padding)
  for lam in po.LAMBDAS:
    out, maps, grad = run_kernels(x, y, lam, padding, torch.float64)
    loss, grad_want = po.combine(parts, lam)
    want = torch.stack([loss, parts['l1'], parts['ssim']])
    close(out, want, 1e-11, f"(loss, l1, ssim) at lambda {lam}")
    for k, name in enumerate('ABC'):
      close(maps[k], parts[name], 1e-11, f"partial map {name}")
    assert grad.shape == x.shape
    if float(grad_want.abs().max()) > 0:
      close(grad, grad_want, 1e-11, f"dL/dimage at lambda {lam}")
    else:
      assert float(grad.abs().max()) == 0.0


def check_float32(x, y, parts, padding, what):
  for lam in po.LAMBDAS:
    tol = po.tolerances(x, y, lam, padding, parts)
    out, _, grad = run_kernels(x, y, lam, padding, torch.float32)
    loss, grad_want = po.combine(parts, lam)
    errs = dict(loss=abs(float(out[0] - loss)), l1=abs(float(out[1] - parts['l1'])), ssim=abs(float(out[2] - parts['ssim'])),
                grad=float((grad - grad_want).abs().max()))
    print(f"{what} lambda {lam}: " + "  ".join(f"{k} {errs[k]:.2e} / {tol[k]:.2e}" for k in errs))
    assert torch.isfinite(out).all() and torch.isfinite(grad).all()
    for k in errs:                        # every element: the gradient bound holds for the largest error of all of them
      assert errs[k] <= tol[k], f"{what}, lambda {lam}: {k} off by {errs[k]:.3e} > {tol[k]:.3e}"


@pytest.mark.parametrize('shape,padding', CASES, ids=[f"{s[0]}x{s[1]}x{s[2]}-{p}" for s, p in CASES])
def test_float32_kernels_stay_inside_the_error_model(shape, padding):
  x, y, parts = oracle('random', shape, padding)
  check_float32(x, y, parts, padding, f"random {shape} {padding}")


@pytest.mark.parametrize('padding', ['same', 'valid'])
@pytest.mark.parametrize('kind', po.KINDS)
def test_float32_kernels_on_the_named_inputs(kind, padding):
  x, y, parts = oracle(kind, po.KIND_SHAPE, padding)
  check_float32(x, y, parts, padding, f"{kind} {padding}")


def small_scene():
  from taichi_splatting_amd import RasterConfig
  from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
  torch.manual_seed(3)
  size = (96, 64)
  cam = random_camera(image_size=size)
  g = random_3d_gaussians(600, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  g = g.replace(feature=(torch.rand(600, 3, 16) - 0.5) * 0.5)
  target = torch.rand((size[1], size[0], 3))
  return g, cam, RasterConfig(), target


FIELDS = ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature')


def test_rendered_input_end_to_end():
  """render -> l1_ssim_loss -> backward: the gradients of the five parameter tensors equal those of the float64 oracle
  loss (torch autograd) fed with the same render and sent back through the same render node (a second, identical frame)"""
  from taichi_splatting_amd import render_gaussians, l1_ssim_loss
  g, cam, cfg, target = small_scene()
  cam_d = cam.to(device=DEV)

  def frame_grads(image_loss):
    gd = g.to(DEV).requires_grad_(True)
    r = render_gaussians(gd, cam_d, cfg, use_sh=True)
    image_loss(r.image).backward()
    return r.image.detach(), [getattr(gd, k).grad for k in FIELDS]

  losses = {}

  def fused(image):
    losses['fused'] = l1_ssim_loss(image, target.to(DEV))
    return losses['fused']

  def through_the_oracle(image):
    image64 = image.detach().cpu().double().requires_grad_(True)
    losses['oracle'] = po.loss_terms(image64, target.double(), 0.2, 'same')[0]
    losses['oracle'].backward()
    return (image * image64.grad.to(DEV, torch.float32)).sum()          # d/dimage = the oracle's gradient

  image_a, grads = frame_grads(fused)
  image_b, want = frame_grads(through_the_oracle)
  assert torch.equal(image_a, image_b) and float(image_a.abs().max()) > 0
  assert abs(float(losses['fused']) - float(losses['oracle'])) <= 1e-5 * abs(float(losses['oracle']))
  for k, got, ref in zip(FIELDS, grads, want):
    assert torch.isfinite(got).all() and float(ref.abs().max()) > 0
    rel = ((got - ref).abs() / ref.abs().max()).reshape(got.shape[0], -1).max(dim=1).values
    assert float(rel.max()) <= 1e-4, f"{k}: a row is off by {float(rel.max()):.2e} of the largest gradient"


def test_upstream_gradient_is_read_on_the_device():
  from taichi_splatting_amd import l1_ssim_loss
  x, y = (t.to(DEV, torch.float32) for t in po.make_pair('smooth_noisy', 45, 70, 3))
  grads = []
  for scale in (None, 3.0, torch.full((), 3.0, device=DEV)):
    xg = x.clone().requires_grad_(True)
    loss = l1_ssim_loss(xg, y)
    (loss if scale is None else scale * loss).backward()
    grads.append(xg.grad)
  assert float(grads[0].abs().max()) > 0
  for g3 in grads[1:]:
    assert float((g3 - 3 * grads[0]).abs().max()) <= 4 * 2.0 ** -24 * float(g3.abs().max())
  assert torch.equal(grads[1], grads[2])


def test_two_calls_are_bit_identical():
  from taichi_splatting_amd import l1_ssim_loss
  x, y = (t.to(DEV, torch.float32) for t in po.make_pair('random', 129, 257, 3))
  results = []
  for _ in range(2):
    xg = x.clone().requires_grad_(True)
    loss, l1, ssim = l1_ssim_loss(xg, y, return_terms=True)
    loss.backward()
    assert not l1.requires_grad and not ssim.requires_grad
    results.append((loss.detach().clone(), l1.clone(), ssim.clone(), xg.grad.clone()))
  for a, b in zip(*results):
    assert torch.equal(a, b)
  loss, l1, ssim, _ = results[0]
  assert abs(float(loss) - (0.8 * float(l1) + 0.2 * (1 - float(ssim)))) <= 1e-6


def test_step_with_the_loss_captures_into_a_graph():
  """render -> loss -> backward captured with frame.FrameGraph and replayed on three targets written into the same
  storage: the loss, dL/dimage and the gradients of all five parameter tensors of every replay equal the eager step on
  that target bit for bit.  The raster backward runs in its deterministic (fixed-point) mode for this test: its default
  float atomics have no fixed order, and bit-equality of the leaves is what shows that nothing between dL/dimage and
  the parameters goes stale in a replay."""
  from taichi_splatting_amd import render_gaussians, l1_ssim_loss, frame
  from taichi_splatting_amd.rasterizer import function as raster_function
  g, cam, cfg, target = small_scene()
  cam_d = cam.to(device=DEV)
  gd = g.to(DEV).requires_grad_(True)
  leaves = [getattr(gd, k) for k in FIELDS]
  target_d = target.to(DEV).clone()

  def step():
    for t in leaves:
      t.grad = None
    r = render_gaussians(gd, cam_d, cfg, use_sh=True)
    r.image.retain_grad()
    loss = l1_ssim_loss(r.image, target_d)
    loss.backward()
    return r, loss

  was = raster_function.DETERMINISTIC_BACKWARD
  raster_function.DETERMINISTIC_BACKWARD = True
  try:
    targets = [torch.rand_like(target_d) for _ in range(3)]
    eager = []
    for t in targets:
      target_d.copy_(t)
      r, loss = step()
      eager.append((loss.detach().clone(), r.image.grad.clone(), [x.grad.clone() for x in leaves]))
      del r, loss
    graph = frame.FrameGraph(step, warmup=2)
    for t, (loss_e, image_grad_e, grads_e) in zip(targets, eager):
      target_d.copy_(t)
      r, loss = graph.replay()
      torch.cuda.synchronize()
      assert torch.equal(loss.detach(), loss_e) and torch.equal(r.image.grad, image_grad_e)
      for k, leaf, ref in zip(FIELDS, leaves, grads_e):
        assert float(ref.abs().max()) > 0
        assert torch.equal(leaf.grad, ref), f"{k}: a replay differs from the eager step by {float((leaf.grad - ref).abs().max()):.3e}"
    assert len({float(e[0]) for e in eager}) == 3
  finally:
    raster_function.DETERMINISTIC_BACKWARD = was


def test_views_and_non_contiguous_inputs():
  from taichi_splatting_amd import l1_ssim_loss
  x, y = (t.to(DEV, torch.float32) for t in po.make_pair('random', 40, 56, 3))

  def run(xi, yi):
    leaf = xi.detach().requires_grad_(True)
    loss = l1_ssim_loss(leaf, yi)
    loss.backward()
    return loss.detach(), leaf.grad

  want = run(x, y)
  big = torch.zeros((50, 70, 3), device=DEV)
  big[5:45, 7:63] = x
  channels_first = x.permute(2, 0, 1).contiguous().permute(1, 2, 0)
  for xi in (big[5:45, 7:63], channels_first):
    assert not xi.is_contiguous()
    got = run(xi, y.permute(2, 0, 1).contiguous().permute(1, 2, 0))
    assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


def test_bad_inputs_raise():
  from taichi_splatting_amd import l1_ssim_loss, ssim
  x = torch.rand((16, 16, 3), device=DEV)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    l1_ssim_loss(x.cpu(), x.cpu())
  with pytest.raises(ValueError, match="channels"):
    l1_ssim_loss(torch.rand((16, 16, 5), device=DEV), torch.rand((16, 16, 5), device=DEV))
  with pytest.raises(ValueError, match="valid"):
    l1_ssim_loss(torch.rand((10, 32, 3), device=DEV), torch.rand((10, 32, 3), device=DEV), padding='valid')
  with pytest.raises(ValueError, match="target"):
    l1_ssim_loss(x, x.clone().requires_grad_(True))
  with pytest.raises(TypeError):
    l1_ssim_loss(x.half(), x.half())
  assert abs(float(ssim(x, x)) - 1) < 1e-5
  xg = x.clone().requires_grad_(True)
  other = torch.rand_like(x)
  s = ssim(xg, other)
  s.backward()
  assert s.dim() == 0 and float(xg.grad.abs().max()) > 0
  assert torch.equal(s.detach(), ssim(x, other))            # one value, whether or not a gradient is wanted
  xl = x.clone().requires_grad_(True)
  (1 - ssim(xl, other)).backward()                          # and its gradient is minus that of the loss at weight 1
  xw = x.clone().requires_grad_(True)
  l1_ssim_loss(xw, other, ssim_weight=1.0).backward()
  assert torch.equal(xl.grad, xw.grad) and torch.equal(xg.grad, -xw.grad)


def test_fit_test_card_with_the_fused_loss():
  """The demo with loss='l1_ssim' (same call as tests/test_gpu_fit_image.py).  Measured PSNR histories of both losses:
  profiles/loss.txt."""
  from taichi_splatting_amd.examples.fit_image_gaussians import fit, test_card, psnr
  ref = test_card(192, 128, torch.device(DEV))
  image, params, history = fit(ref, n=400, iters=240, target=800, seed=0, loss='l1_ssim')
  first, last = history[0][1], history[-1][1]
  print("l1_ssim psnr history:", [(i, round(p, 2), n) for i, p, n in history])
  assert all(torch.isfinite(t).all() for t in params.tensors.values())
  assert 700 <= params.batch_size[0] <= 800, params.batch_size
  assert last > first + 10.8, history        # half of the measured gain (12.0 -> 33.6 dB, profiles/loss.txt)
  assert image.shape == ref.shape and abs(psnr(ref, image) - last) < 1e-3
