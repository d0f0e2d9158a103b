"""Scenes and the float64 oracle of the fused per-gaussian backward pass (csrc/gaussian_bwd.hip), shared by
tests/test_hostmath.py (host build of ``project_backward`` with a covariance gradient) and
tests/test_gpu_gaussian_bwd.py (the kernel itself).  Plain torch on the CPU: nothing here touches a GPU."""
import torch

from oracle import projection as oproj, sh as osh
from taichi_splatting_amd.testing import random_3d_gaussians

BLUR_COV = 0.3
CLAMP_MARGIN = 0.15

# Largest float32 row error of ``project_backward`` with a covariance gradient, relative to the largest float64 gradient
# of the leaf: measured on the host build and asserted by tests/test_hostmath.py::test_projection_backward_cov_f32_rows
# (worst row over 12 scenes x 2 settings: 8.2e-7), times 4 for other scenes and the GPU's exp / sqrt roundings.  Never above the
# 1e-4 the float32 kernels are held to everywhere else.
T_COV = 3.3e-6
assert T_COV <= 1e-4


def clamped_centre_scene(n, camera, scale_factor=1.0, margin=0.6, every=12):
  """``random_3d_gaussians`` (same draws, same order) with every ``every``-th gaussian replaced by a large splat whose
  centre projects OUTSIDE the 15 % clamp margin of ``project_forward`` (0.2 .. 0.4 image sizes beyond the border, on
  one axis or on both) while its extent still reaches the image: the rows on which the clamp of the projected centre
  (``clamp_pass``) is active.  Seeded by the caller's torch.manual_seed."""
  g = random_3d_gaussians(n=n, camera_params=camera, scale_factor=scale_factor, alpha_range=(0.1, 0.9), margin=margin)
  rows = torch.arange(every // 2, max(n, every // 2), every)
  m = rows.numel()
  if m == 0:
    return g
  W, H = camera.image_size
  size = torch.tensor([W, H], dtype=torch.float32)
  beyond = (0.2 + 0.2 * torch.rand(m, 2)) * size                    # distance from the border, per axis
  side = torch.randint(0, 2, (m, 2)).bool()
  outside = torch.where(side, size - 1 + beyond, -beyond)
  inside = torch.rand(m, 2) * size
  which = torch.randint(0, 3, (m,))                                 # 0: x outside, 1: y outside, 2: both
  use_out = torch.stack([which != 1, which != 0], dim=1)
  uv = torch.where(use_out, outside, inside)
  z = camera.near_plane * (4.0 + 40.0 * torch.rand(m))
  fx, fy, cx, cy = [float(v) for v in camera.projection]
  pc = torch.stack([(uv[:, 0] - cx) / fx * z, (uv[:, 1] - cy) / fy * z, z, torch.ones(m)], dim=1)
  world = (torch.inverse(camera.T_camera_world.float()) @ pc.T).T[:, :3]
  sigma_px = 0.35 * max(W, H) * (0.8 + 0.4 * torch.rand(m))        # ~ 3 sigma reaches well into the image
  log_scale = torch.log(sigma_px * z / fx).unsqueeze(1) + 0.2 * torch.randn(m, 3)
  position, log_scaling, alpha_logit = g.position.clone(), g.log_scaling.clone(), g.alpha_logit.clone()
  position[rows], log_scaling[rows] = world, log_scale
  alpha_logit[rows] = torch.logit(0.5 + 0.4 * torch.rand(m, 1))
  return g.replace(position=position, log_scaling=log_scaling, alpha_logit=alpha_logit)


def clamp_active(position, T_camera_world, projection, image_size):
  """(N,) bool: the projected centre lies beyond the clamp margin on at least one axis (float64 oracle arithmetic)"""
  W, H = image_size
  size = torch.tensor([W, H], dtype=torch.float64)
  T = T_camera_world.double()[:3]
  pc = position.double() @ T[:, :3].T + T[:, 3]
  uv = projection.double()[0:2] * pc[:, :2] / pc[:, 2:3] + projection.double()[2:4]
  return ((uv < -size * CLAMP_MARGIN) | (uv > (size - 1) * (1 + CLAMP_MARGIN))).any(dim=1)


def sh_features(n, f, degree, amplitude=None):
  """(n, f, (degree + 1)^2) SH parameters that saturate 10 % .. 75 % of the visible colours (amplitude 2.0, 4.0 at
  degree 0: the clamp mask of the SH backward is live); degree -1: plain colours (n, f)"""
  if degree < 0:
    return torch.rand(n, f)
  amplitude = amplitude or (4.0 if degree == 0 else 2.0)
  return (torch.rand(n, f, (degree + 1) ** 2) - 0.5) * amplitude


def oracle_backward(inputs, image_size, idx, g_points7=None, g_cov_rows=None, g_depth=None, g_colours=None,
                    sh_degree=-1, dtype=torch.float64, clamp_margin=CLAMP_MARGIN):
  """Gradients of the per-gaussian stage by autograd, in ``dtype`` (float64: the truth; float32: the reference's own
  arithmetic as yardstick) on the rows ``idx`` (the visible set; every other row gets zero).

  inputs      position, log_scaling, rotation, alpha_logit (n, 1), feature, T_camera_world (4, 4), projection (4)
  g_points7   (n, 7) upstream of the packed 2D gaussian [mean | axis | sigma | alpha]          -> oracle.projection.apply's chain
  g_cov_rows  (n, 7) upstream in covariance form [d mean | da, db, dc | 0 | d alpha]          -> covariance_all
  g_depth     (n,)   upstream of the depth z
  g_colours   (n, f) upstream of the clamped SH colours (positions and camera position detached)
  Returns dict(position, log_scaling, rotation, alpha_logit, feature, camera (16,): T[:3] row-major then projection),
  plus colours (n, f) (zero outside idx) when sh_degree >= 0."""
  leaves = [t.detach().to(dtype).clone().requires_grad_(True) for t in inputs]
  pos, ls, rot, al, feat, T, P = leaves
  n = pos.shape[0]
  sel = [t[idx] for t in (pos, ls, rot, al)]
  outs, ups = [], []
  far = (0.0, float('inf'))
  if g_points7 is not None:
    points, _, _ = oproj.project_all(*sel, T, P, image_size, far, blur_cov=BLUR_COV, clamp_margin=clamp_margin)
    outs.append(points); ups.append(g_points7[idx].to(dtype))
  if g_cov_rows is not None or g_depth is not None:
    uv, a, b, c, alpha, z = oproj.covariance_all(*sel, T, P, image_size, blur_cov=BLUR_COV, clamp_margin=clamp_margin)
    if g_cov_rows is not None:
      r = g_cov_rows[idx].to(dtype)
      outs += [uv, a, b, c, alpha]; ups += [r[:, 0:2], r[:, 2], r[:, 3], r[:, 4], r[:, 6]]
    if g_depth is not None:
      outs.append(z); ups.append(g_depth[idx].to(dtype))
  result = {}
  if sh_degree >= 0:
    cam_pos = torch.inverse(T.detach())[:3, 3]
    colours = osh.evaluate_sh_at(feat, pos.detach(), idx, cam_pos)
    full = torch.zeros((n, colours.shape[1]), dtype=dtype)
    full[idx] = colours.detach()
    result['colours'] = full
    d = feat.shape[2]
    coeffs = osh.rsh_cart((pos.detach()[idx] - cam_pos) / (pos.detach()[idx] - cam_pos).norm(dim=1, keepdim=True), sh_degree)
    pre = torch.zeros_like(full)
    pre[idx] = (coeffs.unsqueeze(1) * feat.detach()[idx]).sum(-1) + 0.5
    result['pre_clamp'] = pre
    assert d == (sh_degree + 1) ** 2
    if g_colours is not None:
      outs.append(colours); ups.append(g_colours[idx].to(dtype))
  if outs and idx.numel() > 0:
    torch.autograd.backward(outs, ups)
  grad = lambda t: t.grad.detach() if t.grad is not None else torch.zeros_like(t)
  result.update(position=grad(pos), log_scaling=grad(ls), rotation=grad(rot), alpha_logit=grad(al).reshape(-1),
                feature=grad(feat), camera=torch.cat([grad(T)[:3].reshape(-1), grad(P)]))
  return result


def row_error(got, want):
  """per-row (per-gaussian) largest error relative to the largest entry of ``want`` (the float64 gradient of a leaf)"""
  got, want = got.double().reshape(got.shape[0], -1), want.double().reshape(want.shape[0], -1)
  scale = max(float(want.abs().max()), 1e-300)
  return (got - want).abs().max(dim=1).values / scale
