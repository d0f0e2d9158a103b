"""Oracle of the geometry kernels (csrc/geometry.hip): per-gaussian normals and the normal-consistency loss restated in
plain torch with autograd, in whatever dtype the inputs have (float64 is the yardstick; the same code on float32 tensors
is the "torch composition" the tests hold inside the bounds and tools/bench_geometry.py times), with the kernels' tie,
sign, TINY, alpha_min and interior rules.  Also the cases and the error bounds of tests/test_gpu_geometry.py.

Bounds (eps = unit roundoff of the dtype under test, K = 16 roundings behind a value, as tests/test_gpu_bilagrid.py
counts them).  An input P of the stencil carries a few roundings relative to |P|; a = P(x + 1) - P(x - 1) cancels, so its
relative error is eps K_P (|P(x + 1)| + |P(x - 1)|) / |a|, and the same for b.  The unit normal of c = b x a then moves by
at most  (|da| |b| + |a| |db|) / |c| = kappa (|da| / |a| + |db| / |b|),  kappa = |a| |b| / |a x b|.  With
A = (|P(x + 1)| + |P(x - 1)|) / |a| + (|P(y + 1)| + |P(y - 1)|) / |b| the per-pixel condition number is  cond = kappa A:

  n_d            |d| <= K eps cond                                                per component, pixels with cond <= CAP
  loss           |d| <= eps (K sum w cond + K sum 2 w) / ((H - 2)(W - 2))          (the sum's terms are 2 w at most)
  normal grads   |d| <= eps |w g| / |m| (K cond + K)                              m = normal_sum; 0 where it is under TINY
  depth, alpha   with E(p) = eps |w g| / |c| (4 K cond + K) the error of dL/dc at centre p (n_d enters it twice, |c| once,
                 and the edge it is crossed with once), pixel q collects E |b| from its left and right centres and E |a|
                 from the upper and lower ones, times (|u| + |v| + 1) of its ray; / alpha for depth_sum, |d| / alpha for
                 alpha
Pixels whose cond exceeds CAP = 1e4 are left out of the n_d and gradient checks (the cases keep them under 1 %); a pixel
within two pixels of one is left out of the depth and alpha gradients with it.
"""
import torch

TINY = 1e-30
K = 16
CAP = 1e4


def unit_roundoff(dtype):
  return torch.finfo(dtype).eps / 2


# ---- per-gaussian normals ---------------------------------------------------------------------------------------------

def rotation_columns(q):
  """(N, 3, 3) with [:, k] = column k of R(q) for unit quaternions xyzw"""
  x, y, z, w = q.unbind(1)
  c0 = torch.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y + 2 * w * z, 2 * x * z - 2 * w * y], 1)
  c1 = torch.stack([2 * x * y - 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z + 2 * w * x], 1)
  c2 = torch.stack([2 * x * z + 2 * w * y, 2 * y * z - 2 * w * x, 1 - 2 * x * x - 2 * y * y], 1)
  return torch.stack([c0, c1, c2], 1)


def smallest_axis(log_scaling):
  """index of the smallest entry, the lowest index on a tie"""
  s0, s1, s2 = log_scaling.detach().unbind(1)
  k = torch.where(s1 < s0, 1, 0)
  smallest = torch.where(s1 < s0, s1, s0)
  return torch.where(s2 < smallest, 2, k)


def normals(position, log_scaling, rotation, camera_position):
  q = rotation / rotation.square().sum(1, keepdim=True).sqrt()
  k = smallest_axis(log_scaling)
  n = rotation_columns(q)[torch.arange(q.shape[0], device=q.device), k]
  flip = (n.detach() * (position.detach() - camera_position.detach())).sum(1) > 0
  return torch.where(flip[:, None], -n, n)


def normal_margins(position, log_scaling, rotation, camera_position):
  """(|n . (p - c)|, gap between the two smallest log_scaling) per row: where either is tiny the choice is ill-posed"""
  n = normals(position, log_scaling, rotation, camera_position)
  s = log_scaling.sort(dim=1).values
  return (n * (position - camera_position)).sum(1).abs(), s[:, 1] - s[:, 0]


def make_gaussians(n, seed=0):
  """float64 (position, log_scaling, rotation, camera_position).  The first rows are planted where there are enough:
  0: the two smallest scales equal (tie -> lowest index)   1: all three equal   2: an unnormalised quaternion
  3: row 2's quaternion negated and scaled   4: a gaussian behind the camera position's plane (the sign flips);
  the rest are drawn until |n . (p - c)| and the gap between the two smallest scales are >= 1e-3."""
  g = torch.Generator().manual_seed(1000 + seed + n)
  cam = torch.tensor([0.3, -0.2, -4.0], dtype=torch.float64)
  pos = torch.randn((n, 3), generator=g, dtype=torch.float64) * 1.5
  ls = torch.randn((n, 3), generator=g, dtype=torch.float64) * 0.7 - 2
  rot = torch.randn((n, 4), generator=g, dtype=torch.float64)
  for _ in range(20):
    m, gap = normal_margins(pos, ls, rot, cam)
    bad = (m < 1e-3) | (gap < 1e-3)
    if not bool(bad.any()):
      break
    count = int(bad.sum())
    pos[bad] = torch.randn((count, 3), generator=g, dtype=torch.float64) * 1.5
    ls[bad] = torch.randn((count, 3), generator=g, dtype=torch.float64) * 0.7 - 2
  planted = 0
  if n >= 63:
    planted = 5
    ls[0] = torch.tensor([-1.0, -2.5, -2.5], dtype=torch.float64)
    ls[1] = torch.tensor([-2.0, -2.0, -2.0], dtype=torch.float64)
    rot[2] = torch.tensor([3.0, -1.0, 0.5, 2.0], dtype=torch.float64)
    rot[3] = -0.01 * rot[2]
    ls[3] = ls[2]
    pos[3] = pos[2]
    pos[4] = torch.tensor([0.5, 0.1, -9.0], dtype=torch.float64)
  elif n == 1:
    ls[0] = torch.tensor([-2.0, -2.0, -2.0], dtype=torch.float64)         # the tie rule's axis on the one row
    planted = 1
  return pos, ls, rot, cam, planted


# ---- normal consistency -----------------------------------------------------------------------------------------------

def _unit(v):
  vv = v.square().sum(-1, keepdim=True)
  ok = vv.detach() >= TINY
  return torch.where(ok, v / torch.where(ok, vv, torch.ones_like(vv)).sqrt(), torch.zeros_like(v))


def points(accum, oz, oa, projection, alpha_min):
  """(P (H, W, 3), covered (H, W), u (W,), v (H,), d (H, W))"""
  h, w, _ = accum.shape
  fx, fy, cx, cy = projection.detach().unbind(0)
  alpha = accum[..., oa]
  ok = alpha.detach() >= alpha_min
  d = torch.where(ok, accum[..., oz] / torch.where(ok, alpha, torch.ones_like(alpha)), torch.zeros_like(alpha))
  u = (torch.arange(w, dtype=accum.dtype, device=accum.device) + 0.5 - cx) / fx
  v = (torch.arange(h, dtype=accum.dtype, device=accum.device) + 0.5 - cy) / fy
  return torch.stack([d * u[None, :], d * v[:, None], d], -1), ok, u, v, d


def stencil(accum, oz, oa, projection, alpha_min):
  """(a, b, c, indicator) on the (H - 2, W - 2) interior"""
  P, ok, _, _, _ = points(accum, oz, oa, projection, alpha_min)
  a = P[1:-1, 2:] - P[1:-1, :-2]
  b = P[2:, 1:-1] - P[:-2, 1:-1]
  ind = ok[1:-1, 1:-1] & ok[1:-1, 2:] & ok[1:-1, :-2] & ok[2:, 1:-1] & ok[:-2, 1:-1]
  return a, b, torch.linalg.cross(b, a), ind


def consistency(accum, oz, oa, on, projection, pixel_weight=None, alpha_min=0.5):
  """(loss, n_d (H, W, 3)) with autograd through accum"""
  h, w, _ = accum.shape
  nd_full = torch.zeros((h, w, 3), dtype=accum.dtype, device=accum.device)
  if h < 3 or w < 3:
    return accum.sum() * 0, nd_full
  _, _, c, ind = stencil(accum, oz, oa, projection, alpha_min)
  nd = _unit(c) * ind[..., None]
  nh = _unit(accum[1:-1, 1:-1, on:on + 3])
  weight = (accum[..., oa] if pixel_weight is None else pixel_weight).detach()[1:-1, 1:-1] * ind
  loss = (weight * (1 - (nh * nd).sum(-1))).sum() / ((h - 2) * (w - 2))
  nd_full[1:-1, 1:-1] = nd.detach()
  return loss, nd_full


def reference(accum, offsets, projection, pixel_weight=None, alpha_min=0.5, grad_loss=1.0):
  """(loss, n_d, d(grad_loss * loss)/d accum) of ``consistency`` in the inputs' dtype"""
  x = accum.clone().requires_grad_(True)
  loss, nd = consistency(x, *offsets, projection, pixel_weight, alpha_min)
  (loss * grad_loss).backward()
  return loss.detach(), nd, x.grad


def bounds(accum, offsets, projection, pixel_weight, alpha_min, eps, grad_loss=1.0):
  """the docstring's bounds from float64 quantities of ``accum``'s values: dict of loss, nd (H, W), grad (H, W, F),
  covered_nd (H, W) and covered_grad (H, W), cond (H - 2, W - 2 or empty)"""
  oz, oa, on = offsets
  x = accum.double()
  proj = projection.double()
  h, w, f = x.shape
  out = dict(loss=0.0, nd=torch.zeros((h, w), dtype=torch.float64), grad=torch.zeros((h, w, f), dtype=torch.float64),
             covered_nd=torch.ones((h, w), dtype=torch.bool), covered_grad=torch.ones((h, w), dtype=torch.bool),
             covered_depth_grad=torch.ones((h, w), dtype=torch.bool), cond=torch.zeros((0,), dtype=torch.float64), excluded=0.0)
  if h < 3 or w < 3:
    return out
  P, ok, u, v, d = points(x, oz, oa, proj, alpha_min)
  a, b, c, ind = stencil(x, oz, oa, proj, alpha_min)
  norm = lambda t: t.square().sum(-1).sqrt()
  na, nb, nc = norm(a), norm(b), norm(c)
  sum_x = norm(P[1:-1, 2:]) + norm(P[1:-1, :-2])
  sum_y = norm(P[2:, 1:-1]) + norm(P[:-2, 1:-1])
  safe = lambda t: torch.where(ind, t, torch.ones_like(t))
  cond = torch.where(ind, safe(na) * safe(nb) / safe(nc) * (sum_x / safe(na) + sum_y / safe(nb)), torch.zeros_like(na))
  good = cond <= CAP
  weight = (x[..., oa] if pixel_weight is None else pixel_weight.double())[1:-1, 1:-1] * ind
  pixels = (h - 2) * (w - 2)
  out['cond'] = cond[ind]
  out['excluded'] = float((ind & ~good).double().sum() / pixels)
  out['nd'][1:-1, 1:-1] = K * eps * cond
  out['covered_nd'][1:-1, 1:-1] = good
  out['loss'] = float(eps * (K * (weight * cond).sum() + K * 2 * weight.sum()) / pixels)
  wg = weight * abs(grad_loss) / pixels
  m = norm(x[1:-1, 1:-1, on:on + 3])
  m_ok = m.square() >= TINY
  out['grad'][1:-1, 1:-1, on:on + 3] = torch.where(m_ok, eps * wg / torch.where(m_ok, m, torch.ones_like(m)) * (K * cond + K),
                                                   torch.zeros_like(m))[..., None]
  E = torch.zeros((h, w), dtype=torch.float64)
  Ea, Eb = E.clone(), E.clone()
  e = torch.where(ind, eps * wg / safe(nc) * (4 * K * cond + K), torch.zeros_like(nc))
  Ea[1:-1, 1:-1], Eb[1:-1, 1:-1] = e * na, e * nb
  gd = torch.zeros((h, w), dtype=torch.float64)
  gd[:, 1:] += Eb[:, :-1]            # the centre to the left
  gd[:, :-1] += Eb[:, 1:]            # to the right
  gd[1:, :] += Ea[:-1, :]            # above
  gd[:-1, :] += Ea[1:, :]            # below
  gd = gd * (u.abs()[None, :] + v.abs()[:, None] + 1)
  alpha = torch.where(ok, x[..., oa], torch.ones_like(d))
  out['grad'][..., oz] = gd / alpha
  out['grad'][..., oa] = gd * d.abs() / alpha
  bad = torch.zeros((h, w), dtype=torch.bool)
  bad[1:-1, 1:-1] = ind & ~good
  out['covered_grad'] = ~bad
  near = bad.clone()
  near[:, 1:] |= bad[:, :-1]
  near[:, :-1] |= bad[:, 1:]
  near[1:, :] |= bad[:-1, :]
  near[:-1, :] |= bad[1:, :]
  out['covered_depth_grad'] = ~near
  return out


def excess(got, want, bound, covered=None):
  """max of |got - want| / bound (0 / 0 counts as 0, x / 0 as inf) over the covered elements"""
  err = (got.double() - want.double()).abs()
  bound = bound.expand_as(err) if isinstance(bound, torch.Tensor) else torch.full_like(err, bound)
  ratio = torch.where(err == 0, torch.zeros_like(err), err / bound)
  if covered is not None:
    ratio = ratio[covered.expand_as(ratio)]
  return float(ratio.max()) if ratio.numel() else 0.0


def default_projection(h, w):
  side = max(h, w, 8)
  return torch.tensor([1.1 * side, 1.05 * side, 0.5 * w + 0.3, 0.5 * h - 0.2], dtype=torch.float64)


def make_image(h, w, f=5, offsets=(0, 1, 2), seed=0):
  """float64 (accum (H, W, F), projection, pixel_weight): a tilted plane plus bounded bumps seen through the default
  camera; alpha from [0, 0.3] u [0.7, 1] with patches of exact 0 (nothing near alpha_min = 0.5); normal_sum = alpha times
  a perturbed surface normal, a few pixels exactly 0; every other channel random."""
  oz, oa, on = offsets
  g = torch.Generator().manual_seed(77 + 1000 * h + w + seed)
  proj = default_projection(h, w)
  xs = (torch.arange(w, dtype=torch.float64) + 0.5 - proj[2]) / proj[0]
  ys = (torch.arange(h, dtype=torch.float64) + 0.5 - proj[3]) / proj[1]
  px, py = torch.arange(w, dtype=torch.float64)[None, :], torch.arange(h, dtype=torch.float64)[:, None]
  depth = 4.0 / (1 + 0.6 * xs[None, :] - 0.45 * ys[:, None]) + 0.004 * torch.sin(0.7 * px + 0.3) * torch.cos(0.5 * py)
  alpha = torch.rand((h, w), generator=g, dtype=torch.float64) * 0.3
  high = torch.rand((h, w), generator=g, dtype=torch.float64) < 0.85
  alpha = torch.where(high, alpha + 0.7, alpha)
  if h >= 8 and w >= 8:
    alpha[h // 3:h // 3 + 2, w // 4:w // 4 + 3] = 0.0
    alpha[-2:, -3:] = 0.0
  elif h * w > 9:
    alpha[0, 0] = 0.0
  else:
    alpha = torch.where(high, alpha, alpha + 0.7)                         # (3, 3): the one interior pixel counts
  plane = torch.tensor([0.6, -0.45, -1.0], dtype=torch.float64)
  normal = plane / plane.norm() + 0.3 * torch.randn((h, w, 3), generator=g, dtype=torch.float64)
  accum = torch.randn((h, w, f), generator=g, dtype=torch.float64)
  accum[..., oz] = depth * alpha
  accum[..., oa] = alpha
  accum[..., on:on + 3] = normal * (alpha[..., None] + 0.05)
  if h >= 5 and w >= 5:
    accum[1, 1, on:on + 3] = 0.0
    accum[h // 2, w // 2, on:on + 3] = 0.0
  weight = torch.rand((h, w), generator=g, dtype=torch.float64) + 0.1
  return accum, proj, weight


def plane_image(h, w, normal, offset, projection):
  """accum (H, W, 5) of the plane normal . P = offset (alpha 1, normal_sum = normal)"""
  xs = (torch.arange(w, dtype=torch.float64) + 0.5 - projection[2]) / projection[0]
  ys = (torch.arange(h, dtype=torch.float64) + 0.5 - projection[3]) / projection[1]
  depth = offset / (normal[0] * xs[None, :] + normal[1] * ys[:, None] + normal[2])
  accum = torch.ones((h, w, 5), dtype=torch.float64)
  accum[..., 0] = depth
  accum[..., 2:5] = normal
  return accum
