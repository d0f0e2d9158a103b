"""Oracles of the bilateral-grid slice (csrc/bilagrid.hip, taichi_splatting_amd/appearance.py), both on the CPU:

* ``slice_grid_sample``: the composition a user writes from torch's 5-D ``grid_sample(bilinear, border,
  align_corners=True)``, differentiable by autograd (dtype of its inputs: float64 as the oracle, float32 as the
  independent implementation that must also hold the GPU tests' bounds);
* ``slice_loop``: a literal per-pixel loop over the formulas of include/mi355_splat.h, with both gradients written out.

and the error bounds of the GPU tests (``bounds``), with the inputs they use (``make_case``)."""
import math

import torch
import torch.nn.functional as F

LUM = (0.299, 0.587, 0.114)


def make_case(H, W, L, Gy, Gx, seed=0, dtype=torch.float64):
  """image rand 1.6 - 0.3 per channel (luminance on both sides of the clamp), grid = identity + 0.3 randn, upstream randn"""
  gen = torch.Generator().manual_seed(1000 * seed + 7)
  image = torch.rand((H, W, 3), generator=gen, dtype=torch.float64) * 1.6 - 0.3
  eye = torch.eye(3, 4, dtype=torch.float64).reshape(12, 1, 1, 1)
  grid = eye + 0.3 * torch.randn((12, L, Gy, Gx), generator=gen, dtype=torch.float64)
  grad_out = torch.randn((H, W, 3), generator=gen, dtype=torch.float64)
  return image.to(dtype), grid.to(dtype), grad_out.to(dtype)


def luminance(image):
  return image[..., 0] * LUM[0] + image[..., 1] * LUM[1] + image[..., 2] * LUM[2]


def slice_grid_sample(image, grid):
  H, W, _ = image.shape
  u = (torch.arange(W, dtype=image.dtype, device=image.device) + 0.5) / W
  v = (torch.arange(H, dtype=image.dtype, device=image.device) + 0.5) / H
  z = luminance(image).clamp(0, 1)
  coords = torch.stack([(2 * u - 1).expand(H, W), (2 * v - 1)[:, None].expand(H, W), 2 * z - 1], -1)     # x -> Gx, y -> Gy, z -> L
  planes = F.grid_sample(grid[None], coords[None, None], mode='bilinear', padding_mode='border', align_corners=True)
  A = planes[0, :, 0].permute(1, 2, 0).reshape(H, W, 3, 4)
  return (A[..., :3] * image[..., None, :]).sum(-1) + A[..., 3]


def reference(image, grid, grad_out):
  """(out, grad_image, grad_grid) of the grid_sample composition and its autograd"""
  x, g = image.clone().requires_grad_(True), grid.clone().requires_grad_(True)
  out = slice_grid_sample(x, g)
  out.backward(grad_out)
  return out.detach(), x.grad, g.grad


def _cell(coord, size):
  i = max(min(int(math.floor(coord)), size - 2), 0)
  return i, coord - i


def slice_loop(image, grid, grad_out):
  """(out, grad_image, grad_grid) pixel by pixel, float64"""
  H, W, _ = image.shape
  _, L, Gy, Gx = grid.shape
  out, grad_image, grad_grid = torch.zeros_like(image), torch.zeros_like(image), torch.zeros_like(grid)
  lumc = torch.tensor(LUM, dtype=image.dtype)
  for y in range(H):
    for x in range(W):
      p = image[y, x]
      p1 = torch.cat([p, torch.ones(1, dtype=image.dtype)])
      g = grad_out[y, x]
      lum = float(p @ lumc)
      gx, gy = (x + 0.5) / W * (Gx - 1), (y + 0.5) / H * (Gy - 1)
      gz = min(max(lum, 0.0), 1.0) * (L - 1)
      (ix, fx), (iy, fy), (iz, fz) = _cell(gx, Gx), _cell(gy, Gy), _cell(gz, L)
      A, dA = torch.zeros(12, dtype=image.dtype), torch.zeros(12, dtype=image.dtype)
      gp = (g[:, None] * p1[None, :]).reshape(12)
      for dz in range(min(2, L)):
        for dy in range(min(2, Gy)):
          for dx in range(min(2, Gx)):
            # hat weights max(0, 1 - |coord - vertex|) on the clamped coordinates; a size-1 axis weighs 1
            wz = max(0.0, 1 - abs(gz - (iz + dz))) if L > 1 else 1.0
            wy = max(0.0, 1 - abs(gy - (iy + dy))) if Gy > 1 else 1.0
            wx = max(0.0, 1 - abs(gx - (ix + dx))) if Gx > 1 else 1.0
            c = grid[:, iz + dz, iy + dy, ix + dx]
            A += wz * wy * wx * c
            dA += (1.0 if dz else -1.0) * wy * wx * c if L > 1 else 0.0
            grad_grid[:, iz + dz, iy + dy, ix + dx] += wz * wy * wx * gp
      A34 = A.reshape(3, 4)
      out[y, x] = A34[:, :3] @ p + A34[:, 3]
      guide = (L - 1) * float(dA @ gp) if 0.0 < lum < 1.0 else 0.0
      grad_image[y, x] = A34[:, :3].T @ g + guide * lumc
  return out, grad_image, grad_grid


def footprint_abs_sum(image, grad_out, Gy, Gx):
  """S[c, j, yv, xv]: the unweighted sum of |g_c| |p1_j| over the pixels of a vertex's xy footprint |gx - xv| < 1,
  |gy - yv| < 1 (all luminance bins share it)"""
  H, W, _ = image.shape
  image, grad_out = image.double(), grad_out.double()
  gx = (torch.arange(W, dtype=torch.float64) + 0.5) / W * (Gx - 1)
  gy = (torch.arange(H, dtype=torch.float64) + 0.5) / H * (Gy - 1)
  mx = ((gx[None, :] - torch.arange(Gx, dtype=torch.float64)[:, None]).abs() < 1).double()       # (Gx, W)
  my = ((gy[None, :] - torch.arange(Gy, dtype=torch.float64)[:, None]).abs() < 1).double()       # (Gy, H)
  p1 = torch.cat([image.abs(), torch.ones((H, W, 1), dtype=torch.float64)], -1)
  terms = grad_out.abs()[..., :, None] * p1[..., None, :]                                            # (H, W, 3, 4)
  return torch.einsum('yh,hwcj,xw->cjyx', my, terms, mx)


def bounds(image, grid, grad_out, eps):
  """The three error bounds (float64 tensors) for unit roundoff ``eps``, and the pixels the image-gradient bound covers:
  out (H, W), grad_grid (12, L, Gy, Gx), grad_image (H, W), covered (H, W) bool."""
  image, grid, grad_out = image.double(), grid.double(), grad_out.double()
  _, L, Gy, Gx = grid.shape
  G = max(L, Gy, Gx)
  gmax = float(grid.abs().max())
  mass = image.abs().sum(-1) + 1
  out = 16 * eps * G * gmax * mass
  S = footprint_abs_sum(image, grad_out, Gy, Gx)                                     # (3, 4, Gy, Gx)
  grad_grid = (16 * eps * G * S).reshape(12, 1, Gy, Gx).expand(12, L, Gy, Gx)
  grad_image = 16 * eps * G * max(L - 1, 1) * gmax * grad_out.abs().sum(-1) * mass
  t = luminance(image) * (L - 1)
  nearest = t.round()
  covered = ~(((t - nearest).abs() < 1e-4) & (nearest >= 0) & (nearest <= L - 1)) if L > 1 else torch.ones_like(t, dtype=torch.bool)
  return dict(out=out, grad_grid=grad_grid, grad_image=grad_image, covered=covered, S=S)


def unit_roundoff(dtype):
  return torch.finfo(dtype).eps / 2


def excess(got, want, bound, mask=None):
  """largest |got - want| / bound (0 / 0 counts as 0: where the bound is 0 the values must be equal)"""
  diff = (got.double() - want.double()).abs()
  ratio = torch.where(diff == 0, torch.zeros_like(diff), diff / bound)
  if mask is not None:
    ratio = ratio[mask]                                   # a (H, W) mask on a (H, W, 3) tensor keeps whole pixels
  return float(ratio.max()) if ratio.numel() else 0.0
