"""Geometry images of a frame and the normal-consistency regulariser: per-gaussian normals (the shortest axis, turned to
the camera), a depth / alpha / normal feature image blended on the colour frame's own tile lists, and
``sum w (1 - n^ . n_d)`` between the blended normals and the normals of the blended depth, forward and backward in
``csrc/geometry.hip``.

The reference renders no normals; this is an addition.  There is no torch fallback: CPU tensors raise, as everywhere in
this package.  Every call runs on the current stream, allocates through torch only and never reads back to the host, so
it captures into ``frame.FrameGraph`` / ``torch.cuda.graph`` with the rest of a training step; the kernels have no atomics
and are bitwise reproducible.
"""
from __future__ import annotations

from dataclasses import dataclass
from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib
from .perspective.params import CameraParams
from .rasterizer.wide import render_features

TINY = 1e-30          # MS_NORMAL_TINY of include/mi355_splat.h


# ---- per-gaussian normals ---------------------------------------------------------------------------------------------

def _checked_normals(position, log_scaling, rotation, camera_position):
  n = position.shape[0] if position.dim() == 2 else -1
  if tuple(position.shape) != (n, 3) or tuple(log_scaling.shape) != (n, 3) or tuple(rotation.shape) != (n, 4):
    raise ValueError(f"position (N, 3), log_scaling (N, 3) and rotation (N, 4) expected (got {tuple(position.shape)}, "
                     f"{tuple(log_scaling.shape)}, {tuple(rotation.shape)})")
  if tuple(camera_position.shape) != (3,):
    raise ValueError(f"camera_position must be a 3-element tensor (got {tuple(camera_position.shape)})")
  tensors = (position, log_scaling, rotation, camera_position)
  if any(t.dtype != position.dtype or t.device != position.device for t in tensors):
    raise TypeError("position, log_scaling, rotation and camera_position differ in dtype or device ("
                    + ", ".join(f"{t.dtype} on {t.device}" for t in tensors) + ")")
  _lib.dtype_code(position.dtype)
  _lib.require_gpu(*tensors)


def gaussian_normals_forward(position, log_scaling, rotation, camera_position):
  """One ms_gaussian_normals_fwd launch on contiguous tensors: ``(normals (N, 3), code (N,) uint8)``."""
  n = position.shape[0]
  normals = torch.empty((n, 3), dtype=position.dtype, device=position.device)
  code = torch.empty((n,), dtype=torch.uint8, device=position.device)
  _lib.check(_lib.load().ms_gaussian_normals_fwd(_lib.ptr(position), _lib.ptr(log_scaling), _lib.ptr(rotation),
                                                 _lib.ptr(camera_position), n, _lib.dtype_code(position.dtype),
                                                 normals.data_ptr(), code.data_ptr(),
                                                 _lib.current_stream(position.device)), "gaussian_normals")
  return normals, code


def gaussian_normals_backward(rotation, code, grad_normals):
  """dL/drotation (N, 4) of one ms_gaussian_normals_bwd launch."""
  grad = torch.empty_like(rotation)
  _lib.check(_lib.load().ms_gaussian_normals_bwd(_lib.ptr(rotation), _lib.ptr(code), _lib.ptr(grad_normals),
                                                 rotation.shape[0], _lib.dtype_code(rotation.dtype), grad.data_ptr(),
                                                 _lib.current_stream(rotation.device)), "gaussian_normals backward")
  return grad


class _GaussianNormals(torch.autograd.Function):

  @staticmethod
  def forward(ctx, position, log_scaling, rotation, camera_position):
    q = rotation.detach().contiguous()
    normals, code = gaussian_normals_forward(position.detach().contiguous(), log_scaling.detach().contiguous(), q,
                                             camera_position.detach().contiguous())
    ctx.save_for_backward(q, code)
    return normals

  @staticmethod
  @once_differentiable
  def backward(ctx, grad_normals):
    if not ctx.needs_input_grad[2]:
      return None, None, None, None
    q, code = ctx.saved_tensors
    return None, None, gaussian_normals_backward(q, code, grad_normals.to(dtype=q.dtype).contiguous()), None


def gaussian_normals(gaussians, camera_position: torch.Tensor) -> torch.Tensor:
  """``(N, 3)`` unit normals of ``gaussians`` (a ``Gaussians3D``) in the world frame: column ``k`` of the rotation matrix
  of ``rotation / |rotation|`` (xyzw), ``k`` the index of the smallest ``log_scaling`` entry, negated where
  ``normal . (position - camera_position) > 0`` so that it faces the camera (exactly 0 keeps the sign).
  ``camera_position`` is a 3-element DEVICE tensor of the gaussians' dtype (``camera.camera_position``), read by the
  kernel.

  Ties take the lowest index: two equal smallest scales give the first of them, and an isotropic gaussian (all three
  equal, which is how ``Gaussians3D.from_point_cloud`` scenes start) gets its x axis, column 0, until training separates
  the scales.

  Differentiable (once) in ``rotation`` ONLY, through the unnormalised quaternion.  The axis choice ``k`` and the sign
  are piecewise constant, so ``position``, ``log_scaling`` and ``camera_position`` receive no gradient from here (their
  ``.grad`` stays ``None``); where ``rotation`` needs no gradient no backward kernel is launched.  float32 / float64 GPU
  tensors (non-contiguous inputs are copied)."""
  _checked_normals(gaussians.position, gaussians.log_scaling, gaussians.rotation, camera_position)
  return _GaussianNormals.apply(gaussians.position, gaussians.log_scaling, gaussians.rotation, camera_position)


# ---- geometry images --------------------------------------------------------------------------------------------------

@dataclass(frozen=True)
class GeometryImages:
  """The blended geometry features of one frame: ``accum`` ``(H, W, F)`` with channel ``depth_offset`` = sum w z,
  ``alpha_offset`` = sum w (the differentiable ones channel: ``Rendering.image_weight`` carries no gradient),
  ``depth_sq_offset`` = sum w z^2 and ``normal_offset .. + 2`` = sum w n in the camera frame (``None`` where not
  rendered), w the blending weights of the colour image."""
  accum: torch.Tensor
  camera: CameraParams
  depth_offset: int = 0
  alpha_offset: int = 1
  depth_sq_offset: Optional[int] = None
  normal_offset: Optional[int] = None
  alpha_min: float = 0.5

  @property
  def depth_sum(self) -> torch.Tensor:
    return self.accum[..., self.depth_offset]

  @property
  def alpha(self) -> torch.Tensor:
    return self.accum[..., self.alpha_offset]

  @property
  def depth_sq_sum(self) -> torch.Tensor:
    if self.depth_sq_offset is None:
      raise ValueError("no depth_sq_sum: render_geometry(..., depth_variance=True) renders it")
    return self.accum[..., self.depth_sq_offset]

  @property
  def normal_sum(self) -> torch.Tensor:
    if self.normal_offset is None:
      raise ValueError("no normal_sum: render_geometry(..., normals=True) renders it")
    return self.accum[..., self.normal_offset:self.normal_offset + 3]

  @property
  def covered(self) -> torch.Tensor:
    return self.alpha.detach() >= self.alpha_min

  @property
  def depth(self) -> torch.Tensor:
    """``depth_sum / alpha`` where ``alpha >= alpha_min``, else 0 (and no gradient)"""
    ok = self.covered
    return torch.where(ok, self.depth_sum / torch.where(ok, self.alpha, torch.ones_like(self.alpha)), 0.0)

  @property
  def normal(self) -> torch.Tensor:
    """``normal_sum / |normal_sum|`` where ``|normal_sum|^2 >= TINY``, else 0"""
    m = self.normal_sum
    mm = m.square().sum(-1, keepdim=True)
    ok = mm.detach() >= TINY
    return torch.where(ok, m / torch.where(ok, mm, torch.ones_like(mm)).sqrt(), 0.0)

  @property
  def depth_variance(self) -> torch.Tensor:
    """``depth_sq_sum / alpha - depth^2`` where ``alpha >= alpha_min``, else 0"""
    ok = self.covered
    mean_sq = self.depth_sq_sum / torch.where(ok, self.alpha, torch.ones_like(self.alpha))
    return torch.where(ok, mean_sq - self.depth.square(), 0.0)

  @property
  def distortion(self) -> torch.Tensor:
    """``alpha depth_sq_sum - depth_sum^2``: the depth-distortion term of the blended moments"""
    return self.alpha * self.depth_sq_sum - self.depth_sum.square()


def geometry_features(gaussians, camera: CameraParams, normals: bool = True, depth_variance: bool = False) -> torch.Tensor:
  """The ``(N, F)`` float32 feature rows ``[z, 1, (z^2), (n_cam)]`` that ``render_geometry`` blends, through autograd:
  ``z = position @ T_camera_world[2, :3] + T_camera_world[2, 3]``,
  ``n_cam = gaussian_normals(gaussians, camera_position) @ T_camera_world[:3, :3].T``."""
  T = camera.T_camera_world.to(gaussians.position.dtype)
  z = gaussians.position @ T[2, :3] + T[2, 3]
  columns = [z[:, None], torch.ones_like(z)[:, None]]
  if depth_variance:
    columns.append(z.square()[:, None])
  if normals:
    centre = camera.detach().camera_position.to(gaussians.position.dtype)
    columns.append(gaussian_normals(gaussians, centre) @ T[:3, :3].T)
  return torch.cat(columns, dim=1).to(torch.float32)


def render_geometry(rendering, gaussians, *, normals: bool = True, depth_variance: bool = False,
                    alpha_min: float = 0.5) -> GeometryImages:
  """Geometry images of the frame ``rendering`` (of ``render_gaussians(gaussians, rendering.camera, ...)``): one
  ``render_features`` call of ``F = 2 .. 6`` channels ``[z, 1, (z^2), (n_cam)]`` per INPUT gaussian on the colour image's
  own tile lists, so that the geometry gradient joins the frame's one backward pass and the pose gets its gradient through
  ``z`` and ``n_cam``.  A rendering that does not come from the frame executor, or of a tile-row strip, raises what
  ``render_features`` raises.  ``alpha_min`` is the coverage under which ``.depth`` and ``.depth_variance`` are 0."""
  if not alpha_min > 0:
    raise ValueError(f"alpha_min > 0 expected (got {alpha_min})")
  rows = geometry_features(gaussians, rendering.camera, normals, depth_variance)
  accum = render_features(rendering, rows)
  return GeometryImages(accum=accum, camera=rendering.camera, depth_offset=0, alpha_offset=1,
                        depth_sq_offset=2 if depth_variance else None,
                        normal_offset=(3 if depth_variance else 2) if normals else None, alpha_min=float(alpha_min))


# ---- normal consistency -----------------------------------------------------------------------------------------------

def _checked_consistency(accum, depth_offset, alpha_offset, normal_offset, projection, pixel_weight, alpha_min):
  if normal_offset is None:
    raise ValueError("normal_consistency_loss needs the normal channels (render_geometry(..., normals=True))")
  if accum.dim() != 3:
    raise ValueError(f"accum must be (H, W, F) (got {tuple(accum.shape)})")
  h, w, f = accum.shape
  if h < 1 or w < 1:
    raise ValueError(f"empty image {tuple(accum.shape)}")
  offsets = [int(depth_offset), int(alpha_offset)] + [int(normal_offset) + k for k in range(3)]
  if f < 5 or min(offsets) < 0 or max(offsets) >= f or len(set(offsets)) != 5:
    raise ValueError(f"depth, alpha and three normal channels must be distinct channels of the (H, W, {f}) image "
                     f"(got offsets {depth_offset}, {alpha_offset}, {normal_offset})")
  if h * w * f >= 2 ** 31:
    raise ValueError(f"image too large {tuple(accum.shape)}")
  if not float(alpha_min) > 0.0:
    raise ValueError(f"alpha_min > 0 expected (got {alpha_min})")
  if tuple(projection.shape) != (4,):
    raise ValueError(f"projection must be (fx, fy, cx, cy) (got {tuple(projection.shape)})")
  if projection.requires_grad:
    raise NotImplementedError("normal_consistency_loss: no gradient with respect to projection (detach it)")
  tensors = [accum, projection]
  if pixel_weight is not None:
    if tuple(pixel_weight.shape) != (h, w):
      raise ValueError(f"pixel_weight must be (H, W) = ({h}, {w}) (got {tuple(pixel_weight.shape)})")
    tensors.append(pixel_weight)
  if any(t.dtype != accum.dtype or t.device != accum.device for t in tensors):
    raise TypeError("accum, projection and pixel_weight differ in dtype or device ("
                    + ", ".join(f"{t.dtype} on {t.device}" for t in tensors) + ")")
  _lib.dtype_code(accum.dtype)
  _lib.require_gpu(*tensors)


def normal_consistency_forward(accum, offsets, projection, pixel_weight, alpha_min: float, want_normals: bool):
  """One ms_normal_consistency_fwd call on contiguous tensors: ``(loss (0-dim), n_d (H, W, 3) | None)``."""
  lib = _lib.load()
  h, w, f = accum.shape
  dtype, stream = _lib.dtype_code(accum.dtype), _lib.current_stream(accum.device)
  out = torch.empty((1,), dtype=accum.dtype, device=accum.device)
  depth_normals = torch.empty((h, w, 3), dtype=accum.dtype, device=accum.device) if want_normals else None
  _lib.run_with_scratch(lambda tmp, size: lib.ms_normal_consistency_fwd(
    _lib.ptr(accum), _lib.ptr(pixel_weight), _lib.ptr(projection), h, w, f, *offsets, dtype, alpha_min, tmp, size,
    out.data_ptr(), _lib.ptr(depth_normals), stream), accum.device, "normal_consistency_loss")
  return out[0], depth_normals


def normal_consistency_backward(accum, offsets, projection, pixel_weight, alpha_min: float, grad_loss) -> torch.Tensor:
  """dloss/daccum (H, W, F), written whole by one launch; ``grad_loss`` is a one-element DEVICE tensor."""
  h, w, f = accum.shape
  grad = torch.empty_like(accum)
  _lib.check(_lib.load().ms_normal_consistency_bwd(_lib.ptr(accum), _lib.ptr(pixel_weight), _lib.ptr(projection),
                                                   _lib.ptr(grad_loss), h, w, f, *offsets, _lib.dtype_code(accum.dtype),
                                                   alpha_min, grad.data_ptr(), _lib.current_stream(accum.device)),
             "normal_consistency_loss backward")
  return grad


class _NormalConsistency(torch.autograd.Function):

  @staticmethod
  def forward(ctx, accum, projection, pixel_weight, offsets, alpha_min, want_normals):
    x = accum.detach().contiguous()
    proj = projection.detach().contiguous()
    weight = None if pixel_weight is None else pixel_weight.detach().contiguous()
    loss, depth_normals = normal_consistency_forward(x, offsets, proj, weight, alpha_min, want_normals)
    ctx.save_for_backward(x, proj, weight)
    ctx.args = (offsets, alpha_min)
    if depth_normals is None:
      depth_normals = x.new_empty((0, 0, 3))
    ctx.mark_non_differentiable(depth_normals)
    return loss, depth_normals

  @staticmethod
  @once_differentiable
  def backward(ctx, grad_loss, _grad_normals):
    if not ctx.needs_input_grad[0]:
      return None, None, None, None, None, None
    x, proj, weight = ctx.saved_tensors
    offsets, alpha_min = ctx.args
    go = grad_loss.to(dtype=x.dtype).reshape(1).contiguous()       # stays on the device: the kernel reads it through a pointer
    return normal_consistency_backward(x, offsets, proj, weight, alpha_min, go), None, None, None, None, None


def normal_consistency(accum: torch.Tensor, depth_offset: int, alpha_offset: int, normal_offset: int,
                       projection: torch.Tensor, *, pixel_weight: Optional[torch.Tensor] = None, alpha_min: float = 0.5,
                       return_normals: bool = False):
  """The tensor-level form of ``normal_consistency_loss``: ``accum`` ``(H, W, F)`` with ``depth_sum`` in channel
  ``depth_offset``, ``alpha`` in ``alpha_offset`` and ``normal_sum`` in ``normal_offset .. normal_offset + 2`` (five
  distinct channels, in any order), ``projection`` the 4-element DEVICE tensor ``(fx, fy, cx, cy)``."""
  _checked_consistency(accum, depth_offset, alpha_offset, normal_offset, projection, pixel_weight, alpha_min)
  if pixel_weight is not None and pixel_weight.requires_grad:
    pixel_weight = pixel_weight.detach()                           # a weight, never differentiated
  loss, depth_normals = _NormalConsistency.apply(accum, projection, pixel_weight,
                                                 (int(depth_offset), int(alpha_offset), int(normal_offset)),
                                                 float(alpha_min), bool(return_normals))
  return (loss, depth_normals) if return_normals else loss


def normal_consistency_loss(geometry: GeometryImages, *, pixel_weight: Optional[torch.Tensor] = None,
                            alpha_min: float = 0.5, return_normals: bool = False):
  """``sum w (1 - n^ . n_d) / ((H - 2)(W - 2))`` over the interior pixels as a 0-dim tensor, differentiable (once) in
  ``geometry.accum``: ``n^`` the normalised blended normal, ``n_d`` the normal of the blended depth,

    d = depth_sum / alpha     P = d ((x + 0.5 - cx) / fx, (y + 0.5 - cy) / fy, 1)
    n_d = c / |c|,  c = (P(x, y + 1) - P(x, y - 1)) x (P(x + 1, y) - P(x - 1, y))

  which faces the camera as ``gaussian_normals`` does (a fronto-parallel plane gives ``(0, 0, -1)``); a ``c`` or a
  ``normal_sum`` of squared length under 1e-30 counts as 0 and has no gradient.  The weight ``w`` is ``pixel_weight``
  ``(H, W)``, by default ``alpha``, taken as a constant either way, times the indicator that the pixel and its four
  neighbours all have ``alpha >= alpha_min`` (``> 0`` required).  Images with ``H < 3`` or ``W < 3`` give exactly 0 and
  zero gradients.  The camera's ``projection`` is read on the device (it may change between graph replays) and gets no
  gradient: one that requires grad raises.  ``return_normals``: ``(loss, n_d)`` with the non-differentiable ``(H, W, 3)``
  map of the same launch, for viewing and for supervision with normal priors.  One forward launch (+ a fixed-order
  reduction), one backward launch; bitwise reproducible."""
  return normal_consistency(geometry.accum, geometry.depth_offset, geometry.alpha_offset, geometry.normal_offset,
                            geometry.camera.projection.to(geometry.accum.dtype), pixel_weight=pixel_weight,
                            alpha_min=alpha_min, return_normals=return_normals)
