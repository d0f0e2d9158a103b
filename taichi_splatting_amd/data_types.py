"""Data model of the renderer: same names, fields and defaults as the reference.

Mirrors reference ``taichi_splatting/data_types.py``: ``RasterConfig`` (:17-47),
``Gaussians3D`` (:57-115), ``Gaussians2D`` (:122-145).  tensordict / beartype / roma are not
required: containers derive from the in-repo :class:`TensorClass`.
"""
from __future__ import annotations

from dataclasses import dataclass
import math
from typing import List, Optional, Tuple

import torch

from .tensorclass import TensorClass


@dataclass(frozen=True, eq=True, kw_only=True)
class RasterConfig:
  """Rasterizer configuration (reference ``data_types.py:17-47``; identical defaults).

  Frozen + hashable so it can be used as a cache key and with ``dataclasses.replace``.
  """
  tile_size: int = 16

  # pixel tiling per thread in the backward pass.  The reference uses it to pick the
  # thread->pixel map; results never depend on it.  The gfx950 kernels always map one wave64
  # to an 8x8 pixel patch, so the value is validated and otherwise ignored.
  pixel_stride: Tuple[int, int] = (2, 2)

  # clamp position to within this margin of the image for the affine jacobian
  clamp_margin: float = 0.15

  antialias: bool = False       # use the anti-aliased pdf
  blur_cov: float = 0.3         # added to the diagonal of the projected covariance

  clamp_max_alpha: float = 0.99
  alpha_threshold: float = 1. / 255.

  saturate_threshold: float = 0.9999   # backward stops at this accumulated weight
  use_alpha_blending: bool = True      # False + saturate_threshold => quantile (median) render

  compute_point_heuristic: bool = False
  compute_visibility: bool = False

  median_threshold: float = 0.25

  def __post_init__(self):
    assert self.tile_size in (8, 16, 32), \
      f"tile_size must be 8, 16 or 32 (one wave64 per 8x8 pixel patch), got {self.tile_size}"
    sx, sy = self.pixel_stride
    assert self.tile_size % sx == 0 and self.tile_size % sy == 0, \
      f"pixel_stride {self.pixel_stride} must divide tile_size {self.tile_size}"
    # reference rasterizer/backward.py:32-33
    assert (self.tile_size * self.tile_size) // (sx * sy) >= 32, \
      f"pixel_stride {self.pixel_stride} and tile_size {self.tile_size} must allow at least one warp sized (32) tile"


SH_C0 = 0.28209479177387814    # Y_0^0: colour = 0.5 + SH_C0 * coefficient 0 for a degree-0 feature


def check_packed3d(packed_gaussians: torch.Tensor):
  assert len(packed_gaussians.shape) == 2 and packed_gaussians.shape[1] == 11, \
    f"Expected shape (N, 11), got {packed_gaussians.shape}"


def check_packed2d(packed_gaussians: torch.Tensor):
  # the packed 2D gaussian is 7 floats [mean.xy, axis.xy, sigma.xy, alpha] (taichi_lib/generic.py:30-58)
  assert len(packed_gaussians.shape) == 2 and packed_gaussians.shape[1] == 7, \
    f"Expected shape (N, 7), got {packed_gaussians.shape}"


def _quat_to_mat(q: torch.Tensor) -> torch.Tensor:
  x, y, z, w = q.unbind(-1)
  x2, y2, z2 = x * x, y * y, z * z
  return torch.stack([
    1 - 2 * y2 - 2 * z2, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
    2 * x * y + 2 * w * z, 1 - 2 * x2 - 2 * z2, 2 * y * z - 2 * w * x,
    2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x2 - 2 * y2], dim=-1).reshape(q.shape[:-1] + (3, 3))


def _mat_to_quat(m: torch.Tensor) -> torch.Tensor:
  """Rotation matrix -> unit quaternion (xyzw), numerically robust branch selection."""
  m00, m11, m22 = m[..., 0, 0], m[..., 1, 1], m[..., 2, 2]
  qw = torch.sqrt(torch.clamp_min(1 + m00 + m11 + m22, 0)) / 2
  qx = torch.sqrt(torch.clamp_min(1 + m00 - m11 - m22, 0)) / 2
  qy = torch.sqrt(torch.clamp_min(1 - m00 + m11 - m22, 0)) / 2
  qz = torch.sqrt(torch.clamp_min(1 - m00 - m11 + m22, 0)) / 2
  qx = torch.copysign(qx, m[..., 2, 1] - m[..., 1, 2])
  qy = torch.copysign(qy, m[..., 0, 2] - m[..., 2, 0])
  qz = torch.copysign(qz, m[..., 1, 0] - m[..., 0, 1])
  q = torch.stack([qx, qy, qz, qw], dim=-1)
  return q / torch.norm(q, dim=-1, keepdim=True)


class Gaussians3D(TensorClass):
  """3D gaussians (reference ``data_types.py:57``).  ``rotation`` is an xyzw quaternion."""
  position: torch.Tensor      # 3  - xyz
  log_scaling: torch.Tensor   # 3  - scale = exp(log_scaling)
  rotation: torch.Tensor      # 4  - quaternion xyzw (normalised inside the kernels)
  alpha_logit: torch.Tensor   # 1  - alpha = sigmoid(alpha_logit)
  feature: torch.Tensor       # (N, C) colours or (N, 3, (deg+1)^2) spherical harmonics

  def __post_init__(self):
    assert self.position.shape[1] == 3, f"Expected shape (N, 3), got {self.position.shape}"
    assert self.log_scaling.shape[1] == 3, f"Expected shape (N, 3), got {self.log_scaling.shape}"
    assert self.rotation.shape[1] == 4, f"Expected shape (N, 4), got {self.rotation.shape}"
    assert self.alpha_logit.shape[1] == 1, f"Expected shape (N, 1), got {self.alpha_logit.shape}"

  def packed(self):
    return torch.cat([self.position, self.log_scaling, self.rotation, self.alpha_logit], dim=-1)

  def shape_tensors(self):
    return (self.position, self.log_scaling, self.rotation, self.alpha_logit)

  def scaled(self, scale: float) -> 'Gaussians3D':
    return self.replace(position=self.position * scale,
                        log_scaling=math.log(scale) + self.log_scaling)

  def translated(self, translation: torch.Tensor) -> 'Gaussians3D':
    return self.replace(position=self.position + translation.view(1, 3))

  @property
  def scale(self):
    return torch.exp(self.log_scaling)

  @property
  def alpha(self):
    return torch.sigmoid(self.alpha_logit)

  def transform_rigid(self, m: torch.Tensor) -> 'Gaussians3D':
    """Transform the gaussians by a rigid 4x4 matrix (reference ``data_types.py:91-102``).
    Like the reference it leaves SH coefficients alone; ``transformed`` rotates them too."""
    assert m.shape == (4, 4), f"Expected shape (4, 4), got {m.shape}"
    r, t = m[:3, :3], m[:3, 3]
    position = self.position @ r.T + t
    q = self.rotation / torch.norm(self.rotation, dim=-1, keepdim=True)
    rotation = _mat_to_quat(r.unsqueeze(0) @ _quat_to_mat(q))
    return self.replace(position=position, rotation=rotation)

  def transformed(self, m: torch.Tensor, *, rotate_sh: bool = True, inplace: bool = False) -> 'Gaussians3D':
    """The scene in another world frame: ``m = [[s R, t], [0, 1]]`` with ``R`` a proper rotation and ``s > 0``, applied
    by one kernel launch (``ms_scene_transform``, csrc/scene_transform.hip; no reference counterpart).

    ``position' = s R p + t``, ``log_scaling' = log_scaling + ln s``, ``rotation' = q_R (x) q`` (xyzw; the row is not
    normalised, the kernels normalise on read), ``alpha_logit`` unchanged.  SH features (N, F, (D+1)^2) are rotated band
    by band, ``c'_l = M_l(R) c_l`` (``spherical_harmonics.sh_rotation_matrices``), so that the moved scene shows from
    the moved camera ``diag(s, s, s, 1) T_camera_world m^-1`` (near and far times ``s``) what the old one showed from
    the old; ``rotate_sh=False`` leaves them alone, which is what ``transform_rigid`` does.  (N, C) colours and degree-0
    features do not change and are shared with ``self``.

    ``inplace=True`` writes into the scene's own tensors (no N x 48 temporary) and returns ``self``; tensors that
    require grad are refused outside ``torch.no_grad()``.  The tensors must be on the GPU, float32 or float64.
    ``m`` is validated on the host in float64: a reflection, shear or non-uniform scale raises ``ValueError``.

    Out of scope: gradients with respect to ``m`` (the result is detached from ``self``), optimiser moments (the second
    moment does not transform linearly: reset the optimiser state of a transformed scene) and reflections."""
    from . import _lib
    from .spherical_harmonics import pack_scene_transform, scene_transform, check_sh_degree
    s, r, t = similarity_from_matrix(m)
    geometry = (self.position, self.log_scaling, self.rotation)
    _lib.require_gpu(*geometry, self.feature)
    for x in (*geometry, self.feature):
      _lib.dtype_code(x.dtype)
    degree = check_sh_degree(self.feature) if self.feature.ndim == 3 else 0
    if not 0 <= degree <= 3:
      raise ValueError(f"SH degree must be between 0 and 3, got {degree}")
    with_feature = bool(rotate_sh) and degree >= 1
    fields = geometry + ((self.feature,) if with_feature else ())
    if not all(x.dtype == self.position.dtype and x.is_contiguous() for x in fields):
      raise ValueError("transformed: contiguous tensors of one dtype expected")
    if inplace:
      if torch.is_grad_enabled() and any(x.requires_grad for x in fields):
        raise RuntimeError("transformed(inplace=True) would overwrite tensors that require grad: "
                           "call it under torch.no_grad()")
      outs = [x.detach() for x in fields]
    else:
      outs = [torch.empty_like(x, requires_grad=False) for x in fields]
    packed = pack_scene_transform(s, r, t, max(degree, 1))
    ins = [x.detach() for x in fields]
    scene_transform(packed, position=ins[0], log_scaling=ins[1], rotation=ins[2], feature=ins[3] if with_feature else None,
                    out_position=outs[0], out_log_scaling=outs[1], out_rotation=outs[2],
                    out_feature=outs[3] if with_feature else None)
    if inplace:
      return self
    return self.replace(position=outs[0], log_scaling=outs[1], rotation=outs[2],
                        feature=outs[3] if with_feature else self.feature)

  def with_filter_3d(self, sigma: torch.Tensor) -> 'Gaussians3D':
    """The scene with an isotropic 3-D smoothing filter of standard deviation ``sigma`` (n,) baked in, as Mip-Splatting
    fuses its filter after training (no reference counterpart; ``misc.coverage.Coverage.filter_sigma`` gives the sigma
    a camera set calls for).  Per axis ``s'^2 = s^2 + sigma^2``; the opacity keeps the gaussian's integral,
    ``alpha' = alpha sqrt(prod s^2 / prod s'^2)``.  Both are evaluated through the per-axis growth
    ``s'^2 / s^2 = 1 + (sigma / s)^2``: ``log_scaling' = log_scaling + log1p((sigma / s)^2) / 2`` (a small correction is
    added to the stored value, not recovered from a logarithm of s'^2), ``alpha'`` from the product of the three
    ``1 / sqrt(growth)``, stored as ``alpha_logit' = log(alpha') - log1p(-alpha')``.  ``position``, ``rotation`` and ``feature`` are shared with ``self``.

    A plain differentiable torch composition, on purpose: this is an offline operation, and autograd flows to
    ``log_scaling`` and ``alpha_logit``.  Rows with ``sigma == 0`` keep their ``log_scaling`` and ``alpha_logit`` bitwise
    (``torch.where`` on the inputs).  Raises ValueError on a ``sigma`` that is not (n,), negative or not finite; that check
    reads the device."""
    n = self.position.shape[0]
    if not isinstance(sigma, torch.Tensor) or tuple(sigma.shape) != (n,):
      raise ValueError(f"sigma must be a ({n},) tensor, got {tuple(getattr(sigma, 'shape', ()))}")
    if not sigma.is_floating_point():
      raise ValueError(f"sigma must be a floating-point tensor, got {sigma.dtype}")
    if not bool((torch.isfinite(sigma) & (sigma >= 0)).all()):
      raise ValueError("sigma must be finite and non-negative")
    sigma = sigma.to(device=self.log_scaling.device, dtype=self.log_scaling.dtype).unsqueeze(1)
    filtered = sigma > 0
    ratio = sigma / torch.exp(self.log_scaling)
    growth = 1 + ratio * ratio                                       # s'^2 / s^2 per axis
    alpha = torch.sigmoid(self.alpha_logit) * torch.rsqrt(growth).prod(dim=1, keepdim=True)
    return self.replace(log_scaling=torch.where(filtered, self.log_scaling + 0.5 * torch.log1p(ratio * ratio), self.log_scaling),
                        alpha_logit=torch.where(filtered, torch.log(alpha) - torch.log1p(-alpha), self.alpha_logit))

  @staticmethod
  def concat_batch(gaussians: List['Gaussians3D']) -> 'Gaussians3D':
    return Gaussians3D.cat(gaussians, dim=0)

  @staticmethod
  def from_point_cloud(points: torch.Tensor, colours: Optional[torch.Tensor] = None, *, sh_degree: Optional[int] = None,
                       k: int = 3, initial_alpha: float = 0.1, min_dist2: float = 1e-7) -> 'Gaussians3D':
    """Initial gaussians of a sparse point cloud, as the upstream trainers build them (no reference counterpart):
    isotropic, scale = sqrt of the mean squared distance to the k nearest other points (``misc.knn.mean_knn_dist2``,
    clamped below by ``min_dist2``), identity rotation (xyzw), alpha = ``initial_alpha``.

    ``colours`` (N, 3) in [0, 1], 0.5 when omitted.  ``sh_degree=None``: feature = colours, (N, 3).  ``sh_degree=D``:
    feature (N, 3, (D + 1)^2) with coefficient 0 = (colours - 0.5) / SH_C0 and the rest zero, the layout
    ``evaluate_sh_at`` and ``render_gaussians(use_sh=True)`` read.  The points must be on the GPU (the neighbour search
    has no CPU fallback) and N >= 2; like ``misc.knn.knn`` this reads the points' bounding box back to the host once.
    """
    if not isinstance(points, torch.Tensor) or points.ndim != 2 or points.shape[1] != 3:
      raise ValueError(f"points must be a (N, 3) tensor, got {tuple(getattr(points, 'shape', ()))}")
    n = points.shape[0]
    if n < 2:
      raise ValueError(f"from_point_cloud needs at least 2 points, got {n}")
    if colours is not None and (not isinstance(colours, torch.Tensor) or colours.shape != (n, 3)):
      raise ValueError(f"colours must be a ({n}, 3) tensor, got {tuple(getattr(colours, 'shape', ()))}")
    if colours is not None and colours.device != points.device:
      raise ValueError(f"colours are on {colours.device}, points on {points.device}")
    if sh_degree is not None and (not isinstance(sh_degree, int) or isinstance(sh_degree, bool) or not 0 <= sh_degree <= 3):
      raise ValueError(f"sh_degree must be None or an integer in 0..3 (the SH kernels' range), got {sh_degree!r}")
    if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= 8:
      raise ValueError(f"k must be an integer in 1..8, got {k!r}")
    if not 0.0 < initial_alpha < 1.0:
      raise ValueError(f"initial_alpha must be inside (0, 1), got {initial_alpha}")
    if not min_dist2 > 0.0:
      raise ValueError(f"min_dist2 must be positive, got {min_dist2}")

    from .misc.knn import mean_knn_dist2     # (imports the kernel library: kept out of the data model's import)
    position = points.detach().to(torch.float32).contiguous()
    dist2 = mean_knn_dist2(position, k)
    log_scale = torch.log(torch.sqrt(torch.clamp_min(dist2, min_dist2)))
    rotation = position.new_zeros((n, 4))
    rotation[:, 3] = 1.0
    alpha_logit = inverse_sigmoid(position.new_full((n, 1), float(initial_alpha)))
    rgb = position.new_full((n, 3), 0.5) if colours is None else colours.detach().to(torch.float32)
    if sh_degree is None:
      feature = rgb.clone()
    else:
      feature = position.new_zeros((n, 3, (sh_degree + 1) ** 2))
      feature[:, :, 0] = (rgb - 0.5) / SH_C0
    return Gaussians3D(position=position, log_scaling=log_scale.unsqueeze(1).repeat(1, 3), rotation=rotation,
                       alpha_logit=alpha_logit, feature=feature, batch_size=(n,))

  @staticmethod
  def load_ply(path, *, device='cpu', sh_degree='file', chunk_rows: int = 1 << 20) -> 'Gaussians3D':
    """A scene from a 3DGS PLY file (``scene_io.load_ply``: field mapping, formats and errors are described there)."""
    from .scene_io import load_ply     # (numpy, file handling: kept out of the data model's import)
    return load_ply(path, device=device, sh_degree=sh_degree, chunk_rows=chunk_rows)

  def save_ply(self, path, *, chunk_rows: int = 1 << 20) -> None:
    """Write the scene as a binary 3DGS PLY file (``scene_io.save_ply``)."""
    from .scene_io import save_ply
    save_ply(self, path, chunk_rows=chunk_rows)

  def compressed(self, sh_codes: int = 4096, iterations: int = 10, weights: Optional[torch.Tensor] = None,
                 seed: Optional[int] = None):
    """The scene with its higher SH bands vector-quantised (``scene_codec.compress_scene``)."""
    from .scene_codec import compress_scene
    return compress_scene(self, sh_codes=sh_codes, iterations=iterations, weights=weights, seed=seed)


def similarity_from_matrix(m) -> Tuple[float, torch.Tensor, torch.Tensor]:
  """``(s, R, t)`` of ``m = [[s R, t], [0, 1]]``, float64 on the CPU, or ``ValueError``: ``m`` must be (4, 4) with last
  row (0, 0, 0, 1), ``s = det(m[:3, :3])^(1/3) > 0`` and ``m[:3, :3] / s`` a proper rotation."""
  from .spherical_harmonics import check_rotation
  if not isinstance(m, torch.Tensor) or m.shape != (4, 4):
    raise ValueError(f"m must be a (4, 4) tensor, got {tuple(getattr(m, 'shape', ()))}")
  m = m.detach().to(device='cpu', dtype=torch.float64)
  if not bool(torch.isfinite(m).all()):
    raise ValueError("m has non-finite entries")
  if m[3].tolist() != [0.0, 0.0, 0.0, 1.0]:
    raise ValueError(f"the last row of m must be (0, 0, 0, 1), got {tuple(m[3].tolist())}")
  why = "a quaternion and an isotropic log_scaling offset cannot represent it"
  det = float(torch.linalg.det(m[:3, :3]))
  if not det > 0:
    raise ValueError(f"m[:3, :3] has determinant {det:.3g}: a reflection or a singular matrix; {why}")
  s = det ** (1.0 / 3.0)
  try:
    r = check_rotation(m[:3, :3] / s, "m[:3, :3] / s")
  except ValueError as e:
    raise ValueError(f"m is not a similarity transform ({e}); {why}") from None
  return s, r, m[:3, 3].clone()


def inverse_sigmoid(x: torch.Tensor):
  return torch.log(x / (1 - x))


class Gaussians2D(TensorClass):
  """2D gaussians used by the 2D harness (reference ``data_types.py:122``)."""
  position: torch.Tensor      # 2  - xy
  depths: torch.Tensor        # 1  - for sorting
  log_scaling: torch.Tensor   # 2
  rotation: torch.Tensor      # 2  - unit length complex number
  alpha_logit: torch.Tensor   # 1  - alpha = sigmoid(alpha_logit)
  feature: torch.Tensor       # N  - (any rgb, label etc)

  @property
  def opacity(self):
    return self.alpha_logit.sigmoid()

  @property
  def scaling(self):
    return torch.exp(self.log_scaling)

  def set_scaling(self, scaling) -> 'Gaussians2D':
    return self.replace(log_scaling=torch.log(scaling))
