"""Camera-set coverage: which cameras of a set see each gaussian, by how many it is seen, and the nearest depth and the
highest sampling rate ``focal / depth`` at which any of them sees it — one launch (``ms_camera_coverage``,
csrc/camera_coverage.hip) instead of a loop of ``project_to_image`` with a host read, an index tensor and a scatter per
camera.  No reference counterpart.

"In view" is, bit for bit, the decision ``project_to_image`` takes for that camera with the same ``RasterConfig``: the
gaussian's depth lies between the camera's clip planes and the bounding box of its blurred, alpha-thresholded footprint
meets the camera's image.  A gaussian whose opacity is below ``alpha_threshold`` or whose quaternion is zero or not
finite is in view of no camera, as in the renderer.
"""
from __future__ import annotations

from dataclasses import dataclass
import math
import operator
from typing import Optional, Sequence, Union

import torch

from .. import _lib
from ..data_types import Gaussians3D, RasterConfig
from ..perspective.params import CameraParams

CAMERA_VALUES = _lib.COVERAGE_CAMERA_VALUES    # values per packed camera row (MS_COVERAGE_CAMERA_VALUES)
MAX_CAMERAS = _lib.COVERAGE_MAX_CAMERAS


def pack_cameras(cameras: Sequence[CameraParams], dtype: torch.dtype = torch.float32, device=None) -> torch.Tensor:
  """(C, 20) tensor of ``dtype`` on ``device`` (None: the first camera's), the layout ``ms_camera_coverage`` reads.  Per
  camera: rows 0..2 of ``T_camera_world`` row-major (12 values), ``fx, fy, cx, cy``, ``near, far``, ``width, height``.

  The camera tensors are stacked and cast where they live (no ``.item()`` or ``.cpu()`` on them, so packing does not
  wait for the device); clip planes and image sizes are host numbers and travel in one small copy.  Detached.
  Raises ValueError on an empty sequence or more than 65535 cameras."""
  cameras = list(cameras)
  if not 1 <= len(cameras) <= MAX_CAMERAS:
    raise ValueError(f"pack_cameras: between 1 and {MAX_CAMERAS} cameras expected, got {len(cameras)}")
  if device is None:
    device = cameras[0].T_camera_world.device
  pose = torch.stack([c.T_camera_world.detach().to(device=device, dtype=dtype)[:3].reshape(12) for c in cameras])
  projection = torch.stack([c.projection.detach().to(device=device, dtype=dtype) for c in cameras])
  host = torch.tensor([[float(c.near_plane), float(c.far_plane), float(c.image_size[0]), float(c.image_size[1])]
                       for c in cameras], dtype=torch.float64)          # rounded once to dtype, as the C call rounds them
  return torch.cat([pose, projection, host.to(device=device, dtype=dtype)], dim=1).contiguous()


@dataclass
class Coverage:
  """Result of ``camera_coverage`` for n gaussians and ``num_cameras`` cameras.

  count:      (n,) int32, number of cameras that have the gaussian in view
  max_rate:   (n,) maximum over those cameras of ``max(fx, fy) / depth`` (pixels per world unit); 0 where unseen
  min_depth:  (n,) minimum over those cameras of the camera-space depth; +inf where unseen
  mask:       None, or (ceil(C / 32), n) int32 holding the library's uint32 words, word-major: bit ``c % 32`` of
              ``mask[c // 32, i]`` is set exactly when camera ``c`` sees gaussian ``i``; unused high bits are zero
  """
  count: torch.Tensor
  max_rate: torch.Tensor
  min_depth: torch.Tensor
  mask: Optional[torch.Tensor]
  num_cameras: int

  @property
  def seen(self) -> torch.Tensor:
    """(n,) bool: in view of at least one camera"""
    return self.count > 0

  def seen_by(self, c: int) -> torch.Tensor:
    """(n,) bool: in view of camera ``c`` (needs ``masks=True``)"""
    if self.mask is None:
      raise ValueError("seen_by needs the per-camera masks: call camera_coverage(..., masks=True)")
    try:
      index = None if isinstance(c, bool) else operator.index(c)
    except TypeError:
      index = None
    if index is None or not 0 <= index < self.num_cameras:
      raise IndexError(f"camera {c!r} is not an integer in 0..{self.num_cameras - 1}")
    c = index
    return ((self.mask[c // 32] >> (c % 32)) & 1) != 0

  def filter_sigma(self, variance: float = 0.2) -> torch.Tensor:
    """(n,) standard deviation of Mip-Splatting's 3-D smoothing filter for the sampling rate this camera set provides:
    ``sqrt(variance) / max_rate``, and 0 (no filter) where the gaussian is unseen.  ``Gaussians3D.with_filter_3d`` bakes
    it into a scene."""
    if not variance >= 0.0:
      raise ValueError(f"variance must be non-negative, got {variance}")
    rate = self.max_rate
    return torch.where(rate > 0, math.sqrt(variance) / rate, torch.zeros_like(rate))


def _packed(cameras, dtype, device) -> torch.Tensor:
  if isinstance(cameras, torch.Tensor):
    if cameras.ndim != 2 or cameras.shape[1] != CAMERA_VALUES or not 1 <= cameras.shape[0] <= MAX_CAMERAS:
      raise ValueError(f"packed cameras must be a (C, {CAMERA_VALUES}) tensor with 1 <= C <= {MAX_CAMERAS}, "
                       f"got {tuple(cameras.shape)}")
    _lib.require_gpu(cameras)
    return cameras.detach().to(dtype).contiguous()
  cameras = list(cameras)
  _lib.require_gpu(*[t for c in cameras for t in (c.T_camera_world, c.projection)])
  return pack_cameras(cameras, dtype, device)


def camera_coverage(gaussians: Gaussians3D, cameras: Union[Sequence[CameraParams], torch.Tensor],
                    config: RasterConfig = RasterConfig(), *, masks: bool = False) -> Coverage:
  """Coverage of ``gaussians`` by a camera set, one kernel launch (see the module docstring for what "in view" means).

  ``cameras`` is a sequence of ``CameraParams``, each with its own image size and clip planes, or an already packed
  (C, 20) tensor (``pack_cameras``) — the form to use inside a captured graph.  ``blur_cov``, ``clamp_margin`` and
  ``alpha_threshold`` come from ``config``, exactly as in ``project_to_image``.  The inputs are detached and made
  contiguous, the cameras cast to the gaussians' dtype (float32 or float64).  Everything must be on the GPU: there is
  no CPU fallback.  No host synchronisation and no atomics: the outputs are bitwise reproducible.

  ``Coverage.filter_sigma`` turns the result into the input of Mip-Splatting's 3-D smoothing filter.  Two deliberate
  differences from Mip-Splatting's code:

  - Visibility is the renderer's own ``in_view`` — extent-aware (the footprint's bounding box against the image) and
    alpha-aware (a gaussian below the alpha threshold is seen by nobody).  Mip-Splatting tests whether the centre lies
    in a frustum enlarged by 15 %.
  - Gaussians no camera sees get no filter (sigma 0).  Mip-Splatting gives them the filter of the largest observed
    distance.
  """
  tensors = [t.detach().contiguous() for t in gaussians.shape_tensors()]
  _lib.require_gpu(*tensors)
  position = tensors[0]
  device, dtype = position.device, position.dtype
  code = _lib.dtype_code(dtype)
  if not all(t.dtype == dtype for t in tensors):
    raise ValueError("camera_coverage: position, log_scaling, rotation and alpha_logit must share one dtype")
  packed = _packed(cameras, dtype, device)
  if packed.device != device:
    raise ValueError(f"camera_coverage: cameras are on {packed.device}, the gaussians on {device}")
  n, num_cameras = position.shape[0], packed.shape[0]

  count = torch.empty((n,), dtype=torch.int32, device=device)
  max_rate = torch.empty((n,), dtype=dtype, device=device)
  min_depth = torch.empty((n,), dtype=dtype, device=device)
  mask = torch.empty(((num_cameras + 31) // 32, n), dtype=torch.int32, device=device) if masks else None
  _lib.check(_lib.load().ms_camera_coverage(*[t.data_ptr() for t in tensors], packed.data_ptr(), num_cameras,
                                            float(config.blur_cov), float(config.clamp_margin),
                                            float(config.alpha_threshold), n, count.data_ptr(), max_rate.data_ptr(),
                                            min_depth.data_ptr(), _lib.ptr(mask), code, _lib.current_stream(device)),
             "camera_coverage")
  return Coverage(count=count, max_rate=max_rate, min_depth=min_depth, mask=mask, num_cameras=num_cameras)


__all__ = ["camera_coverage", "pack_cameras", "Coverage", "CAMERA_VALUES", "MAX_CAMERAS"]
