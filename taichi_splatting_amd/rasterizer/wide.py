"""Wide-feature rasteriser: ``(N, F)`` float32 features with ``1 <= F <= 128`` blended in ONE pass over the tile lists
(csrc/raster_wide.hip, contractions on the f32-input MFMA), where ``rasterize_with_tiles`` renders wide features four
channels at a time.  No reference counterpart; the semantics are those of ``rasterize_with_tiles`` with
``use_alpha_blending=True, antialias=False`` at tile size 16.

``rasterize_wide`` is the operator on given tile lists; ``render_features`` blends per-gaussian features with the tile
lists and weights of a ``render_gaussians`` frame, so that a feature image costs no second projection or mapping and
its geometry gradient flows into the frame's one backward pass.
"""
from __future__ import annotations

from numbers import Integral
from typing import Tuple

import torch

from .. import _lib
from ..data_types import RasterConfig
from .function import RasterOut

MAX_WIDE_FEATURES = 128      # MS_RASTER_WIDE_MAX_F
WIDE_TILE_SIZE = 16


def check_wide_arguments(gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size, config: RasterConfig):
  """The configurations the wide kernels serve; raises before anything is launched."""
  for name, t in (('gaussians2d', gaussians2d), ('features', features), ('overlap_to_point', overlap_to_point),
                  ('tile_overlap_ranges', tile_overlap_ranges)):
    if not t.is_cuda:
      raise ValueError(f"rasterize_wide: {name} is on {t.device}; the wide rasteriser runs on the GPU only "
                       "(there is no CPU fallback)")
  if gaussians2d.ndim != 2 or gaussians2d.shape[1] != 7:
    raise ValueError(f"rasterize_wide: gaussians2d must be (N, 7), got {tuple(gaussians2d.shape)}")
  if features.ndim != 2 or features.shape[0] != gaussians2d.shape[0]:
    raise ValueError(f"rasterize_wide: features must be (N, F), got {tuple(features.shape)} for "
                     f"{gaussians2d.shape[0]} gaussians")
  f = features.shape[1]
  if not 1 <= f <= MAX_WIDE_FEATURES:
    raise ValueError(f"rasterize_wide: {f} feature channels, supported are 1..{MAX_WIDE_FEATURES} "
                     "(render wider features in slices of 128 channels)")
  if gaussians2d.dtype != torch.float32 or features.dtype != torch.float32:
    raise NotImplementedError(f"rasterize_wide: float32 only (got {gaussians2d.dtype} / {features.dtype}); "
                              "rasterize_with_tiles renders float64")
  if config.tile_size != WIDE_TILE_SIZE:
    raise NotImplementedError(f"rasterize_wide: tile_size {config.tile_size} is not supported, only {WIDE_TILE_SIZE}")
  if config.antialias:
    raise NotImplementedError("rasterize_wide: antialias is not supported (rasterize_with_tiles has it)")
  if not config.use_alpha_blending:
    raise NotImplementedError("rasterize_wide: use_alpha_blending=False (quantile render) is not supported")
  if overlap_to_point.dtype != torch.int32 or tile_overlap_ranges.dtype != torch.int32:
    raise ValueError("rasterize_wide: overlap_to_point and tile_overlap_ranges must be int32")
  w, h = int(image_size[0]), int(image_size[1])
  if w <= 0 or h <= 0:
    raise ValueError(f"rasterize_wide: bad image size {w}x{h}")
  tiles = ((w + WIDE_TILE_SIZE - 1) // WIDE_TILE_SIZE) * ((h + WIDE_TILE_SIZE - 1) // WIDE_TILE_SIZE)
  if tile_overlap_ranges.numel() != 2 * tiles:
    raise ValueError(f"rasterize_wide: tile_overlap_ranges has {tile_overlap_ranges.numel() // 2} tiles, image {w}x{h} "
                     f"with tile_size {WIDE_TILE_SIZE} needs {tiles}")


def _or_placeholder(t: torch.Tensor, dtype) -> torch.Tensor:
  """An empty array has no address to hand to the kernels; with every tile range empty nothing reads this one"""
  return t if t.numel() > 0 else torch.zeros((8,), dtype=dtype, device=t.device)


class _WideRasterFunction(torch.autograd.Function):

  @staticmethod
  def forward(ctx, gaussians, features, overlap_to_point, tile_overlap_ranges, image_size, config):
    check_wide_arguments(gaussians, features, overlap_to_point, tile_overlap_ranges, image_size, config)
    lib = _lib.load()
    gaussians_c = gaussians.detach().contiguous()
    features_c = features.detach().contiguous()
    o2p = overlap_to_point.contiguous()
    ranges = tile_overlap_ranges.contiguous().view(-1, 2)
    w, h = int(image_size[0]), int(image_size[1])
    device = gaussians.device
    f = features_c.shape[1]

    image = torch.empty((h, w, f), dtype=torch.float32, device=device)
    alpha = torch.empty((h, w), dtype=torch.float32, device=device)
    _lib.check(lib.ms_raster_wide_fwd(_or_placeholder(gaussians_c, torch.float32).data_ptr(),
                                      _or_placeholder(features_c, torch.float32).data_ptr(), ranges.data_ptr(),
                                      _or_placeholder(o2p, torch.int32).data_ptr(), w, h, f, _lib.raster_config_c(config),
                                      image.data_ptr(), alpha.data_ptr(), _lib.current_stream(device)),
               "rasterize_wide forward")

    point_heuristic = torch.empty((0, 2), dtype=torch.float32, device=device)
    visibility = torch.empty((0,), dtype=torch.float32, device=device)
    ctx.set_materialize_grads(False)
    ctx.overlap_to_point, ctx.tile_overlap_ranges = o2p, ranges
    ctx.config, ctx.size = config, (w, h)
    ctx.mark_non_differentiable(alpha, point_heuristic, visibility)
    ctx.save_for_backward(gaussians_c, features_c, image)
    return image, alpha, point_heuristic, visibility

  @staticmethod
  def backward(ctx, grad_image, grad_alpha, grad_point_heuristic, grad_visibility):
    gaussians, features, image = ctx.saved_tensors
    need_points, need_features = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    if grad_image is None or not (need_points or need_features):
      return None, None, None, None, None, None
    grad_gaussians = torch.zeros_like(gaussians) if need_points else None
    grad_features = torch.zeros_like(features) if need_features else None
    w, h = ctx.size
    if gaussians.shape[0] > 0 and ctx.overlap_to_point.numel() > 0:
      grad_image = grad_image.contiguous()
      _lib.check(_lib.load().ms_raster_wide_bwd(
        gaussians.data_ptr(), features.data_ptr(), ctx.tile_overlap_ranges.data_ptr(), ctx.overlap_to_point.data_ptr(),
        image.data_ptr(), grad_image.data_ptr(), w, h, features.shape[1], _lib.raster_config_c(ctx.config),
        _lib.ptr(grad_gaussians), _lib.ptr(grad_features), _lib.current_stream(gaussians.device)),
        "rasterize_wide backward")
    return grad_gaussians, grad_features, None, None, None, None


def rasterize_wide(gaussians2d: torch.Tensor, features: torch.Tensor, overlap_to_point: torch.Tensor,
                   tile_overlap_ranges: torch.Tensor, image_size: Tuple[Integral, Integral],
                   config: RasterConfig) -> RasterOut:
  """``rasterize_with_tiles`` for wide features in one pass: float32, ``1 <= F <= 128``, tile size 16, plain pdf, alpha
  blending.

  Parameters are those of ``rasterize_with_tiles`` (no tile-row window).  Returns RasterOut(image (H, W, F),
  image_weight (H, W), point_heuristic (0, 2), visibility (0,)): the wide pass computes neither heuristics nor
  visibility, whatever ``config`` asks for — the colour render of the same frame has them.  Differentiable w.r.t.
  gaussians2d and features; an input that does not require a gradient costs none (without ``gaussians2d`` the
  geometry part of the backward pass is skipped).  The forward is bitwise reproducible, the gradients are summed with
  float atomics.  float64, other tile sizes, antialias and the quantile render raise NotImplementedError, more than
  128 channels or CPU tensors ValueError.
  """
  image, image_weight, point_heuristic, visibility = _WideRasterFunction.apply(
    gaussians2d, features, overlap_to_point, tile_overlap_ranges, image_size, config)
  return RasterOut(image, image_weight, point_heuristic, visibility)


def render_features(rendering, features: torch.Tensor) -> torch.Tensor:
  """The ``(H, W, F)`` image of per-gaussian ``features`` (N, F) — one row per INPUT gaussian of the
  ``render_gaussians`` call that produced ``rendering`` — blended with the colour image's own tile lists and weights:
  no second projection, no second mapping.  The geometry gradient of the feature image enters the frame's backward
  pass with the colour image's, so one ``backward()`` of ``colour_loss + feature_loss`` runs the frame backward once and
  reaches position, log_scaling, rotation, alpha_logit and the camera.  Settles the frame first (one host wait in
  eager mode, as the median-depth pass)."""
  state = getattr(rendering, 'frame', None)
  points7 = getattr(rendering, 'frame_points7', None)
  if state is None or points7 is None:
    raise ValueError("render_features: this rendering does not come from the frame executor; blend the features with "
                     "rasterize_wide on the tile lists of map_to_tiles instead")
  window = state.window
  if window is None or not window.whole or window.cropped:
    raise NotImplementedError("render_features: a rendering of a tile-row strip (tile_rows) is not supported")
  if features.ndim != 2 or features.shape[0] != points7.shape[0]:
    raise ValueError(f"render_features: features must be (N, F) with one row per input gaussian (N = {points7.shape[0]}), "
                     f"got {tuple(features.shape)}")
  state.settle()
  if state.capacity == 0 or state.keep_k is None:
    o2p = torch.empty((0,), dtype=torch.int32, device=points7.device)
  else:
    o2p = state.overlap_to_point()
  return rasterize_wide(points7, features, o2p, state.tile_ranges().view(-1, 2), (window.w, window.h),
                        rendering.config).image
