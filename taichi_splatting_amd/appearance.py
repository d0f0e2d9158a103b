"""Per-image appearance compensation: a render is sliced through a small learnable bilateral grid of 3 x 4 affine colour
matrices ("Bilateral guided radiance field processing") before the loss, so that exposure, white balance and tone curve
of each photograph are absorbed by its grid and not baked into the gaussians.  One forward launch and up to three
backward launches of ``csrc/bilagrid.hip`` on the renderer's ``(H, W, 3)`` images.

The reference has no appearance model; this is an addition.  There is no torch fallback: CPU tensors raise, as everywhere
in this package.  Every call runs on the current stream, allocates through torch only and never reads back to the host,
so it captures into ``frame.FrameGraph`` / ``torch.cuda.graph`` with the rest of a training step; the grid gradient is a
gather without atomics and is bitwise reproducible.
"""
from __future__ import annotations

from typing import Tuple, Union

import torch
from torch.autograd.function import once_differentiable

from . import _lib

MAX_L, MAX_G = 16, 128       # BG_MAX_L / BG_MAX_G of csrc/bilagrid.hip


def _checked(image: torch.Tensor, grid: torch.Tensor):
  if image.dim() != 3 or image.shape[2] != 3:
    raise ValueError(f"image must be (H, W, 3) (got {tuple(image.shape)})")
  if grid.dim() != 4 or grid.shape[0] != 12:
    raise ValueError(f"grid must be (12, L, Gy, Gx) (got {tuple(grid.shape)})")
  if image.dtype != grid.dtype or image.device != grid.device:
    raise TypeError(f"image and grid differ in dtype or device ({image.dtype} on {image.device}, {grid.dtype} on {grid.device})")
  _lib.dtype_code(image.dtype)
  h, w, _ = image.shape
  _, l, gy, gx = grid.shape
  if h < 1 or w < 1:
    raise ValueError(f"empty image {tuple(image.shape)}")
  if not (1 <= l <= MAX_L and 1 <= gy <= MAX_G and 1 <= gx <= MAX_G):
    raise ValueError(f"grid (12, L, Gy, Gx) needs 1 <= L <= {MAX_L} and 1 <= Gy, Gx <= {MAX_G} (got {tuple(grid.shape)})")
  if h * w * 3 >= 2 ** 31:
    raise ValueError(f"image too large {tuple(image.shape)}")
  _lib.require_gpu(image, grid)


def bilagrid_forward(image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
  """One ms_bilagrid_fwd launch on contiguous ``(H, W, 3)`` and ``(12, L, Gy, Gx)`` tensors."""
  h, w, _ = image.shape
  _, l, gy, gx = grid.shape
  out = torch.empty_like(image)
  _lib.check(_lib.load().ms_bilagrid_fwd(_lib.ptr(image), _lib.ptr(grid), h, w, l, gy, gx, _lib.dtype_code(image.dtype),
                                         out.data_ptr(), _lib.current_stream(image.device)), "apply_bilateral_grid")
  return out


def bilagrid_backward(image: torch.Tensor, grid: torch.Tensor, grad_out: torch.Tensor, want_image: bool, want_grid: bool):
  """``(dL/dimage | None, dL/dgrid | None)`` of one ms_bilagrid_bwd call: only the wanted gradients are launched."""
  lib = _lib.load()
  h, w, _ = image.shape
  _, l, gy, gx = grid.shape
  dtype, stream = _lib.dtype_code(image.dtype), _lib.current_stream(image.device)
  grad_image = torch.empty_like(image) if want_image else None
  grad_grid = torch.empty_like(grid) if want_grid else None       # written whole by the kernels
  _lib.run_with_scratch(lambda tmp, size: lib.ms_bilagrid_bwd(
    _lib.ptr(image), _lib.ptr(grid), _lib.ptr(grad_out), h, w, l, gy, gx, dtype, _lib.ptr(grad_image), _lib.ptr(grad_grid),
    tmp, size, stream), image.device, "apply_bilateral_grid backward")
  return grad_image, grad_grid


class _ApplyBilateralGrid(torch.autograd.Function):

  @staticmethod
  def forward(ctx, image, grid):
    x, g = image.detach().contiguous(), grid.detach().contiguous()
    ctx.save_for_backward(x, g)
    return bilagrid_forward(x, g)

  @staticmethod
  @once_differentiable
  def backward(ctx, grad_out):
    x, g = ctx.saved_tensors
    want_image, want_grid = ctx.needs_input_grad
    if not (want_image or want_grid):
      return None, None
    return bilagrid_backward(x, g, grad_out.to(dtype=x.dtype).contiguous(), want_image, want_grid)


def apply_bilateral_grid(image: torch.Tensor, grid: torch.Tensor) -> torch.Tensor:
  """``image`` ``(H, W, 3)`` sliced through ``grid`` ``(12, L, Gy, Gx)``: per pixel ``out = A[:, :3] p + A[:, 3]`` with
  ``A`` the trilinear interpolation of the twelve planes at ``((x + 0.5) / W (Gx - 1), (y + 0.5) / H (Gy - 1),
  clamp(luminance, 0, 1) (L - 1))``, which is ``grid_sample(bilinear, border, align_corners=True)`` of the planes; coefficient
  ``4c + j`` is row ``c``, column ``j`` of the 3 x 4 matrix.  Differentiable (once) in both arguments, the luminance
  guide included.  float32 / float64 GPU tensors of one dtype (non-contiguous inputs are copied); ``1 <= L <= 16``,
  ``1 <= Gy, Gx <= 128``; sizes of 1 are legal (``L = Gy = Gx = 1`` is one global affine: exposure and white balance)."""
  _checked(image, grid)
  return _ApplyBilateralGrid.apply(image, grid)


def identity_bilateral_grid(L: int = 8, Gy: int = 16, Gx: int = 16, dtype: torch.dtype = torch.float32,
                            device: Union[str, torch.device, None] = None) -> torch.Tensor:
  """``(12, L, Gy, Gx)`` grid whose every vertex holds the identity affine ``[I | 0]``: ``apply_bilateral_grid`` returns the image."""
  if min(L, Gy, Gx) < 1:
    raise ValueError(f"L, Gy, Gx >= 1 expected (got {L}, {Gy}, {Gx})")
  eye = torch.eye(3, 4, dtype=dtype, device=device).reshape(12, 1, 1, 1)
  return eye.expand(12, L, Gy, Gx).contiguous()


def bilateral_grid_tv(grids: torch.Tensor) -> torch.Tensor:
  """Total-variation regulariser of ``(..., 12, L, Gy, Gx)`` grids: the sum over the three lattice axes of the mean
  squared difference of neighbouring vertices, ``sum_axis mean((delta_axis grids)^2)``; an axis of size 1 contributes 0.
  Plain torch on purpose (the tensor is kilobytes).  Other trainers' versions of this term differ by constant factors
  (per-axis normalisation, a division by the batch), which the weight the user puts on it absorbs."""
  if grids.dim() < 4 or grids.shape[-4] != 12:
    raise ValueError(f"grids must be (..., 12, L, Gy, Gx) (got {tuple(grids.shape)})")
  total = grids.new_zeros(())
  for axis in (-3, -2, -1):
    if grids.shape[axis] > 1:
      total = total + grids.diff(dim=axis).square().mean()
  return total


class BilateralGrids(torch.nn.Module):
  """One bilateral grid per training image: a parameter ``grids`` ``(num_images, 12, L, Gy, Gx)`` initialised to the
  identity affine.  ``grid_shape`` is ``(Gx, Gy, L)``, default 16 x 16 x 8."""

  def __init__(self, num_images: int, grid_shape: Tuple[int, int, int] = (16, 16, 8), dtype: torch.dtype = torch.float32,
               device: Union[str, torch.device, None] = None):
    super().__init__()
    if num_images < 1:
      raise ValueError(f"num_images >= 1 expected (got {num_images})")
    gx, gy, l = (int(v) for v in grid_shape)
    if not (1 <= l <= MAX_L and 1 <= gy <= MAX_G and 1 <= gx <= MAX_G):
      raise ValueError(f"grid_shape (Gx, Gy, L) needs 1 <= Gx, Gy <= {MAX_G} and 1 <= L <= {MAX_L} (got {tuple(grid_shape)})")
    grid = identity_bilateral_grid(l, gy, gx, dtype, device)
    self.grids = torch.nn.Parameter(grid.unsqueeze(0).repeat(num_images, 1, 1, 1, 1))

  def forward(self, image: torch.Tensor, index: Union[int, torch.Tensor]) -> torch.Tensor:
    """``image`` corrected by grid ``index``: an ``int``, or a 0-dim integer DEVICE tensor, selected on the device so that
    a captured training step changes the image by writing the tensor, without a new capture."""
    if isinstance(index, torch.Tensor):
      if index.dim() != 0 or index.dtype.is_floating_point or index.dtype == torch.bool:
        raise TypeError(f"index must be an int or a 0-dim integer tensor (got {index.dtype}, shape {tuple(index.shape)})")
      grid = self.grids.index_select(0, index.reshape(1)).squeeze(0)
    else:
      if not 0 <= int(index) < self.grids.shape[0]:
        raise IndexError(f"image index {index} outside 0..{self.grids.shape[0] - 1}")
      grid = self.grids[int(index)]
    return apply_bilateral_grid(image, grid)

  def tv_loss(self) -> torch.Tensor:
    return bilateral_grid_tv(self.grids)
