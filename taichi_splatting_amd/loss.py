"""Photometric loss of a gaussian-splatting trainer, ``(1 - w) L1 + w (1 - SSIM)``, on the renderer's ``(H, W, C)``
images: one fused forward launch (+ a tiny fixed-order reduction) and one backward launch of ``csrc/loss.hip``.

The reference has no loss; this is an addition.  SSIM is the usual one of 3-D gaussian splatting: 11 x 11 gaussian
window, sigma 1.5, ``C1 = 0.01^2``, ``C2 = 0.03^2``, per channel, ``padding='same'`` zero-padded like
``conv2d(padding=5)`` or ``'valid'``.  There is no torch fallback: CPU tensors raise, as everywhere in this package.
Every call runs on the current stream, allocates through torch only and never reads back to the host, so it captures
into ``frame.FrameGraph`` / ``torch.cuda.graph`` with the rest of a training step.
"""
from __future__ import annotations


import torch
from torch.autograd.function import once_differentiable

from . import _lib

PADDING = dict(same=_lib.PAD_SAME, valid=_lib.PAD_VALID)
WINDOW = 11


def _checked(image: torch.Tensor, target: torch.Tensor, ssim_weight: float, padding: str):
  _lib.require_gpu(image, target)
  if padding not in PADDING:
    raise ValueError(f"padding must be 'same' or 'valid' (got {padding!r})")
  if image.dim() != 3 or image.shape != target.shape:
    raise ValueError(f"image and target must be (H, W, C) of one shape (got {tuple(image.shape)} and {tuple(target.shape)})")
  if image.dtype != target.dtype or image.device != target.device:
    raise TypeError(f"image and target differ in dtype or device ({image.dtype} on {image.device}, {target.dtype} on {target.device})")
  _lib.dtype_code(image.dtype)
  h, w, c = image.shape
  if not 1 <= c <= 4:
    raise ValueError(f"1 to 4 channels expected (got {c})")
  if h < 1 or w < 1:
    raise ValueError(f"empty image {tuple(image.shape)}")
  if padding == 'valid' and min(h, w) < WINDOW:
    raise ValueError(f"padding='valid' needs H, W >= {WINDOW} (got {h} x {w})")
  if not 0.0 <= float(ssim_weight) <= 1.0:
    raise ValueError(f"0 <= ssim_weight <= 1 expected (got {ssim_weight})")
  if target.requires_grad:
    raise ValueError("l1_ssim_loss has no gradient for target: detach it")


def photometric_forward(x: torch.Tensor, y: torch.Tensor, ssim_weight: float, padding: str, want_maps: bool):
  """One ms_photometric_fwd launch on contiguous (H, W, C) tensors: ``(out, maps)`` with ``out`` = (loss, l1, ssim) and
  ``maps`` the (3, Hm, Wm, C) partial maps A, B, C the backward reads (None unless ``want_maps``)."""
  lib = _lib.load()
  h, w, c = x.shape
  dtype, pad = _lib.dtype_code(x.dtype), PADDING[padding]
  stream = _lib.current_stream(x.device)
  out = torch.empty((3,), dtype=x.dtype, device=x.device)
  maps, pointers = None, (None, None, None)
  if want_maps:
    margin = 0 if padding == 'same' else WINDOW // 2
    maps = torch.empty((3, h - 2 * margin, w - 2 * margin, c), dtype=x.dtype, device=x.device)
    pointers = tuple(maps[k].data_ptr() for k in range(3))
  _lib.run_with_scratch(lambda tmp, size: lib.ms_photometric_fwd(
    _lib.ptr(x), _lib.ptr(y), h, w, c, dtype, pad, ssim_weight, *pointers, tmp, size, out.data_ptr(), stream),
    x.device, "l1_ssim_loss")
  return out, maps


def photometric_backward(x: torch.Tensor, y: torch.Tensor, maps: torch.Tensor, grad_loss: torch.Tensor,
                         ssim_weight: float, padding: str) -> torch.Tensor:
  """dloss/dimage (H, W, C) from the forward's maps; ``grad_loss`` is a one-element DEVICE tensor (read by the kernel)."""
  h, w, c = x.shape
  grad = torch.empty_like(x)
  _lib.check(_lib.load().ms_photometric_bwd(_lib.ptr(x), _lib.ptr(y), maps[0].data_ptr(), maps[1].data_ptr(),
                                            maps[2].data_ptr(), _lib.ptr(grad_loss), h, w, c, _lib.dtype_code(x.dtype),
                                            PADDING[padding], ssim_weight, grad.data_ptr(),
                                            _lib.current_stream(x.device)), "l1_ssim_loss backward")
  return grad


def _wants_grad(image: torch.Tensor) -> bool:
  """the partial maps are written only when a backward can follow (inside ``forward`` grad mode is always off)"""
  return image.requires_grad and torch.is_grad_enabled()


class _PhotometricLoss(torch.autograd.Function):
  """(loss, l1, ssim) of one forward launch.  One output is differentiable, and only in ``image``: ``loss``, or, with
  ``ssim_output`` (weight 1, where loss = 1 - ssim), the ``ssim`` term itself, whose gradient is minus the loss's."""

  @staticmethod
  def forward(ctx, image, target, ssim_weight, padding, want_grad, ssim_output):
    x, y = image.detach().contiguous(), target.detach().contiguous()
    out, maps = photometric_forward(x, y, ssim_weight, padding, want_maps=want_grad)
    if maps is not None:
      ctx.save_for_backward(x, y, maps)
    ctx.args = (ssim_weight, padding)
    ctx.ssim_output = ssim_output
    loss, l1, ssim_term = out[0], out[1], out[2]
    ctx.mark_non_differentiable(l1, ssim_term if not ssim_output else loss)
    return loss, l1, ssim_term

  @staticmethod
  @once_differentiable
  def backward(ctx, grad_loss, _grad_l1, grad_ssim):
    x, y, maps = ctx.saved_tensors
    go = -grad_ssim if ctx.ssim_output else grad_loss
    go = go.to(dtype=x.dtype).contiguous()                     # stays on the device: the kernel reads it through a pointer
    return photometric_backward(x, y, maps, go, *ctx.args), None, None, None, None, None


def l1_ssim_loss(image: torch.Tensor, target: torch.Tensor, ssim_weight: float = 0.2, padding: str = 'same',
                 return_terms: bool = False):
  """``(1 - ssim_weight) mean|image - target| + ssim_weight (1 - mean SSIM)`` as a 0-dim tensor, differentiable (once)
  in ``image``.  ``image``, ``target``: ``(H, W, C)`` float32 / float64 GPU tensors, ``C`` from 1 to 4 (non-contiguous
  inputs are copied).  ``return_terms``: ``(loss, l1, ssim)`` with the two detached terms of the same launch."""
  _checked(image, target, ssim_weight, padding)
  loss, l1, ssim_term = _PhotometricLoss.apply(image, target, float(ssim_weight), padding, _wants_grad(image), False)
  return (loss, l1, ssim_term) if return_terms else loss


def ssim(image: torch.Tensor, target: torch.Tensor, padding: str = 'same') -> torch.Tensor:
  """Mean SSIM of two ``(H, W, C)`` images as a 0-dim tensor, differentiable (once) in ``image``: the ssim term of the
  launch itself, the same value whether or not a gradient is wanted."""
  _checked(image, target, 1.0, padding)
  return _PhotometricLoss.apply(image, target, 1.0, padding, _wants_grad(image), True)[2]
