"""Fixed-budget densification on a bare ``Gaussians3D`` and the position noise that goes with it (3DGS-MCMC, Kheradmand
et al. 2024; kernels in ``csrc/relocate.hip``, no reference counterpart).

* ``relocate_gaussians3d``: dead gaussians move onto live ones drawn by opacity, in place (``optim/relocate.py`` does the
  same for a ``ParameterClass`` with its optimiser state).
* ``perturb_positions``: ``position += step * g(o) * Sigma @ z`` after an optimiser step (``ms_perturb_positions``).

Random numbers are drawn here with torch and consumed by the kernels: a run is reproducible under ``torch.manual_seed``.
"""
from __future__ import annotations

import math
from typing import Optional, Union

import torch

from .. import _lib
from ..data_types import Gaussians3D
from ..optim.relocate import RelocateResult, relocate_arrays

GEOMETRY = ('position', 'log_scaling', 'rotation', 'alpha_logit')


def _refuse_grad(tensors, who: str):
  if torch.is_grad_enabled() and any(t.requires_grad for t in tensors):
    raise RuntimeError(f"{who} would overwrite tensors that require grad: call it under torch.no_grad()")


def relocate_gaussians3d(gaussians: Gaussians3D, *, min_opacity: float = 0.005,
                         random: Optional[torch.Tensor] = None) -> RelocateResult:
  """Move the dead gaussians (``sigmoid(alpha_logit) <= min_opacity``, NaN included) onto live ones drawn in proportion
  to their opacity, in place on the five tensors of ``gaussians``; sources and copies get the corrected opacity and
  scale (``optim.relocate``).  Tensors that require grad are refused outside ``torch.no_grad()``.  Nothing is read back
  to the host: ``RelocateResult`` holds device tensors."""
  fields = [gaussians.position, gaussians.log_scaling, gaussians.rotation, gaussians.alpha_logit, gaussians.feature]
  _refuse_grad(fields, "relocate_gaussians3d")
  position, log_scaling, rotation, alpha_logit, feature = (t.detach() for t in fields)
  with torch.no_grad():
    return relocate_arrays(alpha_logit, log_scaling,
                           [(position, _lib.RELOCATE_COPY), (log_scaling, _lib.RELOCATE_SCALE), (rotation, _lib.RELOCATE_COPY),
                            (alpha_logit, _lib.RELOCATE_OPACITY), (feature, _lib.RELOCATE_COPY)],
                           min_opacity=min_opacity, random=random)


def perturb_positions(gaussians_or_params: Union[Gaussians3D, 'ParameterClass'], step: float, z: Optional[torch.Tensor] = None,
                      k: float = 100.0, x0: float = 0.995):
  """``position += step * g(o) * Sigma @ z`` in place, one launch: ``Sigma = R diag(exp(2 log_scaling)) R^T`` with ``R``
  from the xyzw quaternion normalised as in the projection, ``o = sigmoid(alpha_logit)`` and
  ``g(o) = 1 / (1 + exp(-k ((1 - o) - x0)))``: opaque gaussians stay, nearly transparent ones explore.  ``z``: (N, 3)
  float32, default standard normal.  ``step`` is the caller's noise scale (the paper: ``5e5 * lr_position``).

  Takes a ``Gaussians3D`` (tensors that require grad are refused outside ``torch.no_grad()``) or a ``ParameterClass``
  with those four tensors (its parameters are updated as an optimiser updates them).  Returns its argument."""
  for name, value in (('step', step), ('k', k), ('x0', x0)):
    if not math.isfinite(float(value)):
      raise ValueError(f"perturb_positions: finite {name} expected, got {value}")
  if isinstance(gaussians_or_params, Gaussians3D):
    fields = [getattr(gaussians_or_params, name) for name in GEOMETRY]
    _refuse_grad(fields, "perturb_positions")
  else:
    tensors = gaussians_or_params.tensors
    missing = [name for name in GEOMETRY if name not in tensors]
    if missing:
      raise KeyError(f"perturb_positions: no tensor {missing} in {list(tensors)}")
    fields = [tensors[name] for name in GEOMETRY]
  position, log_scaling, rotation, alpha_logit = (t.detach() for t in fields)
  n = position.shape[0]
  if z is not None and (z.dtype != torch.float32 or tuple(z.shape) != (n, 3)):
    raise ValueError(f"perturb_positions: z must be ({n}, 3) float32, got {z.dtype} {tuple(z.shape)}")
  _lib.require_gpu(position, log_scaling, rotation, alpha_logit, z)
  for name, t, width in zip(GEOMETRY, (position, log_scaling, rotation, alpha_logit), (3, 3, 4, 1)):
    if t.dtype != torch.float32:
      raise TypeError(f"perturb_positions: {name} must be float32, got {t.dtype}")
    assert t.is_contiguous() and t.numel() == n * width, f"perturb_positions: contiguous ({n}, {width}) {name} expected"
  if z is None:
    z = torch.randn((n, 3), dtype=torch.float32, device=position.device)
  assert z.is_contiguous() and z.device == position.device, "perturb_positions: contiguous z on the scene's device expected"
  _lib.check(_lib.load().ms_perturb_positions(position.data_ptr(), log_scaling.data_ptr(), rotation.data_ptr(),
                                              alpha_logit.data_ptr(), z.data_ptr(), n, float(step), float(k), float(x0),
                                              _lib.current_stream(position.device)), "perturb positions")
  return gaussians_or_params
