"""Splitting gaussians with the kernels of ``csrc/densify.hip``: the child geometry of a densification step.

* ``split_gaussians3d``: children of ``Gaussians3D`` (no counterpart in the reference, whose split helpers are 2-D).
* ``densify_split_gaussians2d`` / ``densify_uniform_split_gaussians2d`` / ``densify_split_gaussians3d``: prune + split a
  ``ParameterClass`` in one fused step (``optim/densify.py``), the children computed as ``split_gaussians2d`` /
  ``uniform_split_gaussians2d`` of ``misc/renderer2d.py`` (reference ``misc/renderer2d.py:60-131``) compute them.

The random numbers are drawn here with torch, in the order the torch functions draw them, and handed to the kernels:
a run stays reproducible under ``torch.manual_seed`` and both paths can be given the same numbers.
"""
from __future__ import annotations

import math
from typing import Dict, Optional, Union

import torch

from .. import _lib
from ..data_types import Gaussians3D
from ..optim.densify import DensifyPlan, densify, plan_densify

Scale = Union[None, float, torch.Tensor]


def _f32(t: Optional[torch.Tensor], shape, name: str) -> Optional[torch.Tensor]:
  if t is None:
    return None
  _lib.require_gpu(t)
  assert tuple(t.shape) == tuple(shape), f"{name}: shape {tuple(shape)} expected, got {tuple(t.shape)}"
  return t.detach().to(torch.float32).contiguous()


def _scale_rows(scale: Scale, parents: int, dims: int, device) -> Optional[torch.Tensor]:
  """Per-parent (parents, dims) scale factors from None, a number or a tensor broadcastable to that shape."""
  if scale is None:
    return None
  if not torch.is_tensor(scale):
    return torch.full((parents, dims), float(scale), dtype=torch.float32, device=device)
  return scale.to(device=device, dtype=torch.float32).expand(parents, dims).contiguous()


def _geometry(tensors: Dict[str, torch.Tensor], dims: int, quat: int):
  out = []
  for name, width in (('position', dims), ('log_scaling', dims), ('rotation', quat)):
    t = tensors[name]
    _lib.require_gpu(t)
    assert t.dtype == torch.float32 and t.is_contiguous() and t.shape[1:] == (width,), \
      f"{name}: contiguous float32 (N, {width}) expected, got {t.dtype} {tuple(t.shape)}"
    out.append(t)
  return out


def split_children2d(tensors: Dict[str, torch.Tensor], first: int, children: int, z: torch.Tensor,
                     scale: Scale = None, depth_offset: Optional[torch.Tensor] = None):
  """In place on rows ``first:`` of ``tensors`` (copies of the parents, ``children`` consecutive rows per parent):
  ``position += point_basis(parent) @ z``, ``log_scaling += log(scale)``, ``depths = max(depths + depth_offset, 1e-6)``
  (``ms_densify_split2d``).  ``z``: (parents, children, 2); ``scale``: number or (parents, 2)."""
  position, log_scaling, rotation = _geometry(tensors, 2, 2)
  count = position.shape[0] - first
  assert count >= 0 and count % children == 0, f"{count} child rows are not a multiple of {children}"
  parents = count // children
  z = _f32(z, (parents, children, 2), 'z')
  scale = _scale_rows(scale, parents, 2, position.device)
  depths = tensors.get('depths')
  if depths is not None:
    assert depths.dtype == torch.float32 and depths.is_contiguous() and depths.numel() == position.shape[0]
  if depth_offset is not None:
    depth_offset = _f32(depth_offset.reshape(-1), (count,), 'depth_offset')
  _lib.check(_lib.load().ms_densify_split2d(position.data_ptr(), log_scaling.data_ptr(), rotation.data_ptr(), _lib.ptr(depths),
                                            first, count, children, z.data_ptr(), _lib.ptr(scale), _lib.ptr(depth_offset),
                                            _lib.current_stream(position.device)), "split2d")


def split_children3d(tensors: Dict[str, torch.Tensor], first: int, children: int, z: torch.Tensor, scale: Scale = None):
  """In place on rows ``first:`` of ``tensors``: ``position += R(q / |q|) (exp(log_scaling) * z)`` (xyzw quaternion),
  ``log_scaling += log(scale)`` (``ms_densify_split3d``).  ``z``: (parents, children, 3); ``scale``: number or (parents, 3)."""
  position, log_scaling, rotation = _geometry(tensors, 3, 4)
  count = position.shape[0] - first
  assert count >= 0 and count % children == 0, f"{count} child rows are not a multiple of {children}"
  parents = count // children
  z = _f32(z, (parents, children, 3), 'z')
  scale = _scale_rows(scale, parents, 3, position.device)
  _lib.check(_lib.load().ms_densify_split3d(position.data_ptr(), log_scaling.data_ptr(), rotation.data_ptr(), first, count,
                                            children, z.data_ptr(), _lib.ptr(scale), _lib.current_stream(position.device)),
             "split3d")


def split_gaussians3d(points: Gaussians3D, n: int = 2, scaling: Scale = None, z: Optional[torch.Tensor] = None) -> Gaussians3D:
  """Replace every gaussian by ``n`` children drawn from it: positions ``R (sigma * z)`` away with ``z`` (N, n, 3)
  (default: half a standard normal, as ``split_gaussians2d``), every axis scaled by ``scaling`` (default 1 / sqrt(n);
  a number or per-parent (N, 3) factors).  Children of one parent are consecutive."""
  _lib.require_gpu(points.position)
  count = points.position.shape[0]
  if z is None:
    z = 0.5 * torch.randn((count, n, 3), device=points.position.device, dtype=torch.float32)
  if scaling is None:
    scaling = 1.0 / math.sqrt(n)
  copies = points.apply(lambda t: torch.repeat_interleave(t.detach(), repeats=n, dim=0).contiguous(), batch_size=[count * n])
  split_children3d({k: getattr(copies, k) for k in ('position', 'log_scaling', 'rotation')}, 0, n, z, scaling)
  return copies


# ---- prune + split of a ParameterClass ----------------------------------------------------------------------------------

def _plan(params, prune_mask, split_mask, n: int, plan: Optional[DensifyPlan]) -> DensifyPlan:
  return plan if plan is not None else plan_densify(prune_mask, split_mask, n)


def densify_split_gaussians3d(params, prune_mask: torch.Tensor, split_mask: torch.Tensor, n: int = 2, scaling: Scale = None,
                              z: Optional[torch.Tensor] = None, plan: Optional[DensifyPlan] = None, **kwargs):
  """``params`` without the pruned rows, every split row replaced by ``n`` children as ``split_gaussians3d`` makes them
  (appended after the kept rows).  ``z``: (n_split, n, 3)."""
  plan = _plan(params, prune_mask, split_mask, n, plan)
  device = params.tensors['position'].device
  if z is None:
    z = 0.5 * torch.randn((plan.n_split, n, 3), device=device, dtype=torch.float32)
  if scaling is None:
    scaling = 1.0 / math.sqrt(n)
  return densify(params, prune_mask, split_mask, n, plan=plan,
                 split_fn=lambda tensors, p: split_children3d(tensors, p.n_kept, n, z, scaling), **kwargs)


def densify_split_gaussians2d(params, prune_mask: torch.Tensor, split_mask: torch.Tensor, n: int = 2,
                              scaling: Optional[float] = None, depth_noise: float = 1e-2,
                              plan: Optional[DensifyPlan] = None, **kwargs):
  """Fused ``params[keep].append_tensors(split_gaussians2d(params[split], n, scaling, depth_noise))``: same random
  draws in the same order (``z``, then the depth noise)."""
  plan = _plan(params, prune_mask, split_mask, n, plan)
  position = params.tensors['position']
  z = 0.5 * torch.randn((plan.n_split, n, 2), device=position.device, dtype=position.dtype)
  if scaling is None:
    scaling = 1.0 / math.sqrt(n)
  depths = params.tensors['depths']
  noise = torch.randn((plan.num_children, *depths.shape[1:]), device=depths.device, dtype=depths.dtype) * depth_noise
  return densify(params, prune_mask, split_mask, n, plan=plan,
                 split_fn=lambda tensors, p: split_children2d(tensors, p.n_kept, n, z, scaling, noise), **kwargs)


def densify_uniform_split_gaussians2d(params, prune_mask: torch.Tensor, split_mask: torch.Tensor, n: int = 2,
                                      scaling: Optional[float] = None, depth_noise: float = 1e-2, sep: float = 0.7,
                                      random_axis: bool = False, eps: float = 1e-6, plan: Optional[DensifyPlan] = None,
                                      **kwargs):
  """Fused ``params[keep].append_tensors(uniform_split_gaussians2d(params[split], ...))``: the axis choice and the depth
  noise are drawn with torch exactly as there (same order, same values under a seed); a step without split rows draws
  nothing."""
  plan = _plan(params, prune_mask, split_mask, n, plan)
  if plan.n_split == 0:
    return densify(params, prune_mask, split_mask, n, plan=plan, **kwargs)
  log_scaling = params.tensors['log_scaling'].detach().index_select(0, plan.parent_rows)
  dtype, device = log_scaling.dtype, log_scaling.device
  if random_axis:
    probs = torch.nn.functional.normalize(torch.exp(log_scaling) + eps, p=1, dim=1)
    axis = torch.multinomial(probs, num_samples=1).squeeze(1)
  else:
    axis = torch.argmax(log_scaling, dim=1)
  onehot = torch.nn.functional.one_hot(axis, num_classes=2).to(dtype)
  steps = torch.linspace(-sep, sep, n, device=device, dtype=dtype)
  z = steps.view(1, n, 1) * onehot.view(-1, 1, 2)
  if scaling is None:
    scaling = math.sqrt(n) / n
  scale = onehot * scaling + (1 - onehot)
  depths = params.tensors['depths']
  noise = torch.randn((plan.num_children, *depths.shape[1:]), device=depths.device, dtype=depths.dtype) * depth_noise
  return densify(params, prune_mask, split_mask, n, plan=plan,
                 split_fn=lambda tensors, p: split_children2d(tensors, p.n_kept, n, z, scale, noise), **kwargs)
