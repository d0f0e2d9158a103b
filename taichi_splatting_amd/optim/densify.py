"""Fused densification of a ``ParameterClass``: prune and split the rows of every parameter and every per-point
optimiser state tensor with the kernels of ``csrc/densify.hip`` (``ms_densify_*``).

Replaces ``params[keep].append_tensors(children)`` (reference ``optim/parameter_class.py:215-248`` as used by
``examples/fit_image_gaussians.py:190-231``): a ``nonzero`` and one gather per tensor and per state tensor, one
``torch.cat`` per tensor, two rebuilt optimisers.  Here: plan (flags, one scan, counts) -> ONE host read (the new row
count) -> source table -> ONE move launch for all arrays -> optionally the child geometry, in place.

The destination layout is that of the torch path: ``[kept rows in storage order | children grouped by parent in storage
order, n per parent]`` with ``keep = ~(prune | split)``; a row flagged in both masks is pruned.
"""
from __future__ import annotations

import ctypes
from dataclasses import dataclass
from typing import Callable, Dict, Iterable, List, Optional, Tuple

import torch

from .. import _lib
from .parameter_class import per_point_arrays

_pinned_counts: Dict[torch.device, torch.Tensor] = {}


@dataclass
class DensifyPlan:
  """Where every row of the densified arrays comes from.  ``src_row`` / ``child_slot`` are (n_out,) int32 device tensors
  (source row; 0 .. children - 1 for a child, -1 for a kept row); ``counts`` is the device copy of
  (n_kept, n_split, n_out, n)."""
  n: int
  children: int
  n_kept: int
  n_split: int
  n_out: int
  src_row: torch.Tensor
  child_slot: torch.Tensor
  counts: torch.Tensor

  @property
  def parent_rows(self) -> torch.Tensor:
    """(n_split,) int64 source rows of the split parents in storage order (no host synchronisation)."""
    return self.src_row[self.n_kept::self.children].long()

  @property
  def num_children(self) -> int:
    return self.n_split * self.children


def _mask_bytes(mask: torch.Tensor, n: int, name: str) -> torch.Tensor:
  assert mask.shape == (n,), f"{name}: one flag per point expected, got {tuple(mask.shape)} for {n} points"
  assert mask.dtype in (torch.bool, torch.uint8), f"{name}: bool or uint8 expected, got {mask.dtype}"
  mask = mask.contiguous()
  return mask.view(torch.uint8) if mask.dtype == torch.bool else mask


def plan_densify(prune_mask: torch.Tensor, split_mask: torch.Tensor, children: int = 2) -> DensifyPlan:
  """Destination layout for the two masks; the one host read of the step (the counts) happens here."""
  _lib.require_gpu(prune_mask, split_mask)
  n = prune_mask.shape[0]
  device = prune_mask.device
  prune, split = _mask_bytes(prune_mask, n, 'prune_mask'), _mask_bytes(split_mask, n, 'split_mask')
  lib, stream = _lib.load(), _lib.current_stream(device)

  scan = torch.empty((2 * n + 1,), dtype=torch.int32, device=device)
  counts = torch.empty((4,), dtype=torch.int32, device=device)
  if device not in _pinned_counts:
    _pinned_counts[device] = torch.zeros((4,), dtype=torch.int32).pin_memory()
  host = _pinned_counts[device]
  _lib.run_with_scratch(lambda tmp, size: lib.ms_densify_plan(
    prune.data_ptr(), split.data_ptr(), n, int(children), scan.data_ptr(), counts.data_ptr(), host.data_ptr(), tmp, size,
    stream), device, "densify plan")
  torch.cuda.current_stream(device).synchronize()
  n_kept, n_split, n_out, n_seen = (int(x) for x in host.tolist())
  assert n_seen == n and n_out == n_kept + n_split * children, "densify plan: inconsistent counts"

  src_row = torch.empty((n_out,), dtype=torch.int32, device=device)
  child_slot = torch.empty((n_out,), dtype=torch.int32, device=device)
  _lib.check(lib.ms_densify_table(scan.data_ptr(), n, int(children), n_out, src_row.data_ptr(), child_slot.data_ptr(), stream),
             "densify table")
  return DensifyPlan(n=n, children=int(children), n_kept=n_kept, n_split=n_split, n_out=n_out, src_row=src_row,
                     child_slot=child_slot, counts=counts)


def move_rows(plan: DensifyPlan, arrays: List[Tuple[torch.Tensor, bool]]) -> List[torch.Tensor]:
  """One launch (``ms_densify_move``) for every ``(tensor, children_copy_parent)``: returns the new tensors, (n_out, ...)
  each.  Children that do not copy their parent are zero."""
  if not arrays:
    return []
  device = plan.src_row.device
  sources, outputs = [], []
  descriptors = (_lib.DensifyArrayC * len(arrays))()
  for d, (t, copy_parent) in zip(descriptors, arrays):
    _lib.require_gpu(t)
    assert t.shape[0] == plan.n and t.device == device, f"expected {plan.n} rows on {device}, got {tuple(t.shape)} on {t.device}"
    src = t.detach().contiguous()
    out = torch.empty((plan.n_out, *t.shape[1:]), dtype=t.dtype, device=device)
    sources.append(src)
    outputs.append(out)
    d.struct_size = ctypes.sizeof(_lib.DensifyArrayC)
    d.child_fill = int(bool(copy_parent))
    d.src, d.dst = src.data_ptr(), out.data_ptr()
    d.row_bytes = _lib.row_bytes(src, plan.n)
  _lib.check(_lib.load().ms_densify_move(descriptors, len(arrays), plan.src_row.data_ptr(), plan.child_slot.data_ptr(),
                                         plan.n, plan.n_out, _lib.current_stream(device)), "densify move")
  return outputs


def _densify_torch(params, prune_mask, split_mask, children: int, child_tensors, inherit_state):
  """The torch formulation (CPU tensors): ``params[keep].append_tensors(...)`` with parent copies as children."""
  prune_mask, split_mask = prune_mask.bool(), split_mask.bool()
  split_only = split_mask & ~prune_mask
  keep = ~(prune_mask | split_mask)
  repeat = lambda t: torch.repeat_interleave(t.detach()[split_only], children, dim=0)
  if int(keep.sum()) + int(split_only.sum()) == 0:
    raise ValueError("densify: no rows left (every point pruned)")
  tensors = {k: (child_tensors[k] if child_tensors and k in child_tensors else repeat(t)) for k, t in params.tensors.items()}
  state = {k: {s: (repeat(v) if s in inherit_state else torch.zeros_like(repeat(v))) for s, v in st.items()}
           for k, st in params.tensor_state.items()}
  if not bool(keep.any()):       # every row split: ParameterClass refuses the empty intermediate params[keep]
    return params._rebuild(tensors, state)
  return params[keep].append_tensors(tensors, state)


def densify(params, prune_mask: torch.Tensor, split_mask: torch.Tensor, children: int = 2,
            child_tensors: Optional[Dict[str, torch.Tensor]] = None,
            split_fn: Optional[Callable[[Dict[str, torch.Tensor], DensifyPlan], None]] = None,
            inherit_state: Iterable[str] = (), plan: Optional[DensifyPlan] = None):
  """New ``ParameterClass`` equal to ``params[~(prune | split)].append_tensors(children_of_the_split_rows)``: same keys,
  parameter groups and options, non-tensor optimiser state carried over, every per-point state tensor moved with its
  rows and zero for the children (state keys listed in ``inherit_state``, e.g. ``'running_vis'``, copy the parent).

  Each split row gets ``children`` children, which start as copies of their parent.  ``child_tensors`` (name ->
  (n_split * children, ...)) replaces the children of the named tensors; ``split_fn(tensors, plan)`` may then edit
  the child rows ``tensors[k][plan.n_kept:]`` in place (``misc/densify.py`` has the 2-D and 3-D geometry kernels).
  ``plan``: a ``plan_densify`` result for these masks, if the caller needed its counts before (random draws).

  CPU tensors take the torch path (``params[keep].append_tensors``); ``split_fn`` needs the GPU."""
  first = next(iter(params.tensors.values()))
  n = first.shape[0]
  inherit_state = set(inherit_state)
  if not first.is_cuda:
    assert split_fn is None, "densify: the split kernels run on the GPU only; pass child_tensors for CPU tensors"
    return _densify_torch(params, prune_mask, split_mask, int(children), child_tensors, inherit_state)

  if plan is None:
    plan = plan_densify(prune_mask, split_mask, children)
  assert plan.n == n and plan.children == int(children), "densify: the plan was made for other masks"
  if plan.n_out == 0:
    raise ValueError("densify: no rows left (every point pruned)")

  names, state_keys, arrays = per_point_arrays(params)
  copy_parent = [True] * len(names) + [key in inherit_state for _, key in state_keys]
  moved = move_rows(plan, list(zip(arrays, copy_parent)))

  tensors = dict(zip(names, moved[:len(names)]))
  new_state: Dict[str, Dict[str, torch.Tensor]] = {name: {} for name in params.tensor_state}
  for (name, key), t in zip(state_keys, moved[len(names):]):
    new_state[name][key] = t

  if child_tensors:
    for name, value in child_tensors.items():
      assert name in tensors, f"child tensor {name} not in {names}"
      assert value.shape == tensors[name][plan.n_kept:].shape, \
        f"child tensor {name}: {tuple(tensors[name][plan.n_kept:].shape)} expected, got {tuple(value.shape)}"
      tensors[name][plan.n_kept:] = value.to(tensors[name].device)
  if split_fn is not None and plan.num_children > 0:
    split_fn(tensors, plan)
  return params._rebuild(tensors, new_state)
