"""Fixed-budget densification of a ``ParameterClass``: move the dead rows onto live gaussians, in place, with the
kernels of ``csrc/relocate.hip`` (``ms_relocate_*``).  The strategy of 3DGS-MCMC (Kheradmand et al., "3D Gaussian
Splatting as Markov Chain Monte Carlo", NeurIPS 2024); no reference counterpart.

Unlike ``densify`` the row count never changes: no tensor is replaced, no optimiser is rebuilt and nothing is read back
to the host, so a captured graph, a ``frame.ShapeRecord`` and the remembered overlap capacity all stay valid.  A caller
who wants the scene to grow allocates spare rows with a very negative ``alpha_logit``: they are dead, the projection
culls them, and relocation populates them.

Launch sequence: weights -> ``torch.cumsum`` (int64: exact, so the draw is bitwise reproducible whatever order the scan
adds in) -> draw -> fresh opacity and scale of the drawn rows -> ONE move launch over every tensor and state tensor.
The random words are drawn here with torch and consumed by the kernels: reproducible under ``torch.manual_seed``.
"""
from __future__ import annotations

import ctypes
import math
from dataclasses import dataclass
from typing import Dict, Iterable, List, Optional, Tuple

import torch

from .. import _lib
from .parameter_class import per_point_arrays

_binomials: Dict[torch.device, torch.Tensor] = {}


@dataclass
class RelocateResult:
  """What a relocation did, as device tensors (reading them is the caller's synchronisation, not this module's).
  ``src`` (N,) int32: the row each row was filled from, ``src[i] == i`` for a row that did not move; ``count`` (N,)
  int32: how many dead rows landed on each live row; ``weights`` (N,) int64: the integer sampling weights, 0 for a dead
  row; ``counts`` (3,) int64: (dead rows, live rows that were drawn, total weight)."""
  src: torch.Tensor
  count: torch.Tensor
  weights: torch.Tensor
  counts: torch.Tensor


def logit_threshold(min_opacity: float) -> float:
  """``float32(logit(min_opacity))`` evaluated in float64: a row is dead iff ``not (alpha_logit > threshold)``."""
  min_opacity = float(min_opacity)
  if not (0.0 < min_opacity < 1.0 - 1e-7):
    raise ValueError(f"relocate: 0 < min_opacity < 1 - 1e-7 expected, got {min_opacity}")
  return ctypes.c_float(math.log(min_opacity / (1.0 - min_opacity))).value


def binomial_table() -> List[List[float]]:
  """``[m][k] = C(m, k)`` for m, k < 51 (0 above the diagonal); every entry is below 2^53, so exact in float64."""
  n = _lib.RELOCATE_MAX_RATIO
  return [[float(math.comb(m, k)) for k in range(n)] for m in range(n)]


def _device_binomials(device: torch.device) -> torch.Tensor:
  """The table on the device, uploaded once per device (so call once before capturing a graph, as for any torch op)."""
  if device not in _binomials:
    _binomials[device] = torch.tensor(binomial_table(), dtype=torch.float64).to(device).contiguous()
  return _binomials[device]


def _random_words(random: Optional[torch.Tensor], n: int, device) -> torch.Tensor:
  if random is None:
    info = torch.iinfo(torch.int64)
    # randint's upper end is exclusive: the one word 2^63 - 1 (of 2^64) is never drawn
    return torch.randint(info.min, info.max, (n,), dtype=torch.int64, device=device)
  assert random.is_contiguous() and random.device == device, f"relocate: contiguous random words on {device} expected"
  return random


def _check_random(random: Optional[torch.Tensor], n: int):
  if random is not None and (random.dtype != torch.int64 or tuple(random.shape) != (n,)):
    raise ValueError(f"relocate: random must be an ({n},) int64 tensor (read as unsigned 64-bit words), "
                     f"got {random.dtype} {tuple(random.shape)}")


def relocate_arrays(alpha_logit: torch.Tensor, log_scaling: torch.Tensor, arrays: List[Tuple[torch.Tensor, int]], *,
                    min_opacity: float = 0.005, random: Optional[torch.Tensor] = None) -> RelocateResult:
  """The launch sequence on bare tensors.  ``arrays``: ``(tensor, role)`` with ``role`` one of ``_lib.RELOCATE_*``;
  ``alpha_logit`` and ``log_scaling`` themselves must be in it with the OPACITY and SCALE roles to be updated.  Every
  tensor is contiguous with N rows and modified in place."""
  threshold = logit_threshold(min_opacity)
  n = alpha_logit.shape[0]
  _check_random(random, n)
  _lib.require_gpu(alpha_logit, log_scaling, random, *(t for t, _ in arrays))
  device = alpha_logit.device
  for name, t in (('opacity', alpha_logit), ('scale', log_scaling)):
    if t.dtype != torch.float32:
      raise TypeError(f"relocate: the {name} tensor must be float32, got {t.dtype}")
    assert t.is_contiguous() and t.shape[0] == n and t.device == device, f"relocate: contiguous ({n}, ...) {name} expected"
  assert alpha_logit.numel() == n, f"relocate: one opacity logit per point expected, got {tuple(alpha_logit.shape)}"
  dims = log_scaling.numel() // max(n, 1)
  random = _random_words(random, n, device)

  lib, stream = _lib.load(), _lib.current_stream(device)
  binomials = _device_binomials(device)
  weights = torch.empty((n,), dtype=torch.int64, device=device)
  src = torch.empty((n,), dtype=torch.int32, device=device)
  count = torch.empty((n,), dtype=torch.int32, device=device)
  counts = torch.empty((3,), dtype=torch.int64, device=device)
  fresh_opacity = torch.empty((n,), dtype=torch.float32, device=device)
  fresh_scale = torch.empty((n, dims), dtype=torch.float32, device=device)

  descriptors = (_lib.RelocateArrayC * len(arrays))()
  for d, (t, role) in zip(descriptors, arrays):
    assert t.shape[0] == n and t.device == device, f"relocate: expected {n} rows on {device}, got {tuple(t.shape)} on {t.device}"
    assert t.is_contiguous(), "relocate works in place: every tensor must be contiguous"
    d.struct_size = ctypes.sizeof(_lib.RelocateArrayC)
    d.role = int(role)
    d.data = t.data_ptr()
    d.row_bytes = _lib.row_bytes(t, n)
    if role in (_lib.RELOCATE_OPACITY, _lib.RELOCATE_SCALE):
      fresh = fresh_opacity if role == _lib.RELOCATE_OPACITY else fresh_scale
      assert t.dtype == torch.float32 and t.numel() == fresh.numel(), "relocate: opacity / scale role on a tensor of another shape"
      d.fresh = fresh.data_ptr()

  _lib.check(lib.ms_relocate_weights(alpha_logit.data_ptr(), n, threshold, weights.data_ptr(), count.data_ptr(),
                                     counts.data_ptr(), stream), "relocate weights")
  cdf = torch.cumsum(weights, 0)
  _lib.check(lib.ms_relocate_draw(weights.data_ptr(), cdf.data_ptr(), random.data_ptr(), n, src.data_ptr(), count.data_ptr(),
                                  counts.data_ptr(), stream), "relocate draw")
  _lib.check(lib.ms_relocate_fresh(alpha_logit.data_ptr(), log_scaling.data_ptr(), dims, count.data_ptr(), n,
                                   float(min_opacity), binomials.data_ptr(), fresh_opacity.data_ptr(), fresh_scale.data_ptr(),
                                   counts.data_ptr(), stream), "relocate fresh")
  _lib.check(lib.ms_relocate_move(descriptors, len(arrays), src.data_ptr(), count.data_ptr(), n, stream), "relocate move")
  return RelocateResult(src=src, count=count, weights=weights, counts=counts)


def relocate(params, *, min_opacity: float = 0.005, random: Optional[torch.Tensor] = None,
             inherit_state: Iterable[str] = (), opacity: str = 'alpha_logit', scale: str = 'log_scaling') -> RelocateResult:
  """Move every dead row of ``params`` (opacity ``sigmoid(params[opacity]) <= min_opacity``, NaN included) onto a live
  row drawn in proportion to its opacity, in place on the tensors and on every per-point optimiser state tensor:

  * a dead row takes its source's row in every tensor; source and copies get the corrected opacity
    ``1 - (1 - o)^(1 / ratio)`` (``ratio`` = copies + 1, at most 51) and the scale factor of the paper's equation 9;
  * optimiser state of the dead rows and of the drawn live rows becomes zero; state keys in ``inherit_state`` (e.g.
    ``'running_vis'``) follow the gaussian instead: a dead row copies its source, a drawn row keeps its own;
  * with every row dead nothing moves (not an error).

  ``random``: (N,) int64 read as unsigned words, default ``torch.randint`` over the int64 range.  Storage, optimiser and
  row count stay as they are and nothing is read back to the host: the call can be captured into a graph (after one
  call outside a capture, which uploads the binomial table).  Gradients (``.grad``) are not touched."""
  for key in (opacity, scale):
    if key not in params.tensors:
      raise KeyError(f"relocate: no tensor {key!r} in {list(params.tensors.keys())}")
  logit_threshold(min_opacity)
  inherit_state = set(inherit_state)
  _check_random(random, next(iter(params.tensors.values())).shape[0])
  _lib.require_gpu(*params.tensors.values())

  names, state_keys, tensors = per_point_arrays(params)
  roles = [_lib.RELOCATE_OPACITY if name == opacity else _lib.RELOCATE_SCALE if name == scale else _lib.RELOCATE_COPY
           for name in names]
  roles += [_lib.RELOCATE_INHERIT if key in inherit_state else _lib.RELOCATE_ZERO_TOUCHED for _, key in state_keys]
  with torch.no_grad():
    arrays = [(t.detach(), role) for t, role in zip(tensors, roles)]
    return relocate_arrays(params.tensors[opacity].detach(), params.tensors[scale].detach(), arrays,
                           min_opacity=min_opacity, random=random)
