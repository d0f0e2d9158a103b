"""k-means over the rows of a (N, D) float32 matrix (``ms_kmeans_assign`` / ``ms_kmeans_update``, csrc/kmeans.hip): the
codebook builder behind ``scene_codec.compress_scene``.  The reference package has no counterpart.

Assignment scores every (point, code) pair on the exact f32-input MFMA, ``s(i, j) = ||c_j||^2 - 2 x_i . c_j``, and keeps
the arg-min in registers; the lowest index wins a tie.  The update is a float64 mean in an order fixed by the
assignment, so a Lloyd run is bitwise reproducible.  1 <= D <= ``MAX_D``, 1 <= K <= ``MAX_K``.
"""
from __future__ import annotations

from typing import NamedTuple, Optional, Tuple

import torch

from .. import _lib

MAX_D = _lib.KMEANS_MAX_D
MAX_K = _lib.KMEANS_MAX_K


class KMeansResult(NamedTuple):
  codebook: torch.Tensor    # (K, D) float32
  index: torch.Tensor       # (N,) int32: the assignment under `codebook`
  dist2: torch.Tensor       # (N,) float32 squared distance to the assigned code
  counts: torch.Tensor      # (K,) int32 members per code under `index`


def _check_matrix(x, name: str, d: Optional[int] = None):
  if not isinstance(x, torch.Tensor) or x.ndim != 2:
    raise ValueError(f"{name} must be a 2D tensor, got {tuple(getattr(x, 'shape', ()))}")
  if x.dtype != torch.float32:
    raise ValueError(f"{name} must be float32, got {x.dtype}")
  if d is None and not 1 <= x.shape[1] <= MAX_D:
    raise ValueError(f"{name} must have between 1 and {MAX_D} columns, got {x.shape[1]}")
  if d is not None and x.shape[1] != d:
    raise ValueError(f"{name} must have {d} columns like x, got {x.shape[1]}")


def _check_codebook(codebook, d: int):
  _check_matrix(codebook, "codebook", d)
  if not 1 <= codebook.shape[0] <= MAX_K:
    raise ValueError(f"codebook must have between 1 and {MAX_K} rows, got {codebook.shape[0]}")


def _check_vector(v, name: str, n: int, dtype: torch.dtype):
  if not isinstance(v, torch.Tensor) or tuple(v.shape) != (n,):
    raise ValueError(f"{name} must be a ({n},) tensor, got {tuple(getattr(v, 'shape', ()))}")
  if v.dtype != dtype:
    raise ValueError(f"{name} must be {dtype}, got {v.dtype}")


def _check_scratch(scratch, need: int):
  if not isinstance(scratch, torch.Tensor) or scratch.dtype != torch.uint8 or scratch.ndim != 1:
    raise ValueError("scratch must be a 1D uint8 tensor")
  if scratch.numel() < need:
    raise ValueError(f"scratch holds {scratch.numel()} bytes, {need} needed")


def _check_contiguous(**tensors):
  for name, t in tensors.items():
    if t is not None and not t.is_contiguous():
      raise ValueError(f"{name} must be contiguous")


def _check_sizes(n: int, d: int, k: int):
  if n < 0 or not 1 <= d <= MAX_D or not 1 <= k <= MAX_K:
    raise ValueError(f"n >= 0, 1 <= d <= {MAX_D} and 1 <= k <= {MAX_K} expected, got n={n}, d={d}, k={k}")


def assign_scratch_bytes(n: int, d: int, k: int) -> int:
  """Bytes of scratch ``kmeans_assign_into`` needs (host arithmetic, no launch): the staged codebook and its norms."""
  _check_sizes(n, d, k)
  lib = _lib.load()
  return _lib.scratch_bytes(lambda tmp, size: lib.ms_kmeans_assign(None, n, d, None, k, None, None, tmp, size, None),
                            "kmeans_assign")


def update_scratch_bytes(n: int, d: int, k: int) -> int:
  """Bytes of scratch ``kmeans_update_into`` needs (host arithmetic, no launch): the sorted pairs and chunk sums."""
  _check_sizes(n, d, k)
  lib = _lib.load()
  return _lib.scratch_bytes(
    lambda tmp, size: lib.ms_kmeans_update(None, None, None, n, d, k, None, None, None, tmp, size, None), "kmeans_update")


def kmeans_assign_into(x: torch.Tensor, codebook: torch.Tensor, out_index: torch.Tensor, out_dist2: Optional[torch.Tensor],
                       scratch: torch.Tensor) -> None:
  """The bare C call on the current stream into buffers the caller owns: no allocation, host read or synchronisation,
  so it can be captured into a graph.  x (N, D) and codebook (K, D) float32, finite (not checked here); out_index (N,)
  int32; out_dist2 (N,) float32 or None; scratch >= ``assign_scratch_bytes(N, D, K)`` bytes of uint8."""
  _check_matrix(x, "x")
  n, d = x.shape
  _check_codebook(codebook, d)
  k = codebook.shape[0]
  _check_vector(out_index, "out_index", n, torch.int32)
  if out_dist2 is not None:
    _check_vector(out_dist2, "out_dist2", n, torch.float32)
  _lib.require_gpu(x, codebook, out_index, out_dist2, scratch)
  _check_scratch(scratch, assign_scratch_bytes(n, d, k))
  _check_contiguous(x=x, codebook=codebook, out_index=out_index, out_dist2=out_dist2)
  lib, stream = _lib.load(), _lib.current_stream(x.device)
  _lib.run_in_scratch(lambda tmp, size: lib.ms_kmeans_assign(
    _lib.ptr(x), n, d, _lib.ptr(codebook), k, _lib.ptr(out_index), _lib.ptr(out_dist2), tmp, size, stream),
    scratch, "kmeans_assign")


def kmeans_update_into(x: torch.Tensor, index: torch.Tensor, codebook: torch.Tensor, out_counts: torch.Tensor,
                       scratch: torch.Tensor, weights: Optional[torch.Tensor] = None,
                       out_weight_sums: Optional[torch.Tensor] = None) -> None:
  """The bare C call on the current stream: ``codebook`` (K, D) is updated IN PLACE to the weighted means of its
  members; a code with no member or zero weight keeps its row.  index (N,) int32 in 0..K-1, weights None or (N,)
  float32 >= 0 (not checked here), out_counts (K,) int32, out_weight_sums None or (K,) float64, scratch >=
  ``update_scratch_bytes(N, D, K)`` bytes of uint8.  No allocation or host read: graph-capturable."""
  _check_matrix(x, "x")
  n, d = x.shape
  _check_codebook(codebook, d)
  k = codebook.shape[0]
  _check_vector(index, "index", n, torch.int32)
  _check_vector(out_counts, "out_counts", k, torch.int32)
  if weights is not None:
    _check_vector(weights, "weights", n, torch.float32)
  if out_weight_sums is not None:
    _check_vector(out_weight_sums, "out_weight_sums", k, torch.float64)
  _lib.require_gpu(x, index, codebook, out_counts, scratch, weights, out_weight_sums)
  _check_scratch(scratch, update_scratch_bytes(n, d, k))
  _check_contiguous(x=x, index=index, codebook=codebook, out_counts=out_counts, weights=weights, out_weight_sums=out_weight_sums)
  lib, stream = _lib.load(), _lib.current_stream(x.device)
  _lib.run_in_scratch(lambda tmp, size: lib.ms_kmeans_update(
    _lib.ptr(x), _lib.ptr(index), _lib.ptr(weights), n, d, k, _lib.ptr(codebook), _lib.ptr(out_counts),
    _lib.ptr(out_weight_sums), tmp, size, stream), scratch, "kmeans_update")


def kmeans_assign(x: torch.Tensor, codebook: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor]:
  """(index (N,) int32, dist2 (N,) float32): the nearest code of every row of x, lowest index on ties.  Inputs must be
  finite; this call does not read them back to check (``kmeans`` does)."""
  _check_matrix(x, "x")
  _check_codebook(codebook, x.shape[1])
  _lib.require_gpu(x, codebook)
  x, codebook = x.detach().contiguous(), codebook.detach().contiguous()
  n, d = x.shape
  index = torch.empty((n,), dtype=torch.int32, device=x.device)
  dist2 = torch.empty((n,), dtype=torch.float32, device=x.device)
  kmeans_assign_into(x, codebook, index, dist2, _lib.scratch_block(assign_scratch_bytes(n, d, codebook.shape[0]), x.device))
  return index, dist2


def kmeans_update(x: torch.Tensor, index: torch.Tensor, codebook: torch.Tensor,
                  weights: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
  """(new codebook (K, D) float32, counts (K,) int32): the weighted means of the rows assigned to each code; a code with
  no member or zero total weight keeps its row of ``codebook``.  ``codebook`` itself is not modified."""
  _check_matrix(x, "x")
  n, d = x.shape
  _check_codebook(codebook, d)
  _check_vector(index, "index", n, torch.int32)
  if weights is not None:
    _check_vector(weights, "weights", n, torch.float32)
  _lib.require_gpu(x, index, codebook, weights)
  k = codebook.shape[0]
  new = codebook.detach().clone().contiguous()
  counts = torch.empty((k,), dtype=torch.int32, device=x.device)
  kmeans_update_into(x.detach().contiguous(), index.contiguous(), new, counts,
                     _lib.scratch_block(update_scratch_bytes(n, d, k), x.device),
                     None if weights is None else weights.detach().contiguous())
  return new, counts


def kmeans(x: torch.Tensor, k: int, iterations: int = 10, weights: Optional[torch.Tensor] = None,
           seed: Optional[int] = None) -> KMeansResult:
  """Lloyd's algorithm: ``iterations`` rounds of assign + update, then a final assign so that ``index`` and ``dist2``
  belong to the returned codebook.  The initial codes are the rows of x at the first k entries of ``torch.randperm(N)``
  (k distinct rows) under torch's generator of x's device, or under a local generator seeded with ``seed``.  Empty
  clusters keep their centroid; nothing is re-seeded.

  One host read up front (x finite, weights finite and >= 0, else ValueError); none inside the loop.  With the same
  ``seed`` two runs return the same bits."""
  _check_matrix(x, "x")
  n, d = x.shape
  if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
    raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")
  if k > n:
    raise ValueError(f"k = {k} codes need at least as many points, got {n}")
  if not isinstance(iterations, int) or isinstance(iterations, bool) or iterations < 0:
    raise ValueError(f"iterations must be a non-negative integer, got {iterations!r}")
  if weights is not None:
    _check_vector(weights, "weights", n, torch.float32)
  x = x.detach().contiguous()
  ok = torch.isfinite(x).all()
  if weights is not None:
    weights = weights.detach().contiguous()
    ok = ok & (torch.isfinite(weights) & (weights >= 0)).all().to(ok.device)
  if not bool(ok):
    raise ValueError("x must be finite, weights finite and non-negative")
  _lib.require_gpu(x, weights)

  generator = None
  if seed is not None:
    generator = torch.Generator(device=x.device)
    generator.manual_seed(int(seed))
  first = torch.randperm(n, generator=generator, device=x.device)[:k]
  codebook = x.index_select(0, first).contiguous()

  index = torch.empty((n,), dtype=torch.int32, device=x.device)
  dist2 = torch.empty((n,), dtype=torch.float32, device=x.device)
  counts = torch.zeros((k,), dtype=torch.int32, device=x.device)
  assign_scratch = _lib.scratch_block(assign_scratch_bytes(n, d, k), x.device)
  update_scratch = _lib.scratch_block(update_scratch_bytes(n, d, k), x.device)
  for _ in range(iterations):
    kmeans_assign_into(x, codebook, index, None, assign_scratch)
    kmeans_update_into(x, index, codebook, counts, update_scratch, weights)
  kmeans_assign_into(x, codebook, index, dist2, assign_scratch)
  counts = torch.bincount(index.long(), minlength=k).to(torch.int32)       # of the final assignment, not of the last update
  return KMeansResult(codebook, index, dist2, counts)


__all__ = ["kmeans", "kmeans_assign", "kmeans_update", "kmeans_assign_into", "kmeans_update_into", "KMeansResult",
           "assign_scratch_bytes", "update_scratch_bytes", "MAX_D", "MAX_K"]
