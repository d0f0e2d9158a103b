"""Exact k nearest neighbours of a 3D point set (``ms_knn_points``, csrc/knn.hip): what a trainer needs to turn a
sparse point cloud into initial gaussian scales.  Upstream this is the CUDA-only ``simple_knn.distCUDA2``; the reference
package has no counterpart.

The search runs over the points in Morton order (``ms_morton_codes64`` + ``ms_radix_sort_pairs``): runs of ``BLOCK``
consecutive points are the blocks whose bounding boxes prune it.  The order decides the speed only: squared distances
are ``(dx dx + dy dy) + dz dz`` on float32 differences, unfused, so the k smallest of a point are the same bits under
any ``order`` (under ties the indices may differ).
"""
from __future__ import annotations

import ctypes
from typing import Optional, Tuple

import numpy as np
import torch

from .. import _lib
from ..cuda_lib import radix_sort_pairs

BLOCK = _lib.KNN_BLOCK      # sorted points per block (MS_KNN_BLOCK)
MAX_K = 8
MORTON_CELLS = 2 ** 21      # cells on the longest axis of the bounding box: the full 21 bits per axis of the codes


def _check_points(points: torch.Tensor, k: int):
  if not isinstance(points, torch.Tensor) or points.ndim != 2 or points.shape[1] != 3:
    raise ValueError(f"points must be a (N, 3) tensor, got {tuple(getattr(points, 'shape', ()))}")
  if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
    raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")


def _bounds(pts: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
  """(lower (3,), upper (3,)) of finite points: the one host read of this module; raises on a non-finite coordinate."""
  row = torch.cat([pts.amin(dim=0), pts.amax(dim=0), torch.isfinite(pts).all().to(torch.float32).reshape(1)]).cpu().numpy()
  if row[6] != 1.0:
    raise ValueError("points must be finite: found a NaN or infinite coordinate")
  return row[0:3].copy(), row[3:6].copy()


def _codes_in_box(pts: torch.Tensor, lower: np.ndarray, upper: np.ndarray) -> torch.Tensor:
  """int64 Morton codes on ``MORTON_CELLS`` cubic cells per axis, sized by the longest axis of the box"""
  longest = np.float32((upper - lower).max())
  inc = np.float32(longest / np.float32(MORTON_CELLS))
  if not (inc > 0 and np.isfinite(inc)):      # all points coincide (or the extent underflows): any positive cell will do
    inc = np.float32(1.0)
  lower = lower.astype(np.float32)
  inc3 = np.full((3,), inc, dtype=np.float32)
  n = pts.shape[0]
  codes = torch.empty((n,), dtype=torch.int64, device=pts.device)
  _lib.check(_lib.load().ms_morton_codes64(_lib.ptr(pts), n, lower.ctypes.data_as(ctypes.c_void_p),
                                           inc3.ctypes.data_as(ctypes.c_void_p), MORTON_CELLS, _lib.ptr(codes),
                                           _lib.current_stream(pts.device)), "knn: morton codes")
  return codes


def _order_in_box(pts: torch.Tensor, lower: np.ndarray, upper: np.ndarray) -> torch.Tensor:
  codes = _codes_in_box(pts, lower, upper)
  index = torch.arange(pts.shape[0], dtype=torch.int32, device=pts.device)
  return radix_sort_pairs(codes, index, 0, 63)[1]


def morton_order(points: torch.Tensor) -> torch.Tensor:
  """int32 (N,) argsort of the points along the Z-order curve of their bounding box (``MORTON_CELLS`` cubic cells on
  the longest axis; an axis of zero extent simply stays in cell 0).  Reads the bounding box back to the host."""
  _check_points(points, 1)
  _lib.require_gpu(points)
  pts = points.detach().to(torch.float32).contiguous()
  if pts.shape[0] == 0:
    return torch.empty((0,), dtype=torch.int32, device=pts.device)
  return _order_in_box(pts, *_bounds(pts))


def scratch_bytes(n: int) -> int:
  """Bytes of scratch ``ms_knn_points`` needs for n points (host arithmetic, no launch)."""
  lib = _lib.load()
  return _lib.scratch_bytes(lambda tmp, size: lib.ms_knn_points(None, None, n, 1, None, None, None, tmp, size, None), "knn")


def knn_into(points: torch.Tensor, order: torch.Tensor, k: int, out_dist2: torch.Tensor, out_index: Optional[torch.Tensor],
             scratch: torch.Tensor, stats: Optional[torch.Tensor] = None) -> None:
  """The bare C call on the current stream, into buffers the caller owns: no allocation, host read or
  synchronisation, so it can be captured into a graph.  points (N, 3) float32, order (N,) int32, out_dist2 (N, k)
  float32, out_index (N, k) int32 or None, scratch >= ``scratch_bytes(N)`` bytes of uint8, stats None or int64 (2,) to
  which the search adds [blocks scanned x queries, distance evaluations]."""
  _check_points(points, k)
  _lib.require_gpu(points, order, out_dist2, out_index, scratch, stats)
  n = points.shape[0]
  assert points.dtype == torch.float32 and order.dtype == torch.int32 and order.shape == (n,)
  assert out_dist2.dtype == torch.float32 and out_dist2.shape == (n, k)
  assert out_index is None or (out_index.dtype == torch.int32 and out_index.shape == (n, k))
  assert stats is None or (stats.dtype == torch.int64 and stats.shape == (2,))
  assert scratch.dtype == torch.uint8
  lib, stream = _lib.load(), _lib.current_stream(points.device)
  _lib.run_in_scratch(lambda tmp, size: lib.ms_knn_points(
    _lib.ptr(points), _lib.ptr(order), n, k, _lib.ptr(out_dist2), _lib.ptr(out_index), _lib.ptr(stats), tmp, size, stream),
    scratch, "knn")


def knn(points: torch.Tensor, k: int = 3, *, order: Optional[torch.Tensor] = None,
        return_indices: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
  """The k nearest OTHER points of every point: (dist2 (N, k) float32 ascending, index (N, k) int32 or None).

  Exact.  Self is excluded by index, so a duplicate of a point is its neighbour at distance 0; with fewer than k other
  points the missing entries are +inf / -1.  ``order`` is a permutation of 0..N-1 in which neighbours in space are
  neighbours in the sequence; None computes the Morton order of the points in their bounding box.  The distances do
  not depend on ``order``, only the time does.

  This is an initialisation operator, not a per-frame one: it reads the bounding box (and whether every coordinate is
  finite) back to the host once, and raises ValueError on a NaN or infinite coordinate.  ``knn_into`` is the call
  without that read.
  """
  _check_points(points, k)
  _lib.require_gpu(points, order)
  pts = points.detach().to(torch.float32).contiguous()
  n = pts.shape[0]
  dist2 = torch.empty((n, k), dtype=torch.float32, device=pts.device)
  index = torch.empty((n, k), dtype=torch.int32, device=pts.device) if return_indices else None
  if n == 0:
    return dist2, index
  lower, upper = _bounds(pts)
  if order is None:
    order = _order_in_box(pts, lower, upper)
  else:
    if order.shape != (n,) or order.dtype not in (torch.int32, torch.int64):
      raise ValueError(f"order must be an int32 or int64 permutation of shape ({n},), got {order.dtype} {tuple(order.shape)}")
    order = order.to(torch.int32).contiguous()
  scratch = torch.empty((max(scratch_bytes(n), 1),), dtype=torch.uint8, device=pts.device)
  knn_into(pts, order, k, dist2, index, scratch)
  return dist2, index


def mean_knn_dist2(points: torch.Tensor, k: int = 3) -> torch.Tensor:
  """(N,) float32 mean squared distance to the k nearest other points (the mean of the finite entries of a row when
  N - 1 < k): upstream's ``distCUDA2`` for k = 3."""
  _check_points(points, k)
  if points.shape[0] < 2:
    raise ValueError(f"mean_knn_dist2 needs at least 2 points, got {points.shape[0]}")
  dist2, _ = knn(points, k, return_indices=False)
  finite = torch.isfinite(dist2)
  return torch.where(finite, dist2, torch.zeros_like(dist2)).sum(dim=1) / finite.sum(dim=1).to(torch.float32)


__all__ = ["knn", "mean_knn_dist2", "knn_into", "scratch_bytes", "morton_order", "BLOCK", "MAX_K"]
