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


# ---- the k nearest points of ANOTHER set (``ms_knn_query``, csrc/knn_query.hip) -----------------------------------------

def _check_query(queries: torch.Tensor, points: torch.Tensor, k: int):
  for name, t in (('queries', queries), ('points', points)):
    if not isinstance(t, torch.Tensor) or t.ndim != 2 or t.shape[1] != 3:
      raise ValueError(f"{name} must be a (N, 3) tensor, got {tuple(getattr(t, 'shape', ()))}")
  if not isinstance(k, int) or isinstance(k, bool) or not 1 <= k <= MAX_K:
    raise ValueError(f"k must be an integer in 1..{MAX_K}, got {k!r}")
  if queries.is_cuda and points.is_cuda and queries.device != points.device:
    raise ValueError(f"queries are on {queries.device}, points on {points.device}: one GPU expected")


def _common_bounds(a: torch.Tensor, b: torch.Tensor) -> Tuple[np.ndarray, np.ndarray]:
  """``_bounds`` of two sets at once (either may be empty, not both): still one host read"""
  sets = [t for t in (a, b) if t.shape[0] > 0]
  lower = torch.stack([t.amin(dim=0) for t in sets]).amin(dim=0)
  upper = torch.stack([t.amax(dim=0) for t in sets]).amax(dim=0)
  finite = torch.stack([torch.isfinite(t).all() for t in sets]).all().to(torch.float32).reshape(1)
  row = torch.cat([lower, upper, finite]).cpu().numpy()
  if row[6] != 1.0:
    raise ValueError("queries and points must be finite: found a NaN or infinite coordinate")
  return row[0:3].copy(), row[3:6].copy()


def _sorted_codes(pts: torch.Tensor, lower: np.ndarray, upper: np.ndarray) -> Tuple[torch.Tensor, torch.Tensor]:
  """(sorted Morton codes, their argsort as int32) of ``pts`` on the grid of the box"""
  index = torch.arange(pts.shape[0], dtype=torch.int32, device=pts.device)
  if pts.shape[0] == 0:
    return torch.empty((0,), dtype=torch.int64, device=pts.device), index
  return radix_sort_pairs(_codes_in_box(pts, lower, upper), index, 0, 63)


def query_scratch_bytes(m: int, n: int) -> int:
  """Bytes of scratch ``ms_knn_query`` needs for m points and n queries (host arithmetic, no launch)."""
  lib = _lib.load()
  return _lib.scratch_bytes(lambda tmp, size: lib.ms_knn_query(None, None, m, None, None, None, n, 1, None, None, None,
                                                               tmp, size, None), "knn_query")


def knn_query_into(points: torch.Tensor, point_order: torch.Tensor, queries: torch.Tensor, query_order: torch.Tensor,
                   query_hint: Optional[torch.Tensor], k: int, out_dist2: torch.Tensor, out_index: Optional[torch.Tensor],
                   scratch: torch.Tensor, stats: Optional[torch.Tensor] = None) -> None:
  """The bare C call on the current stream, into buffers the caller owns: no allocation, host read or
  synchronisation, so it can be captured into a graph.  points (M, 3) and queries (N, 3) float32, point_order (M,) and
  query_order (N,) int32, query_hint None or (N,) int32 (the position in ``point_order`` near which the query at
  position i of ``query_order`` starts), out_dist2 (N, k) float32, out_index (N, k) int32 or None, scratch >=
  ``query_scratch_bytes(M, N)`` bytes of uint8, stats None or int64 (2,) to which the search adds
  [blocks scanned x queries, distance evaluations]."""
  _check_query(queries, points, k)
  _lib.require_gpu(points, point_order, queries, query_order, query_hint, out_dist2, out_index, scratch, stats)
  m, n = points.shape[0], queries.shape[0]
  assert points.dtype == torch.float32 and point_order.dtype == torch.int32 and point_order.shape == (m,)
  assert queries.dtype == torch.float32 and query_order.dtype == torch.int32 and query_order.shape == (n,)
  assert query_hint is None or (query_hint.dtype == torch.int32 and query_hint.shape == (n,))
  assert out_dist2.dtype == torch.float32 and out_dist2.shape == (n, k)
  assert out_index is None or (out_index.dtype == torch.int32 and out_index.shape == (n, k))
  assert stats is None or (stats.dtype == torch.int64 and stats.shape == (2,))
  assert scratch.dtype == torch.uint8
  lib, stream = _lib.load(), _lib.current_stream(queries.device)
  _lib.run_in_scratch(lambda tmp, size: lib.ms_knn_query(
    _lib.ptr(points), _lib.ptr(point_order), m, _lib.ptr(queries), _lib.ptr(query_order), _lib.ptr(query_hint), n, k,
    _lib.ptr(out_dist2), _lib.ptr(out_index), _lib.ptr(stats), tmp, size, stream), scratch, "knn_query")


def knn_query(queries: torch.Tensor, points: torch.Tensor, k: int = 1, *,
              return_indices: bool = True) -> Tuple[torch.Tensor, Optional[torch.Tensor]]:
  """The k nearest ``points`` of every query: (dist2 (N, k) float32 ascending, index (N, k) int32 into ``points`` or None).

  Exact, and nothing is excluded: a query that coincides with a point finds it at distance 0.  With fewer than k points
  the missing entries are +inf / -1; an empty set on either side is legal.  The distance is ``knn``'s, so
  ``knn_query(p, p, k + 1)`` is a column of zeros followed by ``knn(p, k)`` bit for bit.

  Both sets are sorted along ONE Z-order curve, that of their common bounding box, and every wave of 64 consecutive
  queries starts at the block of points where ``torch.searchsorted`` puts its middle query's code; neither the orders
  nor that hint change the distances, only the time.  Like ``knn`` this reads the bounding box (and whether every
  coordinate is finite) back to the host once, and raises ValueError on a NaN or infinite coordinate on either side.
  ``knn_query_into`` is the call without that read.
  """
  _check_query(queries, points, k)
  _lib.require_gpu(queries, points)
  qry = queries.detach().to(torch.float32).contiguous()
  pts = points.detach().to(torch.float32).contiguous()
  n, m = qry.shape[0], pts.shape[0]
  dist2 = torch.empty((n, k), dtype=torch.float32, device=qry.device)
  index = torch.empty((n, k), dtype=torch.int32, device=qry.device) if return_indices else None
  if n == 0:
    return dist2, index
  lower, upper = _common_bounds(qry, pts)
  point_codes, point_order = _sorted_codes(pts, lower, upper)
  query_codes, query_order = _sorted_codes(qry, lower, upper)
  hint = torch.searchsorted(point_codes, query_codes).to(torch.int32)
  scratch = _lib.scratch_block(query_scratch_bytes(m, n), qry.device)
  knn_query_into(pts, point_order, qry, query_order, hint, k, dist2, index, scratch)
  return dist2, index


__all__ = ["knn", "mean_knn_dist2", "knn_into", "scratch_bytes", "morton_order", "knn_query", "knn_query_into",
           "query_scratch_bytes", "BLOCK", "MAX_K"]
