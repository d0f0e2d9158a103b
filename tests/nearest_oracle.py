"""float64 brute-force oracle of the cross-set nearest-neighbour search (csrc/knn_query.hip) and the criterion its GPU
tests share: tests/knn_oracle.py without the self clause.  The point sets come from ``knn_oracle.make``.

Oracle (``cross``): the float32 coordinates cast to float64, squared distances from coordinate DIFFERENCES (never the
expanded |a|^2 + |b|^2 - 2ab form), queries in chunks, NOTHING excluded, the k smallest of a row sorted ascending; a
missing neighbour (M < k) is +inf / -1.  It runs on the device of its input.

Criterion (``check_cross``).  Distances: |got - want| <= 4 * 2^-24 * want, and exactly 0 where the oracle says 0; rows
ascending.  Indices: distinct within a row, in range, and |q[i] - p[index]|^2 recomputed in float32 with the kernel's
expression ((dx dx + dy dy) + dz dz, every operation rounded once) reproduces the returned distance bitwise: under ties
any valid index passes.  Missing neighbours are +inf / -1, exactly max(0, k - M) of them per row.
"""
import math

import numpy as np
import torch

REL_TOL = 4.0 * 2.0 ** -24


def cross(queries, points, k, chunk=2048):
  """(dist2 (N, k) float64 ascending, index (N, k) int64) of the k nearest points of every query"""
  q, p = queries.detach().to(torch.float64), points.detach().to(torch.float64)
  n, m = q.shape[0], p.shape[0]
  dist2 = torch.full((n, k), math.inf, dtype=torch.float64, device=q.device)
  index = torch.full((n, k), -1, dtype=torch.int64, device=q.device)
  kk = min(k, m)
  if kk <= 0 or n == 0:
    return dist2, index
  for begin in range(0, n, chunk):
    rows = q[begin:begin + chunk]
    d2 = torch.zeros((rows.shape[0], m), dtype=torch.float64, device=q.device)
    for axis in range(3):
      diff = rows[:, axis:axis + 1] - p[None, :, axis]
      d2 += diff * diff
    best, where = torch.topk(d2, kk, dim=1, largest=False, sorted=True)
    dist2[begin:begin + rows.shape[0], :kk] = best
    index[begin:begin + rows.shape[0], :kk] = where
  return dist2, index


def kernel_dist2_f32(queries, points, rows, index):
  """|q[row] - p[index]|^2 as the kernels evaluate it: float32, (dx dx + dy dy) + dz dz, every operation rounded once"""
  q = np.ascontiguousarray(queries, dtype=np.float32)
  p = np.ascontiguousarray(points, dtype=np.float32)
  d = q[rows] - p[index]
  dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
  return (dx * dx + dy * dy) + dz * dz


def check_cross(queries, points, k, dist2, index, want_dist2, label=""):
  """asserts the criterion of the module docstring; returns the largest |got - want| / want in units of 2^-24"""
  q, p = queries.detach().cpu().numpy(), points.detach().cpu().numpy()
  n, m = q.shape[0], p.shape[0]
  got = dist2.detach().cpu().numpy()
  want = want_dist2.detach().cpu().numpy()[:, :k]
  assert got.shape == (n, k) and got.dtype == np.float32, (label, got.shape, got.dtype)
  missing = max(0, k - m)
  finite = np.isfinite(want)
  assert (finite.sum(axis=1) == k - missing).all(), label
  assert (np.isinf(got) & (got > 0)).sum() == missing * n and (np.isfinite(got) == finite).all(), f"{label}: missing neighbours are not +inf"
  assert (got[:, :-1][finite[:, 1:]] <= got[:, 1:][finite[:, 1:]]).all(), f"{label}: rows are not ascending"
  g, w = got[finite].astype(np.float64), want[finite]
  assert (g[w == 0] == 0).all(), f"{label}: non-zero distance where the oracle says 0"
  err = np.abs(g - w)
  worst = float((err[w > 0] / w[w > 0]).max() / 2.0 ** -24) if (w > 0).any() else 0.0
  assert (err <= REL_TOL * w).all(), f"{label}: largest relative error {worst:.2f} x 2^-24 (allowed 4)"
  if index is not None:
    idx = index.detach().cpu().numpy()
    assert idx.shape == (n, k) and idx.dtype == np.int32, (label, idx.shape, idx.dtype)
    assert ((idx == -1) == ~finite).all(), f"{label}: index -1 exactly where a neighbour is missing"
    rows = np.broadcast_to(np.arange(n)[:, None], (n, k))
    assert ((idx[finite] >= 0) & (idx[finite] < m)).all(), f"{label}: index out of range"
    s = np.sort(np.where(finite, idx, -1 - np.arange(k)[None, :]), axis=1)      # (distinct placeholders for the missing)
    assert (np.diff(s, axis=1) != 0).all(), f"{label}: an index twice in a row"
    again = kernel_dist2_f32(q, p, rows[finite], idx[finite])
    assert (again.view(np.uint32) == got[finite].view(np.uint32)).all(), f"{label}: index does not reproduce its distance bitwise"
  return worst
