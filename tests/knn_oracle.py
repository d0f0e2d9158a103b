"""float64 brute-force oracle of the k-nearest-neighbour search (csrc/knn.hip), the point sets the GPU tests use and the
criterion they share.  Imported by tests/test_knn_host.py (which checks the oracle itself against hand answers) and
tests/test_gpu_knn.py.

Oracle: the float32 coordinates cast to float64, squared distances from coordinate DIFFERENCES (never the expanded
|a|^2 + |b|^2 - 2ab form), rows in chunks, self excluded by index, the k smallest of a row sorted ascending; a missing
neighbour (N - 1 < k) is +inf / -1.  It runs on the device of its input, so the GPU tests keep it on the GPU.

Criterion (``check``).  Distances: |got - want| <= 4 * 2^-24 * want, and exactly 0 where the oracle says 0.  Indices:
distinct within a row, never the row itself, in range, and |p[i] - p[index]|^2 recomputed in float32 with the kernel's
expression ((dx dx + dy dy) + dz dz, every operation rounded once) reproduces the returned distance bitwise: under ties
any valid index passes.  Missing neighbours are +inf / -1, and there are exactly max(0, k - (N - 1)) of them per row.
"""
import math

import numpy as np
import torch

REL_TOL = 4.0 * 2.0 ** -24


def brute_force(points, k, chunk=2048):
  """(dist2 (N, k) float64 ascending, index (N, k) int64) of the k nearest OTHER points of every point"""
  p = points.detach().to(torch.float64)
  n = p.shape[0]
  dist2 = torch.full((n, k), math.inf, dtype=torch.float64, device=p.device)
  index = torch.full((n, k), -1, dtype=torch.int64, device=p.device)
  kk = min(k, n - 1)
  if kk <= 0:
    return dist2, index
  for begin in range(0, n, chunk):
    rows = p[begin:begin + chunk]
    d2 = torch.zeros((rows.shape[0], n), dtype=torch.float64, device=p.device)
    for axis in range(3):
      diff = rows[:, axis:axis + 1] - p[None, :, axis]
      d2 += diff * diff
    own = torch.arange(begin, begin + rows.shape[0], device=p.device)
    d2[torch.arange(rows.shape[0], device=p.device), own] = math.inf      # self, by index
    best, where = torch.topk(d2, kk, dim=1, largest=False, sorted=True)
    dist2[begin:begin + rows.shape[0], :kk] = best
    index[begin:begin + rows.shape[0], :kk] = where
  return dist2, index


# ---- point sets -------------------------------------------------------------------------------------------------------
def _shuffled(points, gen):
  return points[torch.randperm(points.shape[0], generator=gen)].contiguous()


def uniform_cube(n, block, gen):
  return torch.rand((n, 3), generator=gen)


def plane_z0(n, block, gen):
  """every point on z = 0: one Morton axis is degenerate"""
  p = torch.rand((n, 3), generator=gen)
  p[:, 2] = 0.0
  return p


def clusters_and_loner(n, block, gen):
  """two tight clusters far apart and one isolated point whose neighbours all lie in far blocks"""
  half = (n - 1) // 2
  a = 0.01 * torch.randn((half, 3), generator=gen)
  b = 0.01 * torch.randn((n - 1 - half, 3), generator=gen) + torch.tensor([100.0, 0.0, 0.0])
  return _shuffled(torch.cat([a, b, torch.tensor([[50.0, 40.0, 0.0]])]), gen)


def duplicates(n, block, gen):
  """2 block + 5 copies of one point among random ones: whole blocks of coincident points"""
  copies = 2 * block + 5
  p = torch.rand((n, 3), generator=gen)
  p[:copies] = torch.tensor([0.3, 0.6, 0.2])
  return _shuffled(p, gen)


def lattice(n, block, gen):
  """integer lattice: every distance is tied many times over"""
  side = int(math.ceil(n ** (1.0 / 3.0)))
  g = torch.stack(torch.meshgrid(*(torch.arange(side, dtype=torch.float32),) * 3, indexing='ij'), dim=-1).reshape(-1, 3)
  return _shuffled(g, gen)[:n].contiguous()


def offset_cube(n, block, gen):
  """unit cube at 10^4: only the difference form keeps the distances in float32"""
  return torch.rand((n, 3), generator=gen) + 1.0e4


def geometric_line(n, block, gen):
  """points on the x axis, geometrically spaced over 10 decades"""
  p = torch.zeros((n, 3))
  p[:, 0] = torch.pow(10.0, torch.linspace(-5.0, 5.0, n, dtype=torch.float64)).to(torch.float32)
  return _shuffled(p, gen)


DISTRIBUTIONS = {
  'uniform_cube': uniform_cube, 'plane_z0': plane_z0, 'clusters_and_loner': clusters_and_loner, 'duplicates': duplicates,
  'lattice': lattice, 'offset_cube': offset_cube, 'geometric_line': geometric_line,
}


def make(name, n, block, seed=0):
  gen = torch.Generator().manual_seed(seed + sum(map(ord, name)))
  p = DISTRIBUTIONS[name](n, block, gen).to(torch.float32).contiguous()
  assert p.shape == (n, 3)
  return p


# ---- criterion --------------------------------------------------------------------------------------------------------
def kernel_dist2_f32(points, rows, index):
  """|p[row] - p[index]|^2 as csrc/knn.hip evaluates it: float32, (dx dx + dy dy) + dz dz, every operation rounded once"""
  p = np.ascontiguousarray(points, dtype=np.float32)
  d = p[rows] - p[index]
  dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
  return (dx * dx + dy * dy) + dz * dz


def check(points, k, dist2, index, want_dist2, label=""):
  """asserts the criterion of the module docstring; returns the largest |got - want| / want in units of 2^-24"""
  p = points.detach().cpu().numpy()
  n = p.shape[0]
  got = dist2.detach().cpu().numpy()
  want = want_dist2.detach().cpu().numpy()[:, :k]
  assert got.shape == (n, k) and got.dtype == np.float32, (label, got.shape, got.dtype)
  missing = max(0, k - (n - 1))
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
    assert ((idx[finite] >= 0) & (idx[finite] < n)).all(), f"{label}: index out of range"
    assert (idx[finite] != rows[finite]).all(), f"{label}: a point is its own neighbour"
    s = np.sort(np.where(finite, idx, -1 - np.arange(k)[None, :]), axis=1)      # (distinct placeholders for the missing)
    assert (np.diff(s, axis=1) != 0).all(), f"{label}: an index twice in a row"
    again = kernel_dist2_f32(p, rows[finite], idx[finite])
    assert (again.view(np.uint32) == got[finite].view(np.uint32)).all(), f"{label}: index does not reproduce its distance bitwise"
  return worst
