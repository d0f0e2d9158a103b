"""float64 oracle of misc/kmeans.py (numpy): exact distances, the arg-min with the lowest index on ties, the weighted
update, a Lloyd loop, and the per-pair error bound of the kernel's float32 score.

The kernel evaluates s(i, j) = ||c_j||^2 - 2 x_i . c_j as a float32 fma chain: it starts at ||c_j||^2 (a float64 sum
rounded once) and adds (-2 x_ik) c_jk for k = 0..D-1.  That is D + 1 roundings, each relative u = 2^-24 of a partial sum
no larger than S = ||c_j||^2 + 2 sum_k |x_ik c_jk|, so |s_f32 - s| <= gamma_{D+1} S.  ``score_bound`` is

  b(i, j) = 2 (D + 2) u (||c_j||^2 + 2 sum_k |x_ik c_jk|)

a factor 2 of slack over gamma_{D+1}; ``emulate_scores`` repeats the chain in float32 so that a CPU test can hold the
bound to it (tests/test_kmeans_host.py).
"""
import numpy as np

U = 2.0 ** -24


def _f64(a):
  return np.asarray(a, dtype=np.float64)


def dist2_matrix(x, codebook):
  """(N, K) float64 squared distances, as a sum of squared differences (exact for small integers)"""
  x, c = _f64(x), _f64(codebook)
  out = np.empty((x.shape[0], c.shape[0]))
  step = max(1, (1 << 22) // max(1, c.shape[0] * x.shape[1]))
  for i in range(0, x.shape[0], step):
    diff = x[i:i + step, None, :] - c[None, :, :]
    out[i:i + step] = (diff * diff).sum(axis=2)
  return out


def assign(x, codebook):
  """(index (N,) int32 with the lowest index on ties, dist2 (N,) float64)"""
  d = dist2_matrix(x, codebook)
  index = np.argmin(d, axis=1)                   # numpy: the first occurrence of the minimum
  return index.astype(np.int32), d[np.arange(d.shape[0]), index]


def dist2_to(x, codebook, index):
  """(N,) float64 squared distance of every row to the code its index names"""
  diff = _f64(x) - _f64(codebook)[np.asarray(index, dtype=np.int64)]
  return (diff * diff).sum(axis=1)


def score_bound(x, codebook, index):
  """b(i, index_i) of the module docstring, (N,) float64"""
  x, c = _f64(x), _f64(codebook)[np.asarray(index, dtype=np.int64)]
  d = x.shape[1]
  return 2.0 * (d + 2) * U * ((c * c).sum(axis=1) + 2.0 * np.abs(x * c).sum(axis=1))


def score_bound_matrix(x, codebook):
  """b(i, j) for every pair, (N, K) float64"""
  x, c = _f64(x), _f64(codebook)
  d = x.shape[1]
  return 2.0 * (d + 2) * U * ((c * c).sum(axis=1)[None, :] + 2.0 * (np.abs(x) @ np.abs(c).T))


def exact_scores(x, codebook):
  x, c = _f64(x), _f64(codebook)
  return (c * c).sum(axis=1)[None, :] - 2.0 * (x @ c.T)


def emulate_scores(x, codebook):
  """The kernel's chain in float32: acc = f32(||c||^2); acc = fma(-2 x_k, c_k, acc) for k in order.  The fma is a
  float64 multiply-add (the product of two float32 is exact in float64) rounded to float32: it can differ from a true
  fma by a double rounding, 2^-29 of an ulp, which the bound's slack dwarfs."""
  x32, c32 = np.asarray(x, dtype=np.float32), np.asarray(codebook, dtype=np.float32)
  acc = (_f64(c32) ** 2).sum(axis=1).astype(np.float32)[None, :].repeat(x32.shape[0], axis=0)
  for k in range(x32.shape[1]):
    a = _f64(np.float32(-2.0) * x32[:, k])[:, None]
    acc = (a * _f64(c32[:, k])[None, :] + _f64(acc)).astype(np.float32)
  return acc


def update(x, index, codebook, weights=None):
  """(new codebook (K, D) float32, counts (K,) int32, weight sums (K,) float64): weighted means in float64 rounded once;
  a code with no member or zero weight keeps its row."""
  x, old = _f64(x), np.asarray(codebook, dtype=np.float32)
  index = np.asarray(index, dtype=np.int64)
  k, d = old.shape
  w = np.ones(x.shape[0]) if weights is None else _f64(weights)
  counts = np.bincount(index, minlength=k).astype(np.int32)
  wsum = np.bincount(index, weights=w, minlength=k)
  sums = np.stack([np.bincount(index, weights=w * x[:, j], minlength=k) for j in range(d)], axis=1)
  live = (counts > 0) & (wsum > 0)
  new = old.copy()
  new[live] = (sums[live] / wsum[live, None]).astype(np.float32)
  return new, counts, wsum


def objective(x, codebook, index, weights=None):
  d = dist2_to(x, codebook, index)
  return float(d.sum() if weights is None else (d * _f64(weights)).sum())


def lloyd(x, codebook, iterations, weights=None):
  """(codebook, index, dist2): `iterations` rounds of assign + update from `codebook`, then a final assign"""
  codebook = np.asarray(codebook, dtype=np.float32).copy()
  for _ in range(iterations):
    index, _ = assign(x, codebook)
    codebook, _, _ = update(x, index, codebook, weights)
  index, d = assign(x, codebook)
  return codebook, index, d
