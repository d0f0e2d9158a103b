"""Plain numpy / Python restatement of the fixed-budget densification kernels (csrc/relocate.hip): the float32 threshold
test, the double weights, an integer CDF with Python ints, the draw ``(r * total) >> 64``, the opacity / scale correction
of 3DGS-MCMC in float64 with ``math.comb``, and the position noise in float64.  Written from the formulas, not from the
kernels: no table, no reordered sums."""
import bisect
import math

import numpy as np

MAX_RATIO = 51
WEIGHT_ONE = float(1 << 24)


def threshold(min_opacity):
  """float32(logit(min_opacity)), the logit in float64"""
  return np.float32(math.log(min_opacity / (1.0 - min_opacity)))


def dead_rows(alpha_logit, min_opacity):
  """bool (N,): !(alpha_logit > t) in float32; NaN is dead"""
  a = np.asarray(alpha_logit, dtype=np.float32).reshape(-1)
  return ~(a > threshold(min_opacity))


def weights(alpha_logit, min_opacity):
  """int64 (N,): 0 for a dead row, else max(1, rint(sigmoid(a) 2^24)) in double (rint = llrint: half to even)"""
  a = np.asarray(alpha_logit, dtype=np.float32).reshape(-1)
  dead = dead_rows(a, min_opacity)
  with np.errstate(over='ignore', invalid='ignore'):
    w = np.rint(WEIGHT_ONE / (1.0 + np.exp(-a.astype(np.float64))))
  w = np.where(dead, 0.0, np.maximum(np.nan_to_num(w), 1.0))
  return w.astype(np.int64)


def draw(weight, random_words):
  """(src, count, total) from integer weights and N unsigned 64-bit words (given as Python ints or a uint64 array)."""
  w = [int(x) for x in weight]
  n = len(w)
  cdf, total = [], 0
  for x in w:
    total += x
    cdf.append(total)
  src, count = list(range(n)), [0] * n
  if total > 0:
    for i in range(n):
      if w[i] == 0:
        target = (int(random_words[i]) * total) >> 64
        j = bisect.bisect_right(cdf, target)        # the first j with cdf[j] > target
        src[i] = j
        count[j] += 1
  return np.asarray(src, dtype=np.int64), np.asarray(count, dtype=np.int64), total


def opacity_and_coeff(o, ratio):
  """(o', coeff) of one gaussian of opacity o that becomes `ratio` gaussians, in float64."""
  new = 1.0 - (1.0 - o) ** (1.0 / ratio)
  denom = 0.0
  for i in range(1, ratio + 1):
    for k in range(i):
      denom += math.comb(i - 1, k) * (-1.0) ** k * new ** (k + 1) / math.sqrt(k + 1)
  return new, o / denom


def fresh(alpha_logit, log_scaling, count, min_opacity):
  """float64 (alpha_logit', log_scaling') of every row; rows with count == 0 are returned as they came."""
  a = np.asarray(alpha_logit, dtype=np.float32).reshape(-1).astype(np.float64)
  ls = np.asarray(log_scaling, dtype=np.float32).astype(np.float64).copy()
  out_a = a.copy()
  for j in np.nonzero(np.asarray(count) > 0)[0]:
    ratio = min(int(count[j]) + 1, MAX_RATIO)
    o = 1.0 / (1.0 + math.exp(-a[j]))
    new, coeff = opacity_and_coeff(o, ratio)
    c = min(max(new, min_opacity), 1.0 - 1e-7)
    out_a[j] = math.log(c / (1.0 - c))
    ls[j] += math.log(coeff)
  return out_a, ls


def quat_to_mat(q):
  x, y, z, w = (q[..., i] for i in range(4))
  return np.stack([1 - 2 * y * y - 2 * z * z, 2 * x * y - 2 * w * z, 2 * x * z + 2 * w * y,
                   2 * x * y + 2 * w * z, 1 - 2 * x * x - 2 * z * z, 2 * y * z - 2 * w * x,
                   2 * x * z - 2 * w * y, 2 * y * z + 2 * w * x, 1 - 2 * x * x - 2 * y * y], -1).reshape(q.shape[:-1] + (3, 3))


def perturbation(log_scaling, rotation, alpha_logit, z, step, k=100.0, x0=0.995):
  """float64 (delta (N, 3), g (N,), max |Sigma_ij| (N,)): delta = step g(o) Sigma z."""
  ls = np.asarray(log_scaling, dtype=np.float64)
  q = np.asarray(rotation, dtype=np.float64)
  a = np.asarray(alpha_logit, dtype=np.float64).reshape(-1)
  z = np.asarray(z, dtype=np.float64)
  R = quat_to_mat(q / np.linalg.norm(q, axis=-1, keepdims=True))
  sigma = np.einsum('nik,nk,njk->nij', R, np.exp(2.0 * ls), R)
  with np.errstate(over='ignore'):
    o = 1.0 / (1.0 + np.exp(-a))
    g = 1.0 / (1.0 + np.exp(-k * ((1.0 - o) - x0)))
  delta = step * g[:, None] * np.einsum('nij,nj->ni', sigma, z)
  return delta, g, np.abs(sigma).max(axis=(1, 2))
