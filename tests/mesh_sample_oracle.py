"""numpy oracle of the surface sampler (csrc/mesh_sample.hip; the rules are stated in include/mi355_splat.h).  No GPU.

Generator, restated: mix(x): x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16 on uint32;
word(seed, i, j) = mix(i + mix(seed + 0x9e3779b9 (j + 1))); u_j = (word >> 8) 2^-24.

Two forms of a sample: ``restate`` repeats the kernel's own operations in the kernel's own precisions (float64 stratum
and search, float32 weights), so faces and weights are compared bit for bit; ``sample`` evaluates the same points in
float64 from the float64 weights, the reference the float32 points are held to.
"""
import numpy as np

MASK = np.uint64(0xffffffff)


def mix(x):
  """uint32 -> uint32 (arrays or scalars); the products are taken in uint64 and masked"""
  x = np.asarray(x, dtype=np.uint64) & MASK
  x = x ^ (x >> np.uint64(16))
  x = (x * np.uint64(0x7feb352d)) & MASK
  x = x ^ (x >> np.uint64(15))
  x = (x * np.uint64(0x846ca68b)) & MASK
  x = x ^ (x >> np.uint64(16))
  return x.astype(np.uint32)


def word(seed, i, j):
  inner = mix((np.uint64(int(seed) & 0xffffffff) + np.uint64(0x9e3779b9) * np.uint64(j + 1)) & MASK)
  return mix((np.asarray(i, dtype=np.uint64) + inner.astype(np.uint64)) & MASK)


def unit(seed, i, j):
  """u_j as float64 (a multiple of 2^-24 in [0, 1): exact in float32 as well)"""
  return (word(seed, i, j) >> np.uint32(8)).astype(np.float64) * 2.0 ** -24


def face_areas(vertices, faces):
  """(T,) float64: 0.5 |(b - a) x (c - a)| in float64 on the positions as given"""
  p = np.asarray(vertices, dtype=np.float64)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  m = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
  return 0.5 * np.sqrt((m[:, 0] * m[:, 0] + m[:, 1] * m[:, 1]) + m[:, 2] * m[:, 2])


def strata(cdf, n, seed):
  """t_i (n,) float64 as the kernel forms it: min((i + u0) (cdf[-1] / n), nextafter(cdf[-1], 0))"""
  cdf = np.asarray(cdf, dtype=np.float64)
  i = np.arange(n, dtype=np.uint64)
  total = cdf[-1]
  return np.minimum((i.astype(np.float64) + unit(seed, i, 0)) * (total / np.float64(n)), np.nextafter(total, 0.0))


def restate(cdf, n, seed):
  """(faces (n,) int64, barycentric (n, 3) float32): the kernel's operations in the kernel's precisions"""
  cdf = np.asarray(cdf, dtype=np.float64)
  i = np.arange(n, dtype=np.uint64)
  face = np.searchsorted(cdf, strata(cdf, n, seed), side='right')
  u1, u2 = unit(seed, i, 1).astype(np.float32), unit(seed, i, 2).astype(np.float32)
  r = np.sqrt(u1)                                            # float32, correctly rounded
  one = np.float32(1.0)
  return face, np.stack([one - r, r * (one - u2), r * u2], axis=1)


def sample(vertices, faces, cdf, n, seed):
  """(points (n, 3) float64, faces (n,) int64, barycentric (n, 3) float64): the float32 weights of ``restate`` (they are
  part of the rule), combined with the positions in float64"""
  face, weights = restate(cdf, n, seed)
  p = np.asarray(vertices, dtype=np.float64)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face]
  w = weights.astype(np.float64)
  return w[:, 0:1] * p[f[:, 0]] + w[:, 1:2] * p[f[:, 1]] + w[:, 2:3] * p[f[:, 2]], face, w


def combine_f32(rows, faces, face, weights):
  """(wa A + wb B) + wc C per component in float32, every operation rounded once: the kernel's expression"""
  rows = np.asarray(rows, dtype=np.float32)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)[face]
  w = np.asarray(weights, dtype=np.float32)
  return (w[:, 0:1] * rows[f[:, 0]] + w[:, 1:2] * rows[f[:, 1]]) + w[:, 2:3] * rows[f[:, 2]]


def face_unit_normals(vertices, faces):
  """(T, 3) float64: (b - a) x (c - a) / |.|, zero for a face of zero area"""
  p = np.asarray(vertices, dtype=np.float64)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  m = np.cross(p[f[:, 1]] - p[f[:, 0]], p[f[:, 2]] - p[f[:, 0]])
  length = np.linalg.norm(m, axis=1, keepdims=True)
  return np.divide(m, length, out=np.zeros_like(m), where=length > 0)
