"""numpy / float64 oracle of the mesh clean-up calls (taichi_splatting_amd/mesh.py, csrc/mesh.hip).  No GPU.

Labels: union-find over the faces, the larger root hooked under the smaller, so a component's root is its smallest vertex
index; labels are the ranks of the referenced roots in ascending index; unreferenced vertices get -1.
tests/test_mesh_host.py checks the partition against scipy.sparse.csgraph.connected_components.

Selection: kept faces in input order, the vertices they reference in input order, indices remapped.

Normals: s(v) = sum over the corners (f, k) with faces[f][k] == v of (b - a) x (c - a), evaluated in float64 on the positions
it is given (the tests pass the float32 positions, converted exactly).  ``normal_scale`` is S(v) = sum over the same
corners of |b - a| |c - a|, the scale of the rounding bound.

THE BOUND ON THE KERNEL'S SUM (NORMAL_C).  include/mi355_splat.h states the kernel's operations: float32 positions are
converted to float64 (exact), and differences, products, the cross product's subtractions and the running sum are float64
operations in ascending corner order; the result is rounded to float32 ONCE.  With u = 2^-53 and e = 2^-24:
  * a difference of two float32 numbers in float64 carries a relative error <= u; a product of two such differences
    (1 + u)^3; the subtraction of two products one more u: one face's cross-product component is off by at most
    4 u (|u_y w_z| + |u_z w_y|) <= 4 u |b - a| |c - a| (first order);
  * an in-order sum of deg terms adds at most (deg - 1) u times the sum of the magnitudes, <= (deg - 1) u S(v);
  * so the float64 value differs from the exact one by at most (deg + 3) u S(v), and this oracle — the same operations in
    another order — by as much again: 2 (deg + 3) u S(v) = 2 (deg + 3) 2^-29 e S(v) < e S(v) / 4 for deg < 2^25;
  * the one rounding to float32 adds e |s_k| <= e S(v) per component (a float32 subnormal result — |s_k| < 2^-126 —
    would add 2^-150 instead; the test meshes have edge lengths of order 0.1 to 1 and do not come near).
Together |s - s64| <= (1 + 1/4) e S(v) per component: NORMAL_C = 2 holds with room, for every degree the tests use.  (Had
the kernel formed differences, products and the sum in float32, the constant would be 8 + deg.)

The unit normal, where it is well conditioned (|s64| >= 0.1 S(v)): the kernel divides its float64 sum by its float64
length and rounds once.  A perturbation d of s moves s / |s| by at most 2 |d| / |s| (|d| <= |s| / 2); the float64 sum is
within e S(v) / 4 per component, sqrt(3) e S(v) / 4 in norm, of s64, so the direction moves by at most
2 sqrt(3) (e / 4) / 0.1 < 2 NORMAL_C e / 0.1 per component, and the final rounding adds e (|n_k| <= 1):
UNIT_NORMAL_BOUND = 2 NORMAL_C e / 0.1 + e.
"""
import functools

import numpy as np

EPS = 2.0 ** -24
NORMAL_C = 2.0
WELL_CONDITIONED = 0.1
UNIT_NORMAL_BOUND = 2.0 * NORMAL_C * EPS / WELL_CONDITIONED + EPS


# ---- the three rules ---------------------------------------------------------------------------------------------------

def _check(num_vertices, faces):
  faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  if faces.size and (faces.min() < 0 or faces.max() >= num_vertices):
    raise ValueError(f"a face refers to a vertex outside 0..{num_vertices - 1}")
  return faces


def components(num_vertices, faces):
  """-> dict(vertex_label (V,) int32, face_label (T,) int32, num_components, face_count (K,), vertex_count (K,))"""
  faces = _check(num_vertices, faces)
  parent = list(range(num_vertices))

  def find(x):
    root = x
    while parent[root] != root:
      root = parent[root]
    while parent[x] != root:
      parent[x], x = root, parent[x]
    return root

  for a, b, c in faces.tolist():
    for p, q in ((a, b), (b, c)):
      rp, rq = find(p), find(q)
      if rp != rq:
        parent[max(rp, rq)] = min(rp, rq)
  root = np.array([find(v) for v in range(num_vertices)], dtype=np.int64).reshape(num_vertices)
  referenced = np.zeros((num_vertices,), dtype=bool)
  referenced[faces.reshape(-1)] = True
  is_root = referenced & (root == np.arange(num_vertices))
  rank = np.cumsum(is_root) - 1
  vertex_label = np.where(referenced, rank[root] if num_vertices else root, -1).astype(np.int32)
  face_label = vertex_label[faces[:, 0]].astype(np.int32) if faces.shape[0] else np.zeros((0,), dtype=np.int32)
  count = int(is_root.sum())
  return dict(vertex_label=vertex_label, face_label=face_label, num_components=count,
              face_count=np.bincount(face_label, minlength=count).astype(np.int32),
              vertex_count=np.bincount(vertex_label[referenced], minlength=count).astype(np.int32))


def select(vertices, faces, mask, colours=None, normals=None):
  """-> (vertices, faces, colours, normals) of the kept faces: stable, rows copied, indices remapped"""
  vertices = np.asarray(vertices)
  faces = _check(vertices.shape[0], faces)
  mask = np.asarray(mask, dtype=bool)
  kept = faces[mask]
  used = np.zeros((vertices.shape[0],), dtype=bool)
  used[kept.reshape(-1)] = True
  remap = np.cumsum(used) - 1
  carry = lambda rows: None if rows is None else np.asarray(rows)[used]
  return vertices[used], remap[kept].astype(np.int32).reshape(-1, 3), carry(colours), carry(normals)


def keep_mask(face_label, face_count, min_faces=1, keep_largest=None):
  """(T,) bool mask of remove_small_components: components with face_count >= min_faces, of those the keep_largest
  largest by face count, ties to the lower label"""
  face_count = np.asarray(face_count, dtype=np.int64)
  large = face_count >= min_faces
  keep = large.copy()
  if keep_largest is not None:
    order = sorted(np.flatnonzero(large).tolist(), key=lambda k: (-int(face_count[k]), k))[:keep_largest]
    keep = np.zeros_like(large)
    keep[order] = True
  face_label = np.asarray(face_label, dtype=np.int64)
  return np.where(face_label >= 0, keep[np.clip(face_label, 0, max(len(keep) - 1, 0))] if len(keep) else False, False)


def _corner_terms(vertices, faces):
  p = np.asarray(vertices, dtype=np.float64)
  faces = _check(p.shape[0], faces)
  a, b, c = p[faces[:, 0]], p[faces[:, 1]], p[faces[:, 2]]
  return p, faces, np.cross(b - a, c - a), np.linalg.norm(b - a, axis=1) * np.linalg.norm(c - a, axis=1)


def normal_sums(vertices, faces):
  """(V, 3) float64: s(v), summed per corner"""
  p, faces, cross, _ = _corner_terms(vertices, faces)
  out = np.zeros((p.shape[0], 3), dtype=np.float64)
  for k in range(3):
    np.add.at(out, faces[:, k], cross)
  return out


def normal_scale(vertices, faces):
  """(V,) float64: S(v) = sum over the corners at v of |b - a| |c - a|"""
  p, faces, _, scale = _corner_terms(vertices, faces)
  out = np.zeros((p.shape[0],), dtype=np.float64)
  for k in range(3):
    np.add.at(out, faces[:, k], scale)
  return out


def unit_normals(vertices, faces):
  """(V, 3) float64 s / |s|, zero where |s| = 0"""
  s = normal_sums(vertices, faces)
  length = np.linalg.norm(s, axis=1, keepdims=True)
  return np.divide(s, length, out=np.zeros_like(s), where=length > 0)


def degree(num_vertices, faces):
  return np.bincount(_check(num_vertices, faces).reshape(-1), minlength=num_vertices)


# ---- mesh builders: (vertices (V, 3) float32, faces (T, 3) int32) ------------------------------------------------------

def strip(triangles, seed=0):
  """a zig-zag strip of `triangles` triangles on triangles + 2 vertices with ascending indices, consistently oriented
  (all normals on the same, -z, side), slightly bent so that no normal sum vanishes"""
  rng = np.random.default_rng(seed)
  n = triangles + 2
  i = np.arange(n)
  vertices = np.stack([0.5 * i, (i % 2).astype(np.float64), 0.05 * rng.standard_normal(n)], axis=1)
  t = np.arange(triangles)
  even = (t % 2 == 0)
  faces = np.stack([t, np.where(even, t + 1, t + 2), np.where(even, t + 2, t + 1)], axis=1)
  return vertices.astype(np.float32), faces.astype(np.int32)


def fan(triangles, hub_last=True, seed=0):
  """`triangles` faces round one hub (a cone): rim vertex i, i + 1 and the hub, which carries the highest index when
  hub_last (every hook then contends for the hub's root) and index 0 otherwise"""
  rng = np.random.default_rng(seed)
  angle = 2 * np.pi * np.arange(triangles) / triangles
  rim = np.stack([np.cos(angle), np.sin(angle), 0.01 * rng.standard_normal(triangles)], axis=1)
  hub = np.array([[0.0, 0.0, 0.7]])
  r = np.arange(triangles)
  nxt = (r + 1) % triangles
  if hub_last:
    vertices = np.concatenate([rim, hub])
    faces = np.stack([np.full_like(r, triangles), r, nxt], axis=1)
  else:
    vertices = np.concatenate([hub, rim])
    faces = np.stack([np.zeros_like(r), r + 1, nxt + 1], axis=1)
  return vertices.astype(np.float32), faces.astype(np.int32)


def soup(singles, big, unreferenced, seed=0):
  """`singles` single-triangle components beside one strip component of `big` faces, then `unreferenced` vertices no
  face uses; the vertex numbering is shuffled so that the components interleave"""
  rng = np.random.default_rng(seed)
  sv, sf = strip(big, seed)
  tv = rng.uniform(-1.0, 1.0, size=(singles, 3, 3)) + rng.uniform(-20.0, 20.0, size=(singles, 1, 3))
  tf = np.arange(3 * singles).reshape(singles, 3) + sv.shape[0]
  loose = rng.uniform(-20.0, 20.0, size=(unreferenced, 3))
  vertices = np.concatenate([sv.astype(np.float64), tv.reshape(-1, 3), loose]).astype(np.float32)
  faces = np.concatenate([sf.astype(np.int64), tf])
  vertices, faces = permute_vertices(vertices, faces, rng.permutation(vertices.shape[0]))
  return vertices, shuffle_faces(faces, seed + 1)


H = 0.25
ORIGIN = (0.5, 1.0, 0.25)
GRID = (21, 21, 21)
CENTRE = np.array([0.5 + 2.5 + 0.03, 1.0 + 2.5 - 0.02, 0.25 + 2.5 + 0.01])
SPHERE_RADIUS = 6.3 * H


def analytic_field(kind, dims=GRID):
  """the 21^3 sphere and torus fields of tests/test_gpu_tsdf.py: (tsdf (nz, ny, nx) float32, weight)"""
  from tests import tsdf_oracle as to
  positions = to.grid_positions(ORIGIN, H, dims)
  field = to.sphere_field(positions, CENTRE, SPHERE_RADIUS) if kind == 'sphere' else to.torus_field(positions, CENTRE, 1.5, 0.6)
  values = field.astype(np.float32)
  return values, np.ones_like(values)


@functools.lru_cache(maxsize=None)
def analytic_mesh(kind):
  """the oracle's marching-tetrahedra mesh of analytic_field(kind): (vertices float32, faces int32); do not modify"""
  from tests import tsdf_oracle as to
  values, weight = analytic_field(kind)
  vertices, faces, _ = to.marching_tetrahedra(values, weight, ORIGIN, H)
  return np.asarray(vertices).astype(np.float32), np.asarray(faces).astype(np.int32)


def permute_vertices(vertices, faces, new_index):
  """renumber: old vertex v becomes new_index[v] (positions move with their vertices)"""
  new_index = np.asarray(new_index, dtype=np.int64)
  out = np.empty_like(np.asarray(vertices))
  out[new_index] = vertices
  return out, new_index[np.asarray(faces, dtype=np.int64)].astype(np.int32)


def shuffle_faces(faces, seed=0):
  faces = np.asarray(faces)
  return np.ascontiguousarray(faces[np.random.default_rng(seed).permutation(faces.shape[0])]).astype(np.int32)


def same_partition(label_a, label_b):
  """do two label arrays (any numbering, -1 = none) describe the same partition?"""
  label_a, label_b = np.asarray(label_a, dtype=np.int64), np.asarray(label_b, dtype=np.int64)
  if label_a.shape != label_b.shape or not np.array_equal(label_a < 0, label_b < 0):
    return False
  live = label_a >= 0
  pairs = np.unique(np.stack([label_a[live], label_b[live]], axis=1), axis=0)
  return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


# ---- reading back what save_mesh_ply wrote -----------------------------------------------------------------------------

def read_mesh_ply(path):
  """-> dict(properties=[names], vertex=structured array, faces (T, 3) int32) of a binary little-endian PLY with a vertex
  element of float / uchar properties and a face element of `list uchar int vertex_indices` triangles"""
  kinds = {'float': '<f4', 'uchar': 'u1', 'int': '<i4', 'double': '<f8'}
  with open(path, 'rb') as f:
    data = f.read()
  end = data.index(b'end_header\n') + len(b'end_header\n')
  lines = data[:end].decode('ascii').splitlines()
  assert lines[0] == 'ply' and lines[1] == 'format binary_little_endian 1.0', lines[:2]
  counts, fields, element = {}, [], None
  for line in lines[2:]:
    words = line.split()
    if words[0] == 'element':
      element = words[1]
      counts[element] = int(words[2])
    elif words[0] == 'property' and element == 'vertex':
      fields.append((words[2], kinds[words[1]]))
    elif words[0] == 'property':
      assert words[1:] == ['list', 'uchar', 'int', 'vertex_indices'], line
  vertex_type = np.dtype(fields)
  vertex = np.frombuffer(data, dtype=vertex_type, count=counts['vertex'], offset=end)
  face_type = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
  offset = end + counts['vertex'] * vertex_type.itemsize
  faces = np.frombuffer(data, dtype=face_type, count=counts['face'], offset=offset)
  assert offset + counts['face'] * face_type.itemsize == len(data), "trailing or missing bytes"
  assert (faces['n'] == 3).all()
  return dict(properties=[name for name, _ in fields], vertex=vertex, faces=faces['v'].astype(np.int32).reshape(-1, 3))
