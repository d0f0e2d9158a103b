"""numpy / float64 oracle of ``simplify_mesh`` (taichi_splatting_amd/mesh.py, csrc/mesh_simplify.hip).  No GPU.

The four rules of include/mi355_splat.h, straight from their statement:

CELL RULE.  cell(p) = floor((p - origin) / cell_size) per axis IN FLOAT32 — ``cells`` below is three numpy float32
operations, each one correctly rounded IEEE operation, so it gives the kernel's cell bit for bit.  Key z << 42 | y << 21 | x.
ORDER RULE.  Clusters in ascending key, members in ascending vertex index, faces in input order.
FACE RULE.  Rewrite, drop a face with two equal corners, rotate the smallest index first, keep the lowest input index of
equal triples, drop the clusters no face is left in.
PLACEMENT RULE.  In float64 on the float32 positions: xm = mean of the members; over the corners (f, k) of the cluster
m = (b - a) x (c - a), d = -m . (a - xm), A = sum m m^T, r = sum d m, x = xm - (A + lambda I)^-1 r with
lambda = regularisation trace(A) / 3 (numpy.linalg.solve here, the adjugate in the kernel).  x rounded to float32 once is
taken if it lies in the cluster's own cell by the CELL RULE; else, or when trace(A) == 0 or x is not finite, xm rounded
once under the same test; else the member with the lowest index.

What ``simplify`` reports per cluster beside the result, for the tests to choose their inputs by:
  condition    the condition number of A + lambda I (<= 1 + 3 / regularisation: A is positive semi-definite and
               lambda = regularisation trace(A) / 3 >= regularisation lambda_max / 3)
  margin       the distance of the UNROUNDED optimum to the nearest face of its cell as a fraction of cell_size (negative
               outside the cell): a cluster whose margin is within 1e-4 of zero may take the quadric position in one
               evaluation and the mean in another
  error_bound  a bound on the error of a float64 evaluation of x, per coordinate, derived below

THE BOUND ON A FLOAT64 EVALUATION (error_bound).  u = 2^-53; first order in u; constants rounded up.  Let n be the number
of members, t the number of corners ("terms"), P the largest |coordinate| of a member, D the largest |a - xm| over the
corners, S = sum |m|^2 = trace(A), kappa the condition number of M = A + lambda I and y = x - xm.
  * xm: a sum of n float64 terms in any order and one division: (n + 1) u P.
  * one term of r: differences (u each), the cross product (3 u), the dot product with a - xm (4 u), the product d m (u):
    at most 12 u |m|^2 D; summing t of them in any order adds (t - 1) u sum |d m|: |delta r| <= (t + 12) u S D.  Likewise
    |delta A| <= (t + 12) u S, so |delta A y| <= (t + 12) u S |y|.
  * the exact solve maps a perturbation through M^-1, and |M^-1| = kappa / lambda_max(M) <= 3 kappa / S because
    lambda_max(M) >= trace(M) / 3 >= S / 3.  So the data errors move y by at most 3 kappa (t + 12) u (D + |y|):
    terms x 2^-53 x condition, times the length scale.
  * the closed form itself (the kernel's adjugate over determinant; LU with pivoting here is no worse): a cofactor is a
    difference of two products of entries <= lambda_max, error <= 3 u lambda_max^2; the determinant, a sum of three
    products of magnitude <= lambda_max^3, has an absolute error <= 8 u lambda_max^3 against a value
    lambda_1 lambda_2 lambda_3 >= lambda_max^3 / kappa^2: a relative error <= 8 kappa^2 u, and the numerator adj r loses
    as much against |y| det.  Together <= 16 kappa^2 u |y|.
error_bound = u ((n + 1) P + 3 kappa (t + 12) (D + |y|) + 16 kappa^2 |y|).  Two float64 evaluations (the kernel's and this
one) lie within twice that of each other; where that is below HALF a float32 ulp — error_bound below a QUARTER — their
single roundings to float32 give the same or adjacent floats.  ``cell_ulp`` is the float32 spacing at the largest
|coordinate| of the cluster's cell, per axis: positions in the cell have that spacing or a finer one.
"""
import numpy as np

CELL_BITS = 21
MAX_CELL = 2 ** CELL_BITS - 1
QUADRIC, MEAN, MEMBER = 0, 1, 2
U = 2.0 ** -53
FLIP_MARGIN = 1e-4          # of a cell: closer to a cell face than this, quadric / mean may flip between two evaluations


def cells(points, origin, cell_size):
  """CELL RULE: (n, 3) float32 whole numbers (or inf / nan), by three float32 operations"""
  points = np.asarray(points, dtype=np.float32).reshape(-1, 3)
  origin = np.asarray(origin, dtype=np.float32).reshape(3)
  with np.errstate(all='ignore'):
    out = np.floor((points - origin) / np.float32(cell_size))
  assert out.dtype == np.float32
  return out


def keys_of(cell):
  cell = np.asarray(cell).astype(np.int64)
  return (cell[:, 2] << (2 * CELL_BITS)) | (cell[:, 1] << CELL_BITS) | cell[:, 0]


def default_origin(vertices):
  """the smallest finite coordinate of ALL vertices per axis ((0, 0, 0) for no vertex), -0 counting as below +0: the
  bits of the result are defined too"""
  vertices = np.asarray(vertices, dtype=np.float32).reshape(-1, 3)
  if vertices.shape[0] == 0:
    return np.zeros((3,), dtype=np.float32)
  low = np.where(np.isfinite(vertices), vertices, np.float32(np.inf)).min(axis=0).astype(np.float32)
  minus_zero = ((vertices == 0) & np.signbit(vertices)).any(axis=0)
  zero = np.where(minus_zero, np.float32(-0.0), np.float32(0.0))
  return np.where(low == 0, zero, low).astype(np.float32)


def _inside(position32, origin, cell_size, cell):
  got = cells(position32, origin, cell_size)[0]
  return bool(np.all(np.isfinite(got)) and np.array_equal(got, cell.astype(np.float32)))


def simplify(vertices, faces, cell_size, origin=None, placement='quadric', regularisation=1e-3, colours=None):
  """-> dict: vertices (V', 3) float32, faces (T', 3) int32, colours (V', 3) float32 or None, vertex_map (V,) int32, and
  per OUTPUT vertex: cell (V', 3) int64, choice (V',), quadric and mean (V', 3) float32 = the two candidate positions
  (quadric is NaN where there is none), condition, margin, error_bound (V',), cell_ulp (V', 3), members, corners (V',)"""
  vertices = np.ascontiguousarray(vertices, dtype=np.float32).reshape(-1, 3)
  faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  num_vertices = vertices.shape[0]
  if placement not in ('quadric', 'mean'):
    raise ValueError(f"unknown placement {placement!r}")
  if not (np.isfinite(np.float32(cell_size)) and np.float32(cell_size) > 0):
    raise ValueError("cell_size must be a finite positive float32")
  if not (np.isfinite(regularisation) and regularisation > 0):
    raise ValueError("regularisation must be finite and > 0")
  if faces.size and (faces.min() < 0 or faces.max() >= num_vertices):
    raise ValueError(f"a face refers to a vertex outside 0..{num_vertices - 1}")
  origin = default_origin(vertices) if origin is None else np.asarray(origin, dtype=np.float32)
  if origin.shape != (3,):
    raise ValueError("origin must be (3,)")
  cell_size = np.float32(cell_size)
  referenced = np.zeros((num_vertices,), dtype=bool)
  referenced[faces.reshape(-1)] = True
  live = np.flatnonzero(referenced)
  if not np.isfinite(vertices[live]).all():
    raise ValueError("a vertex that a face references is not finite")
  cell = cells(vertices[live], origin, cell_size)
  if not (np.isfinite(cell).all() and (cell >= 0).all() and (cell <= MAX_CELL).all()):
    raise ValueError(f"a vertex that a face references falls into a cell outside 0..{MAX_CELL}")
  cell = cell.astype(np.int64)
  cluster_keys, first, inverse = np.unique(keys_of(cell), return_index=True, return_inverse=True)      # ascending keys
  num_clusters = cluster_keys.shape[0]
  vertex_cluster = np.full((num_vertices,), -1, dtype=np.int64)
  vertex_cluster[live] = inverse.reshape(-1)
  cluster_cell = cell[first]

  # FACE RULE
  rewritten = vertex_cluster[faces]
  seen, kept_faces = set(), []
  for p, q, r in rewritten.tolist():
    if p == q or q == r or r == p:
      continue
    triple = (p, q, r) if p < q and p < r else ((q, r, p) if q < r else (r, p, q))
    if triple not in seen:
      seen.add(triple)
      kept_faces.append(triple)
  kept_faces = np.asarray(kept_faces, dtype=np.int64).reshape(-1, 3)
  used = np.zeros((num_clusters,), dtype=bool)
  used[kept_faces.reshape(-1)] = True
  new_index = np.where(used, np.cumsum(used) - 1, -1)
  vertex_map = np.append(new_index, -1)[vertex_cluster].astype(np.int32)          # cluster -1 reads the appended -1

  # PLACEMENT RULE, for the clusters that stay
  positions64 = vertices.astype(np.float64)
  corner_cluster = rewritten.reshape(-1)
  corner_order = np.argsort(corner_cluster, kind='stable')
  corner_bounds = np.searchsorted(corner_cluster[corner_order], np.arange(num_clusters + 1))
  member_order = live[np.argsort(inverse.reshape(-1), kind='stable')]
  member_bounds = np.searchsorted(np.sort(inverse.reshape(-1)), np.arange(num_clusters + 1))
  out = {k: [] for k in ('vertices', 'colours', 'cell', 'choice', 'quadric', 'mean', 'condition', 'margin', 'error_bound',
                         'cell_ulp', 'members', 'corners')}
  origin64, size64 = origin.astype(np.float64), float(cell_size)
  for c in np.flatnonzero(used):
    members = member_order[member_bounds[c]:member_bounds[c + 1]]
    corners = corner_order[corner_bounds[c]:corner_bounds[c + 1]]
    mean = positions64[members].sum(axis=0) / members.shape[0]
    mean32 = mean.astype(np.float32)
    quadric32 = np.full((3,), np.nan, dtype=np.float32)
    condition, margin, bound = 1.0, np.nan, (members.shape[0] + 1) * U * np.abs(positions64[members]).max()
    choice = MEMBER
    if placement == 'quadric':
      a, b, d = (positions64[faces[corners // 3, k]] for k in range(3))
      m = np.cross(b - a, d - a)
      dist = -np.einsum('ij,ij->i', m, a - mean)
      A = m.T @ m
      r = m.T @ dist
      trace = float(np.trace(A))
      if trace > 0 and np.isfinite(trace):
        M = A + regularisation * trace / 3.0 * np.eye(3)
        y = np.linalg.solve(M, r)
        x = mean - y
        eigen = np.linalg.eigvalsh(M)
        condition = float(eigen[-1] / eigen[0])
        low = origin64 + cluster_cell[c] * size64
        margin = float(np.minimum(x - low, low + size64 - x).min() / size64)
        reach = float(np.linalg.norm(a - mean, axis=1).max())
        length = float(np.linalg.norm(y))
        bound += U * (3.0 * condition * (corners.shape[0] + 12) * (reach + length) + 16.0 * condition ** 2 * length)
        if np.isfinite(x).all():
          quadric32 = x.astype(np.float32)
          if _inside(quadric32, origin, cell_size, cluster_cell[c]):
            choice = QUADRIC
    if choice == MEMBER and _inside(mean32, origin, cell_size, cluster_cell[c]):
      choice = MEAN
    position = quadric32 if choice == QUADRIC else (mean32 if choice == MEAN else vertices[members[0]])
    low32 = origin64 + cluster_cell[c] * size64
    out['vertices'].append(position)
    out['colours'].append(None if colours is None else
                          (np.asarray(colours, dtype=np.float32)[members].astype(np.float64).sum(axis=0) / members.shape[0]).astype(np.float32))
    out['cell'].append(cluster_cell[c])
    out['choice'].append(choice)
    out['quadric'].append(quadric32)
    out['mean'].append(mean32)
    out['condition'].append(condition)
    out['margin'].append(margin)
    out['error_bound'].append(bound)
    out['cell_ulp'].append(np.spacing(np.maximum(np.abs(low32), np.abs(low32 + size64)).astype(np.float32)))
    out['members'].append(members.shape[0])
    out['corners'].append(corners.shape[0])
  count = int(used.sum())
  shapes = {'vertices': ((count, 3), np.float32), 'colours': ((count, 3), np.float32), 'cell': ((count, 3), np.int64),
            'choice': ((count,), np.int64), 'quadric': ((count, 3), np.float32), 'mean': ((count, 3), np.float32),
            'condition': ((count,), np.float64), 'margin': ((count,), np.float64), 'error_bound': ((count,), np.float64),
            'cell_ulp': ((count, 3), np.float32), 'members': ((count,), np.int64), 'corners': ((count,), np.int64)}
  result = {k: np.asarray(v, dtype=shapes[k][1]).reshape(shapes[k][0]) for k, v in out.items() if not (k == 'colours' and colours is None)}
  result['colours'] = result.get('colours')
  result['faces'] = new_index[kept_faces].astype(np.int32).reshape(-1, 3)
  result['vertex_map'] = vertex_map
  result['origin'] = origin
  return result


# ---- the meshes of the tests -----------------------------------------------------------------------------------------------

def icosphere(subdivisions, radius=1.0):
  """unit icosahedron subdivided: 10 * 4^s + 2 vertices, 20 * 4^s faces, outward orientation; float32 vertices"""
  t = (1.0 + 5.0 ** 0.5) / 2.0
  vertices = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t),
              (t, 0, -1), (t, 0, 1), (-t, 0, -1), (-t, 0, 1)]
  vertices = [np.asarray(v, dtype=np.float64) / np.linalg.norm(v) for v in vertices]
  faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
           (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
  for _ in range(subdivisions):
    middle, refined = {}, []

    def mid(i, j):
      key = (min(i, j), max(i, j))
      if key not in middle:
        point = vertices[i] + vertices[j]
        vertices.append(point / np.linalg.norm(point))
        middle[key] = len(vertices) - 1
      return middle[key]

    for a, b, c in faces:
      ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
      refined += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
    faces = refined
  return (np.asarray(vertices) * radius).astype(np.float32), np.asarray(faces, dtype=np.int32)


def cube_surface(n=12):
  """the surface of the unit cube, n x n quads per side split into two triangles, welded: (n + 1)^3 - (n - 1)^3 vertices,
  12 n^2 faces, outward orientation"""
  index, vertices, faces = {}, [], []

  def vertex(p):
    if p not in index:
      index[p] = len(vertices)
      vertices.append([x / n for x in p])
    return index[p]

  for axis in range(3):
    u, v = (axis + 1) % 3, (axis + 2) % 3
    for side in (0, n):
      for i in range(n):
        for j in range(n):
          def corner(di, dj):
            p = [0, 0, 0]
            p[axis], p[u], p[v] = side, i + di, j + dj
            return vertex(tuple(p))
          quad = [corner(0, 0), corner(1, 0), corner(1, 1), corner(0, 1)]       # counter-clockwise seen from +axis
          if side == 0:
            quad.reverse()
          faces += [(quad[0], quad[1], quad[2]), (quad[0], quad[2], quad[3])]
  return np.asarray(vertices, dtype=np.float32), np.asarray(faces, dtype=np.int32)
