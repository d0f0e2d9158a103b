"""Float64 oracle of TSDF fusion and marching tetrahedra (taichi_splatting_amd/fusion.py, csrc/tsdf.hip): torch / numpy
on the CPU, no GPU needed.

``integrate`` is the rule of include/mi355_splat.h written with whole-volume torch operations; with ``dtype=float64`` it
is the oracle, with ``dtype=float32`` it is the composition a user would write without the kernel (same operations in
the same order, so it is also the yardstick of tools/bench_tsdf.py on the GPU).  With ``analyse=True`` (float64) it also
returns, per sample, the error bound a float32 evaluation may reach and whether the sample is ill-posed, from these
roundings (eps = 2^-24, the unit roundoff of float32; first-order terms, doubled once for the higher orders):

  p_a = o_a + v i_a            one product, one sum:  |dp_a| <= 2 eps P_a,  P_a = |o_a| + |v| i_a
  r = t_r0 px + t_r1 py + t_r2 pz + t_r3   (r = x, y, z): three products of perturbed p (3 eps |t_ra| P_a each) and three
                               sums (eps M_r each):  |dr| <= 6 eps M_r,  M_r = sum_a |t_ra| P_a + |t_r3|
  u = fx x / z + cx            product, quotient, sum:  |du| <= |fx| |dx| / |z| + |fx x / z| (2 eps + |dz| / |z|) + eps |u|
  s = d - z                    |ds| <= eps |s| + |dz|
  t = min(1, s / T)            |dt| <= |ds| / T + eps          (|t| <= 1 where the sample is not skipped)
  running mean                 a convex combination of the old value and t: it carries max(old error, |dt|) and adds
                               K' eps max(1, |value|) with K' = 4 (two products, sum, quotient) + q / 2 for the q-th
                               update of the sample — the weight itself carries q eps of relative error, and a relative
                               error e of the weight moves the combination by at most e / 2 |old - t| <= e.

A sample is ill-posed for a camera when one of the decisions it reaches can flip inside these errors: z within |dz| of a
clip plane, u or v within |du| / |dv| of an integer while the other coordinate is inside or within its own error of the
image, s within |ds| of -truncation.  The depth test d > 0 reads an input: it has no rounding and no margin.

``marching_tetrahedra`` states the triangulation contract independently of the kernel: the triangle sets per case are
those of the header, but every triangle is oriented geometrically (its normal against the direction from the inside
corners to the outside corners of the tetrahedron), not by permutation parity.
"""
import itertools
import math

import numpy as np
import torch

EPS = 2.0 ** -24
CAMERA_VALUES = 20


# ---- cameras and inputs --------------------------------------------------------------------------------------------------

def look_at(eye, target, roll=0.0):
  """(4, 4) float64 T_camera_world of a camera at ``eye`` looking at ``target`` (x right, y down, z forward), rolled"""
  eye, target = np.asarray(eye, dtype=np.float64), np.asarray(target, dtype=np.float64)
  forward = target - eye
  forward /= np.linalg.norm(forward)
  down = np.array([0.13, 1.0, 0.07])
  right = np.cross(down, forward)
  right /= np.linalg.norm(right)
  true_down = np.cross(forward, right)
  c, s = math.cos(roll), math.sin(roll)
  right, true_down = c * right + s * true_down, -s * right + c * true_down
  T = np.eye(4)
  T[:3, :3] = np.stack([right, true_down, forward])
  T[:3, 3] = -T[:3, :3] @ eye
  return T


def pack_camera(T, fx, fy, cx, cy, near, far, width, height):
  """one (20,) float32 row of the layout ``pack_cameras`` produces"""
  row = np.concatenate([np.asarray(T, dtype=np.float64)[:3].reshape(12), [fx, fy, cx, cy, near, far, width, height]])
  return torch.from_numpy(row).to(torch.float32)


def f32(x):
  return float(np.float32(x))


# ---- integration -----------------------------------------------------------------------------------------------------------

def sample_indices(dims, device='cpu'):
  """(i, j, k) of every sample in linear order (x fastest), three (n,) int64 tensors"""
  nx, ny, nz = dims
  linear = torch.arange(nx * ny * nz, device=device)
  return linear % nx, (linear // nx) % ny, linear // (nx * ny)


def integrate(tsdf, weight, colour, origin, voxel_size, truncation, max_weight, depth, cameras, image=None,
              pixel_weight=None, dtype=torch.float64, analyse=False):
  """The integration rule on whole-volume tensors of ``dtype`` (on the device of ``tsdf``).  ``tsdf`` / ``weight``
  (nz, ny, nx), ``colour`` (nz, ny, nx, 3) or None, ``cameras`` (C, 20), ``depth`` (C, H, W), ``image`` (C, H, W, 3) or
  None, ``pixel_weight`` (C, H, W) or None; origin, voxel_size, truncation and max_weight (None: no clamp) are taken as
  float32 numbers.  Returns ``(tsdf, weight, colour)`` of ``dtype``, plus with ``analyse`` a dict of (n,) tensors:
  ``bound`` / ``colour_bound`` (the float32 error bounds of the module docstring), ``ill`` (ill-posed for some camera) and
  ``updates`` (how many cameras updated the sample)."""
  nz, ny, nx = tsdf.shape
  device = tsdf.device
  n = nx * ny * nz
  count, height, width = depth.shape
  num = lambda x: torch.tensor(f32(x), dtype=dtype, device=device)
  ii, jj, kk = sample_indices((nx, ny, nz), device)
  voxel, trunc = num(voxel_size), num(truncation)
  clamp = num(math.inf if max_weight is None else max_weight)
  p = [num(origin[a]) + voxel * index.to(dtype) for a, index in enumerate((ii, jj, kk))]
  T, W = tsdf.reshape(n).to(dtype).clone(), weight.reshape(n).to(dtype).clone()
  C = None if colour is None else colour.reshape(n, 3).to(dtype).clone()
  cams = cameras.to(device=device, dtype=dtype)
  depth = depth.to(device=device, dtype=dtype).reshape(count, height * width)
  image = None if image is None else image.to(device=device, dtype=dtype).reshape(count, height * width, 3)
  pixel_weight = None if pixel_weight is None else pixel_weight.to(device=device, dtype=dtype).reshape(count, height * width)
  one = torch.ones((), dtype=dtype, device=device)
  if analyse:
    assert dtype == torch.float64
    P = [abs(f32(origin[a])) + abs(f32(voxel_size)) * index.to(dtype) for a, index in enumerate((ii, jj, kk))]
    bound, colour_bound = torch.zeros(n, dtype=dtype), torch.zeros(n, dtype=dtype)
    ill, updates = torch.zeros(n, dtype=torch.bool), torch.zeros(n, dtype=torch.int64)
    colour_scale = 1.0 if image is None else max(1.0, float(image[torch.isfinite(image)].abs().max()))

  for c in range(count):
    r = cams[c]
    z = r[8] * p[0] + r[9] * p[1] + r[10] * p[2] + r[11]
    ok = (z >= r[16]) & (z <= r[17])
    x = r[0] * p[0] + r[1] * p[1] + r[2] * p[2] + r[3]
    y = r[4] * p[0] + r[5] * p[1] + r[6] * p[2] + r[7]
    safe_z = torch.where(ok, z, one)
    u = r[12] * x / safe_z + r[14]
    v = r[13] * y / safe_z + r[15]
    after_z = ok
    ok = ok & (u >= 0) & (u < width) & (v >= 0) & (v < height)
    ix = torch.where(ok, u, torch.zeros_like(u)).floor().long().clamp(0, width - 1)
    iy = torch.where(ok, v, torch.zeros_like(v)).floor().long().clamp(0, height - 1)
    pixel = iy * width + ix
    d = depth[c][pixel]
    ok = ok & (d > 0) & torch.isfinite(d)
    pw = pixel_weight[c][pixel] if pixel_weight is not None else torch.ones_like(d)
    ok = ok & (pw > 0)
    s = d - z
    after_weight = ok
    ok = ok & ~(s < -trunc)
    t = torch.minimum(one, s / trunc)
    total = W + pw
    if analyse:
      M = [sum(r[row * 4 + a].abs() * P[a] for a in range(3)) + r[row * 4 + 3].abs() for row in range(3)]
      dx, dy, dz = (2 * 6 * EPS * m for m in M)
      az = safe_z.abs()
      du = r[12].abs() * dx / az + (r[12] * x / safe_z).abs() * (4 * EPS + dz / az) + 2 * EPS * u.abs()
      dv = r[13].abs() * dy / az + (r[13] * y / safe_z).abs() * (4 * EPS + dz / az) + 2 * EPS * v.abs()
      ds = 2 * EPS * s.abs() + dz
      ill_z = ((z - r[16]).abs() <= dz) | ((z - r[17]).abs() <= dz)
      near_u = ((u - u.round()).abs() <= du) & (u >= -du) & (u <= width + du)
      near_v = ((v - v.round()).abs() <= dv) & (v >= -dv) & (v <= height + dv)
      in_u, in_v = (u >= -du) & (u <= width + du), (v >= -dv) & (v <= height + dv)
      ill_uv = after_z & ((near_u & in_v) | (near_v & in_u))
      ill_s = after_weight & ((s + trunc).abs() <= ds)
      ill |= ill_z | ill_uv | ill_s
      q = (updates + 1).to(dtype)
      dt = ds / trunc + 2 * EPS
      step = (4 + q / 2) * EPS
      bound = torch.where(ok, torch.maximum(bound, dt) + step * torch.maximum(one, T.abs()), bound)
      colour_bound = torch.where(ok, colour_bound + step * colour_scale, colour_bound)
      updates = updates + ok.long()
    T = torch.where(ok, (W * T + pw * t) / total, T)
    if C is not None:
      C = torch.where(ok[:, None], (W[:, None] * C + pw[:, None] * image[c][pixel]) / total[:, None], C)
    W = torch.where(ok, torch.minimum(total, clamp), W)

  out = (T.reshape(nz, ny, nx), W.reshape(nz, ny, nx), None if C is None else C.reshape(nz, ny, nx, 3))
  if analyse:
    return out + (dict(bound=bound, colour_bound=colour_bound, ill=ill, updates=updates),)
  return out


# ---- marching tetrahedra -----------------------------------------------------------------------------------------------

DIRECTIONS = [(1, 0, 0), (0, 1, 0), (0, 0, 1), (1, 1, 0), (1, 0, 1), (0, 1, 1), (1, 1, 1)]      # edge types 0..6, (dx, dy, dz)
TETRAHEDRA = []                                                                                 # corner paths, lexicographic
for perm in itertools.permutations(range(3)):
  corner, path = [0, 0, 0], [(0, 0, 0)]
  for axis in perm:
    corner[axis] = 1
    path.append(tuple(corner))
  TETRAHEDRA.append(path)


def tet_triangles(inside):
  """The contract's triangle sets of one tetrahedron as triples of edges (a, b) of path corners 0..3, unoriented"""
  ins = [v for v in range(4) if inside[v]]
  outs = [v for v in range(4) if not inside[v]]
  edge = lambda a, b: (min(a, b), max(a, b))
  if len(ins) in (0, 4):
    return []
  if len(ins) == 2:
    a, b = ins
    c, d = outs
    return [(edge(a, c), edge(b, d), edge(b, c)), (edge(a, c), edge(a, d), edge(b, d))]
  a = ins[0] if len(ins) == 1 else outs[0]
  b, c, d = outs if len(ins) == 1 else ins
  return [(edge(a, b), edge(a, c), edge(a, d))]


def marching_tetrahedra(tsdf, weight, origin, voxel_size, min_weight=0.0, colour=None):
  """``(vertices (V, 3) float64, faces (T, 3) int64, colours (V, 3) | None)`` in the contract's order, from numpy /
  torch fields (nz, ny, nx); origin and voxel_size are taken as float32 numbers, positions are exact in float64."""
  t = np.asarray(tsdf, dtype=np.float64)
  w = np.asarray(weight, dtype=np.float64)
  col = None if colour is None else np.asarray(colour, dtype=np.float64)
  nz, ny, nx = t.shape
  valid = (w > 0) & (w >= f32(min_weight))
  inside = t < 0
  o3 = np.array([f32(x) for x in origin])
  h = f32(voxel_size)
  position = lambda i, j, k: o3 + h * np.array([i, j, k], dtype=np.float64)
  linear = lambda i, j, k: (k * ny + j) * nx + i

  keys, rows, colours = [], [], []
  for e, (dx, dy, dz) in enumerate(DIRECTIONS):
    if nx - dx < 1 or ny - dy < 1 or nz - dz < 1:
      continue
    lo = (slice(0, nz - dz), slice(0, ny - dy), slice(0, nx - dx))
    hi = (slice(dz, nz), slice(dy, ny), slice(dx, nx))
    crossing = valid[lo] & valid[hi] & (inside[lo] != inside[hi])
    for k, j, i in zip(*np.nonzero(crossing)):
      t_o, t_b = t[k, j, i], t[k + dz, j + dy, i + dx]
      lam = t_o / (t_o - t_b)
      p_o, p_b = position(i, j, k), position(i + dx, j + dy, k + dz)
      keys.append(linear(i, j, k) * 7 + e)
      rows.append(p_o + lam * (p_b - p_o))
      if col is not None:
        colours.append(col[k, j, i] + lam * (col[k + dz, j + dy, i + dx] - col[k, j, i]))
  order = np.argsort(np.asarray(keys, dtype=np.int64), kind='stable')
  keys = np.asarray(keys, dtype=np.int64)[order]
  vertices = np.asarray(rows, dtype=np.float64).reshape(-1, 3)[order]
  colours = None if col is None else np.asarray(colours, dtype=np.float64).reshape(-1, 3)[order]
  index_of = {int(key): n for n, key in enumerate(keys)}

  faces = []
  if nx > 1 and ny > 1 and nz > 1:
    cell_valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
    mixed_lo = np.ones_like(cell_valid)
    mixed_hi = np.zeros_like(cell_valid)
    for dz, dy, dx in itertools.product((0, 1), repeat=3):
      part = (slice(dz, nz - 1 + dz), slice(dy, ny - 1 + dy), slice(dx, nx - 1 + dx))
      mixed_lo &= inside[part]
      mixed_hi |= inside[part]
    candidates = np.nonzero(mixed_hi & ~mixed_lo)           # cells whose corners are neither all inside nor all outside
    cells = sorted(zip(*candidates))                         # (k, j, i) ascending = linear order of the lower corner
    for k, j, i in cells:
      for path in TETRAHEDRA:
        corners = [(i + dx, j + dy, k + dz) for dx, dy, dz in path]
        if not all(valid[c[2], c[1], c[0]] for c in corners):
          continue
        ins = [bool(inside[c[2], c[1], c[0]]) for c in corners]
        triangles = tet_triangles(ins)
        if not triangles:
          continue
        pts = [np.array(c, dtype=np.float64) for c in corners]
        outward = (np.mean([pts[v] for v in range(4) if not ins[v]], axis=0)
                   - np.mean([pts[v] for v in range(4) if ins[v]], axis=0))
        for tri in triangles:
          mid = [0.5 * (pts[a] + pts[b]) for a, b in tri]           # the orientation is topological: midpoints decide
          normal = np.cross(mid[1] - mid[0], mid[2] - mid[0])
          ids = []
          for a, b in tri:
            d = tuple(hi_c - lo_c for lo_c, hi_c in zip(path[a], path[b]))
            ids.append(index_of[linear(*corners[a]) * 7 + DIRECTIONS.index(d)])
          if float(normal @ outward) < 0:
            ids[1], ids[2] = ids[2], ids[1]
          faces.append(ids)
  return vertices, np.asarray(faces, dtype=np.int64).reshape(-1, 3), colours


def canonical_faces(faces):
  """each triangle rotated so that its smallest index comes first (the cyclic rotation is free)"""
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  if f.shape[0] == 0:
    return f
  shift = np.argmin(f, axis=1)
  rows = np.arange(f.shape[0])
  return np.stack([f[rows, shift], f[rows, (shift + 1) % 3], f[rows, (shift + 2) % 3]], axis=1)


# ---- mesh statistics ---------------------------------------------------------------------------------------------------

def directed_edges(faces):
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  return np.concatenate([f[:, [0, 1]], f[:, [1, 2]], f[:, [2, 0]]], axis=0)


def directed_edge_multiplicities(faces):
  """counts of every directed edge (a, b) that occurs"""
  e = directed_edges(faces)
  if e.shape[0] == 0:
    return np.zeros((0,), dtype=np.int64)
  return np.unique(e, axis=0, return_counts=True)[1]


def undirected_edges(faces):
  """``(edges (E, 2) with a < b, counts (E,))``"""
  e = np.sort(directed_edges(faces), axis=1)
  if e.shape[0] == 0:
    return e, np.zeros((0,), dtype=np.int64)
  return np.unique(e, axis=0, return_counts=True)


def euler_characteristic(faces):
  """V - E + F over the vertices the faces use"""
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  return int(np.unique(f).size - undirected_edges(f)[0].shape[0] + f.shape[0])


def signed_volume(vertices, faces):
  """sum a . (b x c) / 6: the enclosed volume of a closed mesh whose normals point outwards"""
  v = np.asarray(vertices, dtype=np.float64)
  f = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  a, b, c = v[f[:, 0]], v[f[:, 1]], v[f[:, 2]]
  return float(np.einsum('ij,ij->i', a, np.cross(b, c)).sum() / 6.0)


# ---- analytic fields ---------------------------------------------------------------------------------------------------

def grid_positions(origin, voxel_size, dims):
  """(nz, ny, nx, 3) float64 sample positions from the float32 origin and voxel size"""
  nx, ny, nz = dims
  h = f32(voxel_size)
  axes = [f32(origin[a]) + h * np.arange(n, dtype=np.float64) for a, n in enumerate((nx, ny, nz))]
  z, y, x = np.meshgrid(axes[2], axes[1], axes[0], indexing='ij')
  return np.stack([x, y, z], axis=-1)


def sphere_field(positions, centre, radius):
  return np.linalg.norm(positions - np.asarray(centre, dtype=np.float64), axis=-1) - radius


def torus_field(positions, centre, major, minor):
  q = positions - np.asarray(centre, dtype=np.float64)
  return np.sqrt((np.sqrt(q[..., 0] ** 2 + q[..., 1] ** 2) - major) ** 2 + q[..., 2] ** 2) - minor


def all_sign_patterns():
  """``(tsdf, weight)`` (3, 48, 48) float32: the 256 inside / outside patterns of a cell's 8 corners, cell c at
  (3 (c % 16), 3 (c // 16), 0), separated by samples of weight 0.  Magnitudes vary per corner so that no two vertices
  coincide."""
  tsdf = np.ones((3, 48, 48), dtype=np.float32)
  weight = np.zeros((3, 48, 48), dtype=np.float32)
  for c in range(256):
    i0, j0 = 3 * (c % 16), 3 * (c // 16)
    for corner in range(8):
      dx, dy, dz = corner & 1, corner >> 1 & 1, corner >> 2
      magnitude = 0.25 + 0.09 * corner + 0.001 * (c % 7)
      tsdf[dz, j0 + dy, i0 + dx] = -magnitude if c >> corner & 1 else magnitude
      weight[dz, j0 + dy, i0 + dx] = 1.0 + corner
  return tsdf, weight


# ---- integration cases (tests/test_gpu_tsdf.py) ------------------------------------------------------------------------

def integration_case(dims, size, count, truncation=0.2, weighted=True, coloured=True, seed=0):
  """Deterministic inputs of one integration case: a volume whose longest side spans 1.6 units, ``count`` generic cameras
  (rotated, rolled, off-centre principal point, fx != fy) on a perturbed circle of radius about 2.5 around it, and
  ``size`` = (W, H) images.  Camera 1 sits inside the volume (samples behind it), every third camera has a near plane
  inside the volume and every third a far plane inside it, the odd ones a focal length that leaves part of the volume
  outside the image.  Depth holds holes (0, NaN, inf, a negative value); pixel weights hold exact zeros and a negative
  value.  Returns a dict of CPU tensors and numbers."""
  width, height = size
  nx, ny, nz = dims
  voxel = f32(1.6 / max(dims))
  origin = tuple(f32(x) for x in (-0.41 - 0.5 * voxel * (nx - 1) + 0.4, -0.33 - 0.5 * voxel * (ny - 1) + 0.3,
                                  0.27 - 0.5 * voxel * (nz - 1)))
  centre = np.array([origin[a] + 0.5 * voxel * (n - 1) for a, n in enumerate(dims)])
  rows = []
  for c in range(count):
    angle, elevation = 0.7 + 2.399 * c, 0.35 * math.sin(1.1 * c + 0.2)
    radius = 2.5 + 0.3 * math.cos(1.7 * c)
    eye = centre + radius * np.array([math.cos(elevation) * math.cos(angle), math.sin(elevation), math.cos(elevation) * math.sin(angle)])
    target = centre + 0.2 * np.array([math.sin(1.3 * c), math.cos(0.9 * c), math.sin(0.4 * c + 1.0)])
    if c == 1:
      eye = centre + np.array([0.11, -0.07, 0.05])
    fx = (1.6 if c % 2 else 0.9) * width * (1.0 + 0.2 * math.sin(c))
    near = 2.3 if c % 3 == 0 and c != 1 else 0.3
    far = 2.7 if c % 3 == 1 and c != 1 else 10.0
    rows.append(pack_camera(look_at(eye, target, roll=0.4 + 0.37 * c), fx, 1.07 * fx, 0.5 * width + 0.3, 0.5 * height - 0.2,
                            near, far, width, height))
  cameras = torch.stack(rows)
  cc, yy, xx = torch.meshgrid(torch.arange(count), torch.arange(height), torch.arange(width), indexing='ij')
  depth = (2.5 + 0.25 * torch.sin(0.9 * xx + 0.4 * cc) * torch.cos(0.7 * yy) + 0.15 * torch.sin(0.31 * (xx + yy) + cc)).to(torch.float32)
  key = xx * 7 + yy * 3 + cc
  depth[key % 11 == 0] = 0.0
  depth[key % 13 == 1] = float('nan')
  depth[key % 17 == 2] = float('inf')
  depth[key % 19 == 3] = -1.0
  generator = torch.Generator().manual_seed(seed)
  pixel_weight = None
  if weighted:
    pixel_weight = (0.5 + ((xx * 3 + yy * 5 + cc * 2) % 5) / 4.0).to(torch.float32)
    pixel_weight[(xx + 2 * yy + cc) % 7 == 0] = 0.0
    pixel_weight[(xx + 2 * yy + cc) % 23 == 1] = -0.5
  image = torch.rand((count, height, width, 3), generator=generator) if coloured else None
  return dict(dims=dims, origin=origin, voxel_size=voxel, truncation=f32(truncation), cameras=cameras, depth=depth,
              pixel_weight=pixel_weight, image=image, size=size)
