"""face_area_cdf / sample_mesh_points / surface_distances / surface_metrics / evaluate_mesh on the GPU against the numpy
oracle of tests/mesh_sample_oracle.py (the sampler's rules restated) and the float64 brute force of
tests/nearest_oracle.py.  The meshes are those of tests/mesh_oracle.py plus three small ones built here: faces of zero
area first and last, one triangle, and strips of 63 / 64 / 65 faces (a wave of the area kernel); n sits around one
sample, a wave, and 10 007 (40 workgroups, the last one partial).

What is compared how.  Faces and barycentric weights: bit for bit with the kernel's operations restated in numpy ON THE
DEVICE'S cdf (float64 strata and search, float32 weights; sqrt is correctly rounded on both sides).  Points: bit for bit
with the float32 expression (wa A + wb B) + wc C, and within 4 ulp of the largest vertex coordinate of the float64
combination (three products and two sums, each rounded once, of terms no larger than that coordinate: 2.5 ulp).
Stratification is exact: sample i lies in the i-th of n equal shares of the cdf, so a face spanning x shares meets fewer
than x + 2 of them and contains more than x - 2.
"""
import math

import numpy as np
import pytest
import torch

from taichi_splatting_amd import (TriangleMesh, evaluate_mesh, face_area_cdf, metrics_from_distances, sample_mesh_points,
                                  surface_distances, surface_metrics)
from tests import mesh_oracle as mo
from tests import mesh_sample_oracle as so
from tests import nearest_oracle as no

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'


def zero_area_first_and_last():
  vertices = np.array([[0, 0, 0], [2, 0, 0], [0, 1, 0], [4, 0, 0], [0, 0, 3], [1, 1, 1]], dtype=np.float32)
  faces = np.array([[0, 0, 1],           # two corners on one vertex
                    [0, 1, 2], [5, 5, 5], [0, 2, 4], [1, 2, 4],
                    [0, 1, 3]],          # three points on a line
                   dtype=np.int32)
  return vertices, faces


def one_triangle():
  return np.array([[1, 2, 3], [4, 2.5, 3], [1.5, 6, -2]], dtype=np.float32), np.array([[0, 1, 2]], dtype=np.int32)


MESHES = {
  'sphere': lambda: mo.analytic_mesh('sphere'),
  'strip 1000': lambda: mo.strip(1000, seed=2),
  'fan 200': lambda: mo.fan(200, hub_last=True, seed=3),
  'soup': lambda: mo.soup(40, 300, 25, seed=4),
  'zero-area faces first and last': zero_area_first_and_last,
  'one triangle': one_triangle,
  'strip 63': lambda: mo.strip(63, seed=5),
  'strip 64': lambda: mo.strip(64, seed=6),
  'strip 65': lambda: mo.strip(65, seed=7),
}
COUNTS = (1, 2, 63, 64, 65, 10_007)

_cache = {}


def mesh_of(name):
  """(vertices, faces as numpy; the TriangleMesh on the GPU with colours and normals): made once, never written to"""
  if name not in _cache:
    vertices, faces = MESHES[name]()
    vertices, faces = np.ascontiguousarray(vertices, dtype=np.float32), np.ascontiguousarray(faces, dtype=np.int32)
    rng = np.random.default_rng(len(name))
    colours = rng.uniform(0.0, 1.0, size=vertices.shape).astype(np.float32)
    normals = rng.standard_normal(size=vertices.shape).astype(np.float32)
    mesh = TriangleMesh(vertices=torch.from_numpy(vertices).to(DEV), faces=torch.from_numpy(faces).to(DEV),
                        colours=torch.from_numpy(colours).to(DEV), normals=torch.from_numpy(normals).to(DEV))
    _cache[name] = (vertices, faces, colours, normals, mesh)
  return _cache[name]


def same_bits(got, want):
  got = got.detach().cpu().numpy() if isinstance(got, torch.Tensor) else got
  return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got.view(np.uint32), want.view(np.uint32))


@pytest.mark.parametrize('name', sorted(MESHES))
def test_face_area_cdf(name):
  vertices, faces, _, _, mesh = mesh_of(name)
  cdf = face_area_cdf(mesh)
  assert cdf.shape == (faces.shape[0],) and cdf.dtype == torch.float64
  want = np.cumsum(so.face_areas(vertices, faces))
  np.testing.assert_allclose(cdf.cpu().numpy(), want, rtol=1e-12, atol=0.0)
  assert torch.equal(face_area_cdf(mesh), cdf)


@pytest.mark.parametrize('name', sorted(MESHES))
def test_samples_against_the_oracle(name):
  vertices, faces, colours, normals, mesh = mesh_of(name)
  cdf = face_area_cdf(mesh).cpu().numpy()
  areas = np.diff(cdf, prepend=0.0)
  ulp = float(np.spacing(np.abs(vertices).max()))
  for n in COUNTS:
    seed = 11 + n
    s = sample_mesh_points(mesh, n, seed=seed, return_faces=True, return_barycentric=True)
    label = f"{name}, n = {n}"
    assert s.points.shape == (n, 3) and s.points.dtype == torch.float32 and s.faces.dtype == torch.int32, label
    want_face, want_w = so.restate(cdf, n, seed)
    face = s.faces.cpu().numpy()
    assert np.array_equal(face, want_face), f"{label}: faces differ from searchsorted(cdf, t, 'right')"
    assert (areas[face] > 0).all(), f"{label}: a face of zero area was drawn"
    assert same_bits(s.barycentric, want_w), f"{label}: barycentric weights differ bitwise"
    w = s.barycentric.cpu().numpy()
    assert (w >= 0).all() and np.abs(w.astype(np.float64).sum(axis=1) - 1.0).max() <= 2.0 ** -23, label
    points = s.points.cpu().numpy()
    exact = so.sample(vertices, faces, cdf, n, seed)[0]
    worst = np.abs(points - exact).max() / ulp
    assert worst <= 4.0, f"{label}: a point is {worst:.2f} ulp of the largest coordinate from the float64 oracle (allowed 4)"
    assert same_bits(points, so.combine_f32(vertices, faces, face, w)), f"{label}: points differ from the float32 expression"
    assert same_bits(s.colours, so.combine_f32(colours, faces, face, w)), f"{label}: colours"
    assert same_bits(s.normals, so.combine_f32(normals, faces, face, w)), f"{label}: normals (not renormalised)"
    # stratification, exact
    count = np.bincount(face, minlength=faces.shape[0])
    assert (np.abs(count - n * areas / cdf[-1]) < 2).all(), f"{label}: a face's sample count is 2 or more from n area / A"
    # the optional outputs do not change the others; two calls give equal bits; another seed, other points
    plain = sample_mesh_points(mesh, n, seed=seed)
    assert plain.faces is None and plain.barycentric is None
    assert torch.equal(plain.points, s.points) and torch.equal(plain.colours, s.colours) and torch.equal(plain.normals, s.normals)
    assert not torch.equal(sample_mesh_points(mesh, n, seed=seed + 1).points, s.points), label


def test_seed_is_taken_modulo_2_32_and_defaults_to_zero():
  mesh = mesh_of('fan 200')[4]
  base = sample_mesh_points(mesh, 500).points
  assert torch.equal(sample_mesh_points(mesh, 500, seed=0).points, base)
  assert torch.equal(sample_mesh_points(mesh, 500, seed=2 ** 32).points, base)
  assert torch.equal(sample_mesh_points(mesh, 500, seed=-1).points, sample_mesh_points(mesh, 500, seed=2 ** 32 - 1).points)


def test_density():
  vertices, faces, _, _, mesh = mesh_of('sphere')
  area = float(face_area_cdf(mesh)[-1])
  for density in (0.37, 25.0, 1.0 / area, 0.5 / area):
    s = sample_mesh_points(mesh, density=density)
    assert s.points.shape[0] == math.ceil(density * area), density
  assert torch.equal(sample_mesh_points(mesh, density=25.0, seed=3).points,
                     sample_mesh_points(mesh, math.ceil(25.0 * area), seed=3).points)


@pytest.mark.parametrize('name', ('sphere', 'zero-area faces first and last', 'one triangle'))
def test_face_normals(name):
  vertices, faces, _, _, mesh = mesh_of(name)
  s = sample_mesh_points(mesh, 3000, seed=1, return_faces=True, face_normals=True)
  face = s.faces.cpu().numpy()
  want = so.face_unit_normals(vertices, faces)[face]
  got = s.normals.cpu().numpy().astype(np.float64)
  assert np.abs(got - want).max() <= 2.0 ** -24                           # float64 rounded once: half an ulp of a value <= 1
  assert np.abs(np.linalg.norm(got, axis=1) - 1.0).max() <= 2.0 ** -22
  # mesh_oracle.unit_normals on the face alone: its three vertices carry the face's own term
  for f in np.unique(face)[:20]:
    alone = mo.unit_normals(vertices, faces[f:f + 1])[faces[f, 0]]
    assert np.abs(got[face == f] - alone).max() <= 2.0 ** -24
  bare = TriangleMesh(vertices=mesh.vertices, faces=mesh.faces)
  assert sample_mesh_points(bare, 100).normals is None and sample_mesh_points(bare, 100).colours is None
  assert torch.equal(sample_mesh_points(bare, 3000, seed=1, face_normals=True).normals, s.normals)


def test_meshes_that_cannot_be_sampled():
  vertices, faces, _, _, mesh = mesh_of('strip 64')
  v, f = mesh.vertices, mesh.faces
  with pytest.raises(ValueError, match="no faces"):
    sample_mesh_points(TriangleMesh(vertices=v, faces=f[:0]), 10)
  flat = torch.tensor([[0, 1, 2], [1, 1, 1]], dtype=torch.int32, device=DEV)
  line = torch.tensor([[0.0, 0, 0], [1, 1, 1], [2, 2, 2]], device=DEV)
  with pytest.raises(ValueError, match="total area"):
    sample_mesh_points(TriangleMesh(vertices=line, faces=flat), 10)
  for bad in (-1, v.shape[0]):
    broken = f.clone()
    broken[17, 1] = bad
    with pytest.raises(ValueError, match="outside 0"):
      sample_mesh_points(TriangleMesh(vertices=v, faces=broken), 10)
  for value in (math.nan, math.inf):
    poisoned = v.clone()
    poisoned[int(faces[30, 2]), 1] = value
    with pytest.raises(ValueError, match="not finite"):
      sample_mesh_points(TriangleMesh(vertices=poisoned, faces=f), 10)
  loose = torch.cat([v, torch.full((1, 3), math.nan, device=DEV)])        # a NaN no face references is legal
  assert torch.equal(sample_mesh_points(TriangleMesh(vertices=loose, faces=f), 10).points, sample_mesh_points(mesh, 10).points)
  for kw in (dict(), dict(n=10, density=1.0), dict(n=0)):
    with pytest.raises(ValueError):
      sample_mesh_points(mesh, **kw)
  with pytest.raises(ValueError, match="empty"):
    surface_distances(v, v[:0])


# ---- distances and metrics ------------------------------------------------------------------------------------------------

def brute_distances(a, b):
  """float64 (d_ab, d_ba) on the device"""
  return torch.sqrt(no.cross(a, b, 1)[0][:, 0]), torch.sqrt(no.cross(b, a, 1)[0][:, 0])


@pytest.mark.parametrize('name', sorted(MESHES))
def test_surface_distances_and_metrics(name):
  mesh = mesh_of(name)[4]
  a = sample_mesh_points(mesh, 4001, seed=1).points
  b = sample_mesh_points(mesh, 2503, seed=2).points + torch.tensor([0.01, -0.02, 0.005], device=DEV)
  d_ab, d_ba = surface_distances(a, b)
  assert d_ab.shape == (4001,) and d_ba.shape == (2503,) and d_ab.dtype == torch.float32
  for got, want in zip((d_ab, d_ba), brute_distances(a, b)):
    assert bool(((got.double() - want).abs() <= 4 * 2.0 ** -24 * want).all()), f"{name}: beyond 4 x 2^-24 of the float64 brute force"
  smallest, largest = float(min(d_ab.min(), d_ba.min())), float(max(d_ab.max(), d_ba.max()))
  assert smallest > 0
  m = surface_metrics(a, b, threshold=0.5 * (smallest + largest), max_distance=largest)
  by_hand = metrics_from_distances(d_ab, d_ba, 0.5 * (smallest + largest), largest)
  assert m == by_hand and m.dropped_a == 0.0 and m.dropped_b == 0.0
  assert m.accuracy == float(d_ab.double().sum()) / 4001 and m.completeness == float(d_ba.double().sum()) / 2503
  assert m.chamfer == (m.accuracy + m.completeness) / 2
  above = surface_metrics(a, b, threshold=float(np.nextafter(np.float32(largest), np.float32(np.inf))))
  assert (above.precision, above.recall, above.fscore) == (1.0, 1.0, 1.0)
  below = surface_metrics(a, b, threshold=float(np.nextafter(np.float32(smallest), np.float32(0.0))))
  assert (below.precision, below.recall, below.fscore) == (0.0, 0.0, 0.0)
  assert (below.accuracy, below.completeness) == (above.accuracy, above.completeness)      # the threshold does not touch the means
  # evaluate_mesh = the three calls made by hand, bit for bit
  e = evaluate_mesh(mesh, b, 0.02, n=4001, seed=1, max_distance=0.75 * largest)
  assert e == metrics_from_distances(d_ab, d_ba, 0.02, 0.75 * largest)
  area = float(face_area_cdf(mesh)[-1])
  assert evaluate_mesh(mesh, b, 0.02, density=4000.5 / area, seed=1, max_distance=0.75 * largest) == e


def test_a_sphere_against_a_larger_sphere():
  """Samples A of the analytic sphere mesh (radius R) against points B on the sphere of radius R + 0.05 about the same
  centre c.  With rho(x) = |x - c| and h = max over A of |rho(a) - R| (the mesh's chord and interpolation error, from
  the float64 oracle samples): every pair is at least (R + 0.05) - rho(a) >= 0.05 - h apart, which bounds both means
  from below.  From above, let B' be B pulled radially onto the sphere of radius R, so that |b - b'| = 0.05: then
  d(a, B) <= d(a, B') + 0.05 and d(b, A) <= 0.05 + d(b', A) by the triangle inequality, so
  accuracy <= 0.05 + s_B and completeness <= 0.05 + s_A with s_B = max over A of d(a, B') and s_A = max over B' of
  d(b', A): the covering radius of the other set, by the float64 brute force.  B is rounded to float32, so |b - b'| is
  0.05 to within its own rounding, measured below (`gap`) and used as it is.  No constant is guessed."""
  vertices, faces, _, _, mesh = mesh_of('sphere')
  radius, centre, offset = mo.SPHERE_RADIUS, mo.CENTRE, 0.05
  n = 10_007
  a = sample_mesh_points(mesh, n, seed=5).points
  exact = so.sample(vertices, faces, face_area_cdf(mesh).cpu().numpy(), n, 5)[0]
  h = float(np.abs(np.linalg.norm(exact - centre, axis=1) - radius).max())
  h += float(np.abs(a.cpu().numpy() - exact).max()) * math.sqrt(3.0)        # the float32 samples against the oracle's

  count = 20_000                                                              # a Fibonacci lattice on the larger sphere
  k = np.arange(count) + 0.5
  polar, azimuth = np.arccos(1.0 - 2.0 * k / count), math.pi * (1.0 + math.sqrt(5.0)) * k
  unit = np.stack([np.sin(polar) * np.cos(azimuth), np.sin(polar) * np.sin(azimuth), np.cos(polar)], axis=1)
  b_host = (centre + (radius + offset) * unit).astype(np.float32)
  b = torch.from_numpy(b_host).to(DEV)
  radial = b_host.astype(np.float64) - centre
  rho = np.linalg.norm(radial, axis=1, keepdims=True)
  pulled = torch.from_numpy(centre + radial * (radius / rho)).to(DEV)         # B', float64
  gap = np.abs(rho - radius)
  assert np.abs(gap - offset).max() <= 1e-6

  s_b = float(torch.sqrt(no.cross(a.double(), pulled, 1)[0]).max())
  s_a = float(torch.sqrt(no.cross(pulled, a.double(), 1)[0]).max())
  m = surface_metrics(a, b, threshold=offset)
  print(f"h = {h:.5f}, s_B = {s_b:.5f}, s_A = {s_a:.5f}; accuracy {m.accuracy:.5f}, completeness {m.completeness:.5f}, "
        f"chamfer {m.chamfer:.5f}, precision {m.precision:.3f}, recall {m.recall:.3f}, F {m.fscore:.3f}")
  assert float(gap.min()) - h <= m.accuracy <= float(gap.max()) + s_b
  assert float(gap.min()) - h <= m.completeness <= float(gap.max()) + s_a
  assert m.chamfer == (m.accuracy + m.completeness) / 2
  # every distance is at least 0.05 - h and at most 0.05 + s: the thresholds on either side decide everything
  assert surface_metrics(a, b, threshold=float(gap.min()) - h - 1e-6).fscore == 0.0
  assert surface_metrics(a, b, threshold=float(gap.max()) + max(s_a, s_b)).fscore == 1.0
  e = evaluate_mesh(mesh, b, offset, n=n, seed=5)
  assert e == m
