"""``simplify_mesh`` on the GPU (taichi_splatting_amd/mesh.py, csrc/mesh_simplify.hip) against the numpy oracle of
tests/mesh_simplify_oracle.py.

Clusters, faces, the vertex count and ``vertex_map`` are compared EXACTLY: the cell rule is three IEEE float32 operations
that numpy reproduces bit for bit, and everything downstream of it is integer work.

Positions and colours: the kernel and the oracle each round ONE float64 value to float32.  The oracle's docstring derives
``error_bound``, a bound on the error of a float64 evaluation of the position; every case below ASSERTS that it is under
a quarter of the float32 spacing at the cell's coordinate magnitude (``cell_ulp``), so the two float64 values lie within
half a spacing of each other and their roundings are the same or adjacent floats: every coordinate is held to 1 ``cell_ulp``.
A cluster whose unrounded optimum lies within 1e-4 of a cell of a cell face may pass the in-cell test in one evaluation
and fail it in the other: for those either of the oracle's two positions is accepted, and their share is capped at 1 %
(the two sphere cases have none: the closest is 1.6e-3, tests/test_mesh_simplify_host.py).

Sizes: 63, 64, 65 and 257 vertices in one row of cells (the wave and workgroup edges of the one-lane-per-vertex kernels), a
fan whose hub cluster has 3000 corners (188 rounds of the 16 lanes that share a cluster), clusters of one vertex, a
cluster whose faces all have zero area, vertices exactly on cell faces, and a 32^3 field extracted on the device.
"""
import functools

import numpy as np
import pytest
import torch

from taichi_splatting_amd import TSDFVolume, TriangleMesh, simplify_mesh, with_vertex_normals
from taichi_splatting_amd import mesh as tm
from tests import mesh_simplify_oracle as so

pytestmark = pytest.mark.gpu
DEVICE = 'cuda:0'
SPHERE_ORIGIN = (-1.01, -1.02, -1.03)
CUBE_ORIGIN = (-0.02, -0.02, -0.02)


def bits(t):
  return t.contiguous().view(torch.int32)


def on_device(vertices, faces, colours=None):
  move = lambda a, dtype: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEVICE)
  return TriangleMesh(vertices=move(vertices, torch.float32).reshape(-1, 3), faces=move(faces, torch.int32).reshape(-1, 3),
                      colours=move(colours, torch.float32))


def kept_clusters(cluster_scan):
  """(K,) bool from the selection's scan over the clusters: the cluster still has a face, i.e. is an output vertex"""
  return cluster_scan[1:] != cluster_scan[:-1]


def signed_zeros():
  """642 vertices = one workgroup of the origin kernel, lane t of which walks the vertices t, t + 256, t + 512: wave 0 holds
  the vertices with v % 256 < 64.  x: wave 0 sees -0 and non-negative values only, the negative values are in the other
  waves' shares — the minimum is the most negative one.  y: no negative value, a -0 in wave 0 and a +0 in wave 1 — the
  minimum is -0, by its bits.  z: +0 in wave 2 and otherwise positive — the minimum is +0."""
  vertices, faces = so.icosphere(3)
  vertices = vertices.copy()
  share = np.arange(vertices.shape[0]) % 256
  vertices[share < 64, 0] = np.abs(vertices[share < 64, 0])
  vertices[0, 0] = -0.0
  vertices[:, 1] = np.abs(vertices[:, 1]) + np.float32(0.125)
  vertices[1, 1], vertices[70, 1] = -0.0, 0.0
  vertices[:, 2] = np.abs(vertices[:, 2]) + np.float32(0.125)
  vertices[130, 2] = 0.0
  return vertices, faces


def colours_of(vertices):
  return np.random.default_rng(vertices.shape[0]).uniform(0.1, 1.0, size=vertices.shape).astype(np.float32)


def row_strip(count):
  """``count`` vertices in ONE row of unit cells, one or two to a cell, joined into a strip: some faces span three cells"""
  i = np.arange(count)
  vertices = np.stack([0.6 * i + 0.1, 0.25 + 0.5 * (i % 2), np.full(count, 0.5) + 0.01 * (i % 3)], axis=1).astype(np.float32)
  faces = np.stack([i[:-2], i[1:-1], i[2:]], axis=1).astype(np.int32)
  faces[1::2] = faces[1::2][:, [1, 0, 2]]
  return vertices, faces


def cone_fan(rim, radius=3.0):
  """a hub raised above a rim of ``rim`` vertices, two more vertices in the hub's cell: the hub's cluster has 3 members
  and ``rim`` + 3 corners, and keeps the faces whose two rim vertices fall into different cells"""
  angle = 2.0 * np.pi * np.arange(rim) / rim
  ring = np.stack([4.5 + radius * np.cos(angle), 4.5 + radius * np.sin(angle), np.full(rim, 0.5)], axis=1)
  hub = [(4.5, 4.5, 1.5), (4.25, 4.75, 1.25), (4.75, 4.25, 1.75)]
  vertices = np.concatenate([hub, ring]).astype(np.float32)
  i = np.arange(rim)
  faces = np.stack([np.zeros(rim, dtype=np.int64), 3 + i, 3 + (i + 1) % rim], axis=1)
  extra = [(1, 3, 3 + rim // 3), (2, 3 + rim // 3, 3 + 2 * rim // 3), (1, 2, 3 + rim // 2)]
  return vertices, np.concatenate([faces, extra]).astype(np.int32)


def collinear():
  """two vertices in each of three cells, all on one line: every face has zero area, trace(A) = 0, the mean is used"""
  x = np.array([0.25, 0.5, 1.25, 1.75, 2.5, 2.875])
  vertices = np.stack([x, np.full(6, 0.5), np.full(6, 0.5)], axis=1).astype(np.float32)
  return vertices, np.array([(0, 2, 4), (1, 3, 5), (0, 3, 4)], dtype=np.int32)


def with_loose_vertices(vertices, faces):
  """every third slot a vertex no face references — one of them not even finite"""
  count = vertices.shape[0]
  slots = np.arange(count) + np.arange(count) // 2 + 1
  padded = np.random.default_rng(3).uniform(-1, 1, size=(int(slots[-1]) + 2, 3)).astype(np.float32)
  padded[0] = np.nan
  padded[slots] = vertices
  return padded, slots[faces].astype(np.int32)


def hand_case():
  vertices = np.array([(0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.0, 0.5), (0.5, 0.5, 1.5), (9, 9, 9)], dtype=np.float32)
  faces = np.array([(2, 3, 0), (1, 2, 3), (3, 2, 1), (0, 1, 2), (4, 3, 2), (3, 1, 2)], dtype=np.int32)
  return vertices, faces


def tetrahedron():
  vertices = np.array([(0.1, 0.1, 0.1), (0.9, 0.1, 0.1), (0.1, 0.9, 0.1), (0.1, 0.1, 0.9)], dtype=np.float32)
  return vertices, np.array([(0, 2, 1), (0, 1, 3), (1, 2, 3), (0, 3, 2)], dtype=np.int32)


def no_mesh(num_vertices):
  return np.full((num_vertices, 3), 0.5, dtype=np.float32), np.zeros((0, 3), dtype=np.int32)


# name -> (mesh builder, cell_size, origin)
CASES = {
  'sphere_0.25': (lambda: so.icosphere(4), 0.25, SPHERE_ORIGIN),
  'sphere_0.20': (lambda: so.icosphere(4), 0.20, SPHERE_ORIGIN),
  'cube': (lambda: so.cube_surface(12), 0.26, CUBE_ORIGIN),
  'row_63': (lambda: row_strip(63), 1.0, (0, 0, 0)),
  'row_64': (lambda: row_strip(64), 1.0, (0, 0, 0)),
  'row_65': (lambda: row_strip(65), 1.0, (0, 0, 0)),
  'row_257': (lambda: row_strip(257), 1.0, (0, 0, 0)),
  'on_cell_faces': (lambda: so.cube_surface(8), 0.25, (0, 0, 0)),      # i / 8: every second lattice plane IS a cell face
  'loose_vertices': (lambda: with_loose_vertices(*so.icosphere(3)), 0.25, SPHERE_ORIGIN),
  'duplicates': (hand_case, 1.0, (0, 0, 0)),
  'tetrahedron_in_one_cell': (tetrahedron, 1.0, (0, 0, 0)),
  'fan_of_3000': (lambda: cone_fan(3000), 1.0, (0, 0, 0)),
  'collinear': (collinear, 1.0, (0, 0, 0)),
  'default_origin': (lambda: so.icosphere(3), 0.3, None),
  'default_origin_positive': (lambda: row_strip(257), 1.0, None),      # no negative coordinate: the other branch of the minimum
  'default_origin_signed_zeros': (signed_zeros, 0.3, None),
  'no_faces': (lambda: no_mesh(5), 1.0, None),
  'nothing': (lambda: no_mesh(0), 1.0, None),
}


# The faces of this cube lie IN cell faces: the optimum of a flat cluster is on the face itself, its side a matter of the
# last bit; and vertex 3 of the hand case is the only member of its cluster and lies on a cell face, so its optimum — the
# vertex itself — does too; and with the default origin the lowest vertex of a convex shape lies ON the lowest cell face,
# where the tangent plane that its cluster's optimum sits on coincides with that face.  These cases are there for the cell
# and face rules (integers); the in-cell property is checked on two of them further down.
EXACT_ONLY = ('on_cell_faces', 'duplicates', 'default_origin', 'default_origin_positive', 'default_origin_signed_zeros')


@functools.lru_cache(maxsize=None)
def case(name):
  """(vertices, faces, colours, cell_size, origin, the oracle's result): computed once, not modified"""
  build, cell_size, origin = CASES[name]
  vertices, faces = build()
  colours = colours_of(vertices)
  return vertices, faces, colours, cell_size, origin, so.simplify(vertices, faces, cell_size, origin, colours=colours)


def compare(got, vertex_map, choice, want, what):
  """integers exactly; positions and colours under the module docstring's criterion; returns the number of flip candidates"""
  assert got.normals is None
  assert got.vertices.shape[0] == want['vertices'].shape[0], what
  assert np.array_equal(got.faces.cpu().numpy(), want['faces']), what
  assert np.array_equal(vertex_map.cpu().numpy(), want['vertex_map']), what
  count = want['vertices'].shape[0]
  if count == 0 or what in EXACT_ONLY:
    return 0
  ulp = want['cell_ulp'].astype(np.float64)
  assert (want['error_bound'][:, None] < 0.25 * ulp).all(), (what, float((want['error_bound'][:, None] / ulp).max()))
  positions = got.vertices.cpu().numpy()
  choice = choice.cpu().numpy()
  flip = np.abs(want['margin']) < so.FLIP_MARGIN                          # NaN (no quadric at all): never a candidate
  assert flip.mean() <= 0.01, (what, int(flip.sum()), count)
  near = lambda a, b: (np.abs(a.astype(np.float64) - b.astype(np.float64)) <= ulp).all(axis=1)
  sure = ~flip
  assert np.array_equal(choice[sure], want['choice'][sure]), what
  assert near(positions, want['vertices'])[sure].all(), (what, float((np.abs(positions - want['vertices'])[sure] / ulp[sure]).max()))
  member = sure & (want['choice'] == so.MEMBER)
  assert np.array_equal(positions[member].view(np.int32), want['vertices'][member].view(np.int32)), what
  either = near(positions, want['quadric']) | near(positions, want['mean'])
  assert either[flip].all(), what
  colours = got.colours.cpu().numpy()
  assert (np.abs(colours.astype(np.float64) - want['colours']) <= np.spacing(want['colours'])).all(), what
  return int(flip.sum())


def run(name, placement='quadric'):
  vertices, faces, colours, cell_size, origin, _ = case(name)
  return tm._simplify(on_device(vertices, faces, colours), cell_size, origin, placement, 1e-3)


@pytest.mark.parametrize('name', sorted(CASES))
def test_against_the_oracle(name):
  vertices, faces, colours, cell_size, origin, want = case(name)
  mesh = on_device(vertices, faces, colours)
  before = [bits(mesh.vertices).clone(), mesh.faces.clone(), bits(mesh.colours).clone()]
  got, vertex_map, used_origin, choice, scan = tm._simplify(mesh, cell_size, origin, 'quadric', 1e-3)
  assert np.array_equal(used_origin.cpu().numpy().view(np.int32), want['origin'].view(np.int32))       # bit for bit
  flips = compare(got, vertex_map, choice[kept_clusters(scan)], want, name)
  assert torch.equal(bits(mesh.vertices), before[0]) and torch.equal(mesh.faces, before[1]) and torch.equal(bits(mesh.colours), before[2])
  if name.startswith('sphere') or name == 'cube':
    assert flips == 0
  # the public call: the same tensors, with and without the map
  plain = simplify_mesh(mesh, cell_size, origin)
  pair = simplify_mesh(mesh, cell_size, origin=origin, return_map=True)
  assert isinstance(plain, TriangleMesh) and isinstance(pair, tuple) and pair[1].dtype == torch.int32
  for other in (plain, pair[0]):
    assert torch.equal(bits(other.vertices), bits(got.vertices)) and torch.equal(other.faces, got.faces)
    assert torch.equal(bits(other.colours), bits(got.colours))
  assert torch.equal(pair[1], vertex_map)


def test_the_cases_are_what_their_names_say():
  expected = {'sphere_0.25': (276, 550), 'sphere_0.20': (401, 810), 'cube': (56, 108), 'tetrahedron_in_one_cell': (0, 0),
              'duplicates': (4, 3), 'no_faces': (0, 0), 'nothing': (0, 0)}
  for name, (num_vertices, num_faces) in expected.items():
    want = case(name)[5]
    assert (want['vertices'].shape[0], want['faces'].shape[0]) == (num_vertices, num_faces), name
  assert case('duplicates')[5]['faces'].tolist() == [[0, 1, 2], [0, 2, 1], [1, 3, 2]]
  fan = case('fan_of_3000')[5]
  assert fan['corners'].max() == 3004 and fan['members'][fan['corners'].argmax()] == 3
  assert fan['choice'][fan['corners'].argmax()] == so.QUADRIC
  line = case('collinear')[5]
  assert (line['choice'] == so.MEAN).all() and np.isnan(line['margin']).all() and line['vertices'].shape[0] == 3
  for count in (63, 64, 65, 257):
    vertices, faces, _, _, _, want = case(f'row_{count}')
    assert np.unique(faces).shape[0] == count and (want['cell'][:, 1:] == 0).all()      # one row of cells
    assert 0 < want['faces'].shape[0] < faces.shape[0] and (want['members'] == 2).any() and (want['members'] == 1).any()
  vertices, _, _, cell_size, origin, want = case('on_cell_faces')
  exact = (vertices.astype(np.float64) / cell_size) % 1 == 0
  assert exact.any(axis=1).mean() > 0.5 and want['cell'].max() == 4                     # 1.0 lies in the upper cell 4
  assert (case('loose_vertices')[5]['vertex_map'] == -1).sum() >= case('loose_vertices')[0].shape[0] // 3
  assert np.isnan(case('loose_vertices')[0][0]).all()
  vertices, _, _, _, _, want = case('default_origin_signed_zeros')
  share = np.arange(vertices.shape[0]) % 256
  assert (vertices[share < 64, 0] >= 0).all() and np.signbit(vertices[0, 0]) and vertices[share >= 64, 0].min() < -0.5
  assert vertices[:, 1:].min() == 0 and want['origin'][0] == vertices[:, 0].min() < -0.5
  assert want['origin'].view(np.int32)[1:].tolist() == [-2 ** 31, 0]                    # (-0, +0), by their bits


# ---- properties ------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize('name', ['sphere_0.25', 'cube', 'fan_of_3000', 'on_cell_faces', 'default_origin', 'row_257'])
def test_every_output_vertex_lies_in_its_own_cell_and_a_second_pass_changes_no_face(name):
  _, _, _, cell_size, origin, want = case(name)
  got, _, used_origin, _, _ = run(name)
  # the cell rule in torch float32 (on the host: one subtraction, one division, one floor)
  vertices, origin32 = got.vertices.cpu(), used_origin.cpu()
  cell = torch.floor((vertices - origin32) / torch.tensor(cell_size, dtype=torch.float32))
  assert cell.dtype == torch.float32 and torch.equal(cell.to(torch.int64), torch.from_numpy(want['cell']))
  again = simplify_mesh(got, cell_size, origin=used_origin)
  assert again.vertices.shape[0] == got.vertices.shape[0] and torch.equal(again.faces, got.faces)
  mean_first = run(name, 'mean')[0]
  assert torch.equal(mean_first.faces, got.faces)                       # the placement does not touch the connectivity
  assert torch.equal(simplify_mesh(mean_first, cell_size, origin=used_origin, placement='mean').faces, got.faces)


@pytest.mark.parametrize('name', ['sphere_0.20', 'fan_of_3000', 'loose_vertices'])
def test_two_runs_are_bitwise_equal(name):
  first, second = run(name), run(name)
  for a, b in zip((first[0].vertices, first[0].faces, first[0].colours, first[1], first[3]),
                  (second[0].vertices, second[0].faces, second[0].colours, second[1], second[3])):
    assert torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_the_quadric_keeps_the_cube_corner_and_the_sphere_radius():
  quadric, mean = run('cube')[0], run('cube', 'mean')[0]
  corner = lambda mesh: float(mesh.vertices.abs().amax(dim=1).min())      # the corner at (0, 0, 0), per axis
  assert corner(mean) > 100 * corner(quadric) and 0.05 < corner(mean) < 0.08      # the oracle predicts 1000 x
  _, vertex_map, _, choice, scan = run('cube', 'mean')
  want = so.simplify(*case('cube')[:2], 0.26, CUBE_ORIGIN, placement='mean', colours=case('cube')[2])
  assert compare(mean, vertex_map, choice[kept_clusters(scan)], want, 'cube, mean') == 0 and (want['choice'] == so.MEAN).all()
  for name in ('sphere_0.25', 'sphere_0.20'):
    want = case(name)[5]
    allowed = np.abs(np.linalg.norm(want['vertices'].astype(np.float64), axis=1) - 1).max()
    radius = run(name)[0].vertices.double().norm(dim=1)
    assert float((radius - 1).abs().max()) <= allowed + 2.0 ** -22


@functools.lru_cache(maxsize=None)
def extracted_sphere():
  n = 32
  volume = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (n - 1), (n, n, n), colour=False, device=DEVICE)
  volume.tsdf.copy_(((volume.positions().norm(dim=-1) - 0.8) / volume.truncation).clamp(-1, 1))
  volume.weight.fill_(1.0)
  return volume.extract_mesh(), 2.0 / (n - 1)


def test_an_extracted_sphere_simplified_at_three_voxels():
  mesh, voxel = extracted_sphere()
  vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
  colours = colours_of(vertices)
  mesh = on_device(vertices, faces, colours)
  want = so.simplify(vertices, faces, 3 * voxel, SPHERE_ORIGIN, colours=colours)
  got, vertex_map, _, choice, scan = tm._simplify(mesh, 3 * voxel, SPHERE_ORIGIN, 'quadric', 1e-3)
  compare(got, vertex_map, choice[kept_clusters(scan)], want, 'extracted sphere')
  assert 0 < got.faces.shape[0] < faces.shape[0] / 4
  shaded = with_vertex_normals(got)                                     # the next step of the path takes it as it is
  outward = (shaded.normals * torch.nn.functional.normalize(got.vertices, dim=1)).sum(dim=1)
  assert float(outward.min()) > 0.5


def test_the_vertex_map_is_consistent_with_the_faces():
  vertices, faces, colours, cell_size, origin, _ = case('loose_vertices')
  got, vertex_map = simplify_mesh(on_device(vertices, faces, colours), cell_size, origin, return_map=True)
  vertex_map, new_faces = vertex_map.cpu().numpy(), got.faces.cpu().numpy()
  referenced = np.zeros(vertices.shape[0], dtype=bool)
  referenced[faces.reshape(-1)] = True
  assert (vertex_map[~referenced] == -1).all() and vertex_map.max() == got.vertices.shape[0] - 1
  assert set(np.unique(vertex_map[vertex_map >= 0])) == set(range(got.vertices.shape[0]))       # onto the output vertices
  mapped = vertex_map[faces]
  alive = (mapped[:, 0] != mapped[:, 1]) & (mapped[:, 1] != mapped[:, 2]) & (mapped[:, 2] != mapped[:, 0])
  assert (mapped[alive] >= 0).all()                                     # a face that survives keeps all three clusters
  first = mapped[alive].argmin(axis=1)
  rotated = np.take_along_axis(mapped[alive], (first[:, None] + np.arange(3)) % 3, axis=1)
  _, where = np.unique(rotated, axis=0, return_index=True)
  assert np.array_equal(rotated[np.sort(where)], new_faces)             # first occurrences, in input order
  lost = so.simplify(*tetrahedron(), 1.0, (0, 0, 0))['vertex_map']      # a cluster that lost all its faces
  _, tetra_map = simplify_mesh(on_device(*tetrahedron()), 1.0, (0, 0, 0), return_map=True)
  assert lost.tolist() == [-1] * 4 == tetra_map.tolist()


def test_render_scene_tool_simplifies_its_mesh(tmp_path):
  """``tools/render_scene.py scene.ply --mesh … --keep-components 1 --mesh-cell-size s --mesh-normals``, a fresh child
  process: the report holds the counts before and after, the written file the simplified mesh with normals"""
  import json
  import subprocess
  import sys
  from pathlib import Path
  from taichi_splatting_amd import Gaussians3D, save_ply
  from tests import mesh_oracle as mo
  generator = torch.Generator().manual_seed(5)
  n = 600
  normal = torch.nn.functional.normalize(torch.randn((n, 3), generator=generator), dim=1)
  axis = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]).expand(n, 3), normal)
  rotation = torch.nn.functional.normalize(torch.cat([axis, 1.0 + normal[:, 2:3]], dim=1), dim=1)
  scene = Gaussians3D(position=0.8 * normal, log_scaling=torch.tensor([0.12, 0.12, 0.004]).log().expand(n, 3).contiguous(),
                      rotation=rotation, alpha_logit=torch.full((n, 1), 6.0), feature=torch.rand((n, 3, 1), generator=generator),
                      batch_size=(n,))
  save_ply(scene, tmp_path / 'scene.ply')
  tool = str(Path(__file__).resolve().parent.parent / 'tools' / 'render_scene.py')
  out = tmp_path / 'mesh.ply'
  done = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--views', '6', '--size', '64', '64', '--mesh', str(out),
                         '--voxel-size', '0.08', '--bounds', '-1.2', '-1.2', '-1.2', '1.2', '1.2', '1.2', '--keep-components', '1',
                         '--mesh-cell-size', '0.24', '--mesh-normals'], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stderr[-2000:]
  report = json.loads(done.stdout.strip().splitlines()[-1])['mesh']
  simplification = report['simplification']
  read = mo.read_mesh_ply(out)
  assert read['properties'][:6] == ['x', 'y', 'z', 'nx', 'ny', 'nz'] and report['normals'] is True
  assert simplification['cell_size'] == 0.24 and simplification['simplify_s'] >= 0.0
  assert report['vertices'] == simplification['vertices_after'] == read['vertex'].shape[0] > 20
  assert report['triangles'] == simplification['triangles_after'] == read['faces'].shape[0] > 20
  assert simplification['triangles_before'] > 4 * simplification['triangles_after']
  assert simplification['vertices_before'] > 4 * simplification['vertices_after']
  assert report['triangles_before'] >= simplification['triangles_before']        # the clean-up ran first


# ---- errors ----------------------------------------------------------------------------------------------------------------

def raises_and_leaves_the_input(mesh, match, **arguments):
  before = [bits(mesh.vertices).clone(), mesh.faces.clone()]
  with pytest.raises(ValueError, match=match):
    simplify_mesh(mesh, **arguments)
  assert torch.equal(bits(mesh.vertices), before[0]) and torch.equal(mesh.faces, before[1])


def test_errors_found_on_the_device():
  vertices, faces = so.icosphere(1)
  for bad in (vertices.shape[0], -1, 2 ** 31 - 1):
    broken = faces.copy()
    broken[7, 1] = bad
    raises_and_leaves_the_input(on_device(vertices, broken), "outside 0", cell_size=0.5)
  for value in (np.nan, np.inf, -np.inf):
    broken = vertices.copy()
    broken[5, 2] = value
    raises_and_leaves_the_input(on_device(broken, faces), "not finite", cell_size=0.5, origin=(-2, -2, -2))
  loose = np.concatenate([vertices, [(np.nan, 0, 0), (np.inf, np.nan, 0)]]).astype(np.float32)       # unreferenced: legal
  want = so.simplify(vertices, faces, 0.5, (-2, -2, -2))
  for origin in ((-2, -2, -2), None):
    got = simplify_mesh(on_device(loose, faces), 0.5, origin=origin)
    if origin is not None:
      assert np.array_equal(got.faces.cpu().numpy(), want['faces'])
    assert got.vertices.shape[0] > 0 and bool(torch.isfinite(got.vertices).all())
  # cell indices: 2^21 - 1 is the last legal one, 2^21 is not; a vertex below the origin is not
  edge = np.array([(0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (2.0 ** 21 - 1, 1.5, 0.5)], dtype=np.float32)
  got = simplify_mesh(on_device(edge, [(0, 1, 2)]), 1.0, origin=(0, 0, 0))
  assert got.faces.tolist() == [[0, 1, 2]] and float(got.vertices[2, 0]) == 2.0 ** 21 - 1
  edge[2, 0] = 2.0 ** 21
  raises_and_leaves_the_input(on_device(edge, [(0, 1, 2)]), "cell outside", cell_size=1.0, origin=(0, 0, 0))
  raises_and_leaves_the_input(on_device(edge[:, [1, 2, 0]], [(0, 1, 2)]), "cell outside", cell_size=1.0, origin=(0, 0, 0))
  raises_and_leaves_the_input(on_device(vertices, faces), "cell outside", cell_size=0.5, origin=(0, -2, -2))
  raises_and_leaves_the_input(on_device(vertices, faces), "cell outside", cell_size=1e-7, origin=(-2, -2, -2))


def test_a_cpu_tensor_raises():
  vertices, faces = so.icosphere(1)
  mesh = on_device(vertices, faces)
  for broken in (TriangleMesh(mesh.vertices.cpu(), mesh.faces), TriangleMesh(mesh.vertices, mesh.faces.cpu()),
                 TriangleMesh(mesh.vertices.cpu(), mesh.faces.cpu()), TriangleMesh(mesh.vertices, mesh.faces, colours=mesh.vertices.cpu())):
    with pytest.raises(ValueError, match="no CPU fallback"):
      simplify_mesh(broken, 0.5)
  got = simplify_mesh(mesh, 0.5, origin=torch.tensor([-2.0, -2.0, -2.0], dtype=torch.float64))      # a host origin is an argument
  assert got.colours is None and got.normals is None and got.faces.shape[0] > 0
