"""Mesh clean-up on the GPU (taichi_splatting_amd/mesh.py, csrc/mesh.hip) against the numpy oracle of tests/mesh_oracle.py.

Components, counts and selections are compared EXACTLY (labels follow the smallest-vertex-index rule, selections are
stable bit copies).  The normal sums are held to the bound the oracle's docstring derives from the kernel's stated
operation order (float64 differences, products and in-order sum, one rounding to float32):
|s - s64| <= NORMAL_C 2^-24 S(v) per component with NORMAL_C = 2 and S(v) = sum |b - a| |c - a|; the unit normals to
UNIT_NORMAL_BOUND where |s64| >= 0.1 S(v).

The sizes are the smallest at which the kernels can go wrong: a strip longer than a workgroup (with the numbering that
gives the longest parent chains), a fan whose hooks all contend for one root, 10 001 components in one launch (every wave
of the count kernel then holds 64 labels, beside waves that hold one), and 21^3 / 33^3 fields extracted on the device.
"""
import functools

import numpy as np
import pytest
import torch

from taichi_splatting_amd import TSDFVolume, TriangleMesh, save_mesh_ply
from taichi_splatting_amd import mesh as tm
from tests import mesh_oracle as mo
from tests import tsdf_oracle as to

pytestmark = pytest.mark.gpu
DEVICE = 'cuda:0'
EPS = mo.EPS


def bits(t):
  return t.contiguous().view(torch.int32)


def on_device(vertices, faces, colours=None, normals=None):
  move = lambda a, dtype: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(dtype).to(DEVICE)
  return TriangleMesh(vertices=move(vertices, torch.float32).reshape(-1, 3), faces=move(faces, torch.int32).reshape(-1, 3),
                      colours=move(colours, torch.float32), normals=move(normals, torch.float32))


def extract_field(values, weight, origin, voxel_size, colour=None):
  nz, ny, nx = values.shape
  volume = TSDFVolume(origin, voxel_size, (nx, ny, nz), colour=colour is not None, device=DEVICE)
  volume.tsdf.copy_(torch.as_tensor(values))
  volume.weight.copy_(torch.as_tensor(weight))
  if colour is not None:
    volume.colour.copy_(torch.as_tensor(colour))
  return volume.extract_mesh()


@functools.lru_cache(maxsize=None)
def extracted(kind):
  """the 21^3 sphere / torus of tests/test_gpu_tsdf.py, extracted on the device: (mesh, vertices, faces); not modified"""
  mesh = extract_field(*mo.analytic_field(kind), mo.ORIGIN, mo.H)
  return mesh, mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()


def reversed_strip(triangles):
  vertices, faces = mo.strip(triangles)
  return mo.permute_vertices(vertices, faces, np.arange(vertices.shape[0])[::-1].copy())


def permuted_strip(triangles):
  vertices, faces = mo.strip(triangles)
  return mo.permute_vertices(vertices, faces, np.random.default_rng(7).permutation(vertices.shape[0]))


def small(faces, num_vertices):
  vertices = np.random.default_rng(num_vertices).uniform(-1.0, 1.0, size=(num_vertices, 3)).astype(np.float32)
  return vertices, np.asarray(faces, dtype=np.int32).reshape(-1, 3)


CASES = {
  'empty': lambda: small([], 0),
  'vertices_without_faces': lambda: small([], 5),
  'one_triangle': lambda: small([(2, 0, 1)], 3),
  'two_triangles_sharing_one_vertex': lambda: small([(0, 1, 2), (2, 3, 4)], 5),
  'two_triangles_sharing_none': lambda: small([(5, 1, 2), (0, 3, 4)], 6),
  'degenerate_and_duplicate': lambda: small([(0, 0, 1), (2, 3, 4), (2, 3, 4), (5, 5, 5), (7, 6, 7)], 9),
  'strip_ascending': lambda: mo.strip(3000),
  'strip_reversed': lambda: reversed_strip(3000),
  'strip_permuted': lambda: permuted_strip(3000),
  'fan_hub_last': lambda: mo.fan(5000, hub_last=True),
  'fan_hub_first': lambda: mo.fan(5000, hub_last=False),
  'fan_of_twelve': lambda: mo.fan(12, hub_last=True),
  'soup': lambda: mo.soup(10000, 20000, 100),
  'sphere': lambda: extracted('sphere')[1:],
  'torus': lambda: extracted('torus')[1:],
}


@functools.lru_cache(maxsize=None)
def case(name):
  """(vertices, faces, oracle components): built once, shared, not modified"""
  vertices, faces = CASES[name]()
  return vertices, faces, mo.components(vertices.shape[0], faces)


def assert_components_equal(got, want):
  assert got.num_components == want['num_components']
  for name in ('vertex_label', 'face_label', 'face_count', 'vertex_count'):
    tensor = getattr(got, name)
    assert tensor.dtype == torch.int32 and tuple(tensor.shape) == want[name].shape, name
    assert np.array_equal(tensor.cpu().numpy(), want[name]), name


@pytest.mark.parametrize('name', list(CASES))
def test_components_equal_the_oracle_exactly(name):
  vertices, faces, want = case(name)
  mesh = on_device(vertices, faces)
  got = tm.mesh_components(mesh)
  assert isinstance(got.num_components, int)
  assert_components_equal(got, want)
  print(f"{name}: V = {vertices.shape[0]}, T = {faces.shape[0]}, K = {got.num_components}")
  assert np.array_equal(mesh.faces.cpu().numpy(), faces) and np.array_equal(bits(mesh.vertices).cpu().numpy(), vertices.view(np.int32))


@pytest.mark.parametrize('name', ['strip_permuted', 'soup', 'sphere'])
def test_labels_do_not_depend_on_face_order_and_runs_repeat(name):
  vertices, faces, want = case(name)
  first = tm.mesh_components(on_device(vertices, faces))
  again = tm.mesh_components(on_device(vertices, faces))
  for field in ('vertex_label', 'face_label', 'face_count', 'vertex_count'):
    assert torch.equal(getattr(first, field), getattr(again, field)), field
  assert first.num_components == again.num_components
  order = np.random.default_rng(11).permutation(faces.shape[0])
  shuffled = tm.mesh_components(on_device(vertices, faces[order]))
  assert torch.equal(shuffled.vertex_label, first.vertex_label)
  assert np.array_equal(shuffled.face_label.cpu().numpy(), want['face_label'][order])
  assert torch.equal(shuffled.face_count, first.face_count) and torch.equal(shuffled.vertex_count, first.vertex_count)


@pytest.mark.parametrize('bad', [-1, 9, 2 ** 31 - 1, -2 ** 31])
def test_an_index_out_of_range_raises_and_leaves_the_mesh_alone(bad):
  vertices, faces = small([(0, 1, 2), (3, 4, 5), (6, 7, 8), (1, 4, 7)], 9)
  faces = faces.copy()
  faces[2, 1] = bad
  mesh = on_device(vertices, faces)
  mesh.colours = mesh.vertices.clone()
  before = [t.clone() for t in (mesh.vertices, mesh.faces, mesh.colours)]
  with pytest.raises(ValueError, match="outside"):
    tm.mesh_components(mesh)
  with pytest.raises(ValueError, match="outside"):
    tm.remove_small_components(mesh, min_faces=2)
  with pytest.raises(ValueError, match="outside"):
    tm.select_faces(mesh, torch.ones((4,), dtype=torch.bool, device=DEVICE))
  dropped = tm.select_faces(mesh, torch.tensor([True, True, False, True], device=DEVICE))       # the bad face is not kept
  assert dropped.faces.shape[0] == 3 and dropped.vertices.shape[0] == 7
  normals = tm.vertex_normals(mesh)                                   # no host read: the bad face contributes nothing
  rest = np.delete(faces, 2, axis=0)
  want = mo.unit_normals(vertices, rest)
  well = np.linalg.norm(mo.normal_sums(vertices, rest), axis=1) >= mo.WELL_CONDITIONED * mo.normal_scale(vertices, rest)
  assert well.sum() >= 5 and np.abs(normals.cpu().numpy() - want)[well].max() <= mo.UNIT_NORMAL_BOUND
  assert bool((normals[[6, 8]] == 0).all())
  for t, b in zip((mesh.vertices, mesh.faces, mesh.colours), before):
    assert torch.equal(bits(t), bits(b))


# ---- selection ----------------------------------------------------------------------------------------------------------

def arbitrary_rows(count, seed):
  """(count, 3) float32 rows of arbitrary bit patterns (NaNs, infinities and subnormals included)"""
  raw = np.random.default_rng(seed).integers(-2 ** 31, 2 ** 31 - 1, size=(count, 3), dtype=np.int64).astype(np.int32)
  return raw.view(np.float32)


@pytest.mark.parametrize('which', ['random', 'all_true', 'all_false'])
@pytest.mark.parametrize('attributes', [True, False])
def test_select_faces_equals_the_oracle_exactly(which, attributes):
  vertices, faces, _ = case('soup')
  count, total = vertices.shape[0], faces.shape[0]
  colours = arbitrary_rows(count, 1) if attributes else None
  normals = arbitrary_rows(count, 2) if attributes else None
  mask = {'random': np.random.default_rng(3).random(total) < 0.4, 'all_true': np.ones(total, dtype=bool),
          'all_false': np.zeros(total, dtype=bool)}[which]
  mesh = on_device(vertices, faces, colours, normals)
  got = tm.select_faces(mesh, torch.from_numpy(mask).to(DEVICE))
  want_v, want_f, want_c, want_n = mo.select(vertices, faces, mask, colours, normals)
  assert got.vertices.dtype == torch.float32 and got.faces.dtype == torch.int32
  assert tuple(got.vertices.shape) == want_v.shape and tuple(got.faces.shape) == want_f.shape
  assert np.array_equal(bits(got.vertices).cpu().numpy(), want_v.view(np.int32))
  assert np.array_equal(got.faces.cpu().numpy(), want_f)
  if attributes:
    assert np.array_equal(bits(got.colours).cpu().numpy(), want_c.view(np.int32))
    assert np.array_equal(bits(got.normals).cpu().numpy(), want_n.view(np.int32))
  else:
    assert got.colours is None and got.normals is None
  if which == 'all_false':
    assert got.vertices.shape == (0, 3) and got.faces.shape == (0, 3)
    assert tm.mesh_components(got).num_components == 0 and tm.vertex_normals(got).shape == (0, 3)
  if which == 'all_true':                                             # only the 100 unreferenced vertices leave
    assert got.vertices.shape[0] == count - 100 and got.faces.shape == mesh.faces.shape
  again = tm.select_faces(mesh, torch.from_numpy(mask).to(DEVICE))
  assert torch.equal(bits(again.vertices), bits(got.vertices)) and torch.equal(again.faces, got.faces)


def test_an_all_true_mask_on_a_mesh_without_loose_vertices_is_a_bit_copy():
  mesh, vertices, faces = extracted('torus')
  coloured = TriangleMesh(vertices=mesh.vertices, faces=mesh.faces, colours=on_device(arbitrary_rows(vertices.shape[0], 5), faces).vertices)
  got = tm.select_faces(coloured, torch.ones((faces.shape[0],), dtype=torch.bool, device=DEVICE))
  assert torch.equal(bits(got.vertices), bits(mesh.vertices)) and torch.equal(got.faces, mesh.faces)
  assert torch.equal(bits(got.colours), bits(coloured.colours)) and got.normals is None
  assert got.vertices.data_ptr() != mesh.vertices.data_ptr()


# ---- small components ---------------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def floater_scene():
  """two spheres of different radius and 30 one-cell shells (single inside samples in free space, no two adjacent) in one
  33^3 field, extracted on the device: (mesh, vertices, faces, oracle components)"""
  dims, h = (33, 33, 33), 0.25
  positions = to.grid_positions((0.0, 0.0, 0.0), h, dims)
  field = np.minimum(to.sphere_field(positions, np.array([2.6, 2.7, 2.5]), 1.6), to.sphere_field(positions, np.array([6.0, 5.9, 6.1]), 1.1))
  values = field.astype(np.float32)
  free = [(k, j, i) for k in range(2, 31, 4) for j in range(2, 31, 4) for i in range(2, 31, 4) if values[k, j, i] > 0.8]
  chosen = [free[n] for n in np.random.default_rng(4).permutation(len(free))[:30]]
  assert len(chosen) == 30
  for k, j, i in chosen:
    values[k, j, i] = -0.1
  colour = np.random.default_rng(6).random((33, 33, 33, 3)).astype(np.float32)
  mesh = extract_field(values, np.ones_like(values), (0.0, 0.0, 0.0), h, colour)
  vertices, faces = mesh.vertices.cpu().numpy(), mesh.faces.cpu().numpy()
  return mesh, vertices, faces, mo.components(vertices.shape[0], faces)


def assert_selection(got, vertices, faces, mask, colours=None):
  want_v, want_f, want_c, _ = mo.select(vertices, faces, mask, colours)
  assert np.array_equal(bits(got.vertices).cpu().numpy(), want_v.view(np.int32))          # input rows, in input order
  assert np.array_equal(got.faces.cpu().numpy(), want_f)
  if colours is not None:
    assert np.array_equal(bits(got.colours).cpu().numpy(), want_c.view(np.int32))


def test_remove_small_components_keeps_the_two_spheres():
  mesh, vertices, faces, want = floater_scene()
  colours = mesh.colours.cpu().numpy()
  counts = np.sort(want['face_count'])
  assert want['num_components'] == 32 and (counts[:30] == counts[0]).all() and counts[30] > 10 * counts[0]
  shell_faces = int(counts[0])
  print(f"floater scene: V = {vertices.shape[0]}, T = {faces.shape[0]}, 30 shells of {shell_faces} faces, spheres of {counts[30:].tolist()}")

  cleaned, components = tm.remove_small_components(mesh, min_faces=shell_faces + 1, return_components=True)
  assert_components_equal(components, want)
  assert_selection(cleaned, vertices, faces, mo.keep_mask(want['face_label'], want['face_count'], shell_faces + 1), colours)
  after = tm.mesh_components(cleaned)
  assert after.num_components == 2 and sorted(after.face_count.tolist()) == counts[30:].tolist()
  for label in range(2):
    part = tm.select_faces(cleaned, after.face_label == label).faces.cpu().numpy().astype(np.int64)
    assert to.euler_characteristic(part) == 2
    assert (to.undirected_edges(part)[1] == 2).all() and (to.directed_edge_multiplicities(part) == 1).all()

  same = tm.remove_small_components(mesh, min_faces=shell_faces)                          # the threshold is inclusive
  assert same.faces.shape[0] == faces.shape[0]
  largest = tm.remove_small_components(mesh, keep_largest=1)
  assert largest.faces.shape[0] == int(counts[-1])
  assert_selection(largest, vertices, faces, mo.keep_mask(want['face_label'], want['face_count'], 1, 1), colours)
  assert to.euler_characteristic(largest.faces.cpu().numpy().astype(np.int64)) == 2
  for min_faces, keep_largest in ((1, 3), (1, 2), (shell_faces + 1, 5), (shell_faces, 31), (10 ** 9, None), (10 ** 12, 2), (1, 10 ** 12)):
    got = tm.remove_small_components(mesh, min_faces=min_faces, keep_largest=keep_largest)
    assert_selection(got, vertices, faces, mo.keep_mask(want['face_label'], want['face_count'], min_faces, keep_largest), colours)


def test_a_tie_goes_to_the_lower_label():
  mesh, vertices, faces, want = floater_scene()
  shell_faces = int(want['face_count'].min())
  shells = tm.select_faces(mesh, torch.from_numpy(want['face_count'][want['face_label']] == shell_faces).to(DEVICE))
  components = tm.mesh_components(shells)
  assert components.num_components == 30 and bool((components.face_count == shell_faces).all())
  for keep in (1, 2, 29):
    got = tm.remove_small_components(shells, keep_largest=keep)
    assert got.faces.shape[0] == keep * shell_faces
    want_faces = tm.select_faces(shells, components.face_label < keep)
    assert torch.equal(got.faces, want_faces.faces) and torch.equal(bits(got.vertices), bits(want_faces.vertices))
  two = on_device(*small([(3, 4, 5), (0, 1, 2)], 6))                  # two identical single-triangle shells: label 0 = vertex 0
  got = tm.remove_small_components(two, keep_largest=1)
  assert torch.equal(bits(got.vertices), bits(two.vertices[:3])) and got.faces.cpu().tolist() == [[0, 1, 2]]


# ---- normals ------------------------------------------------------------------------------------------------------------

NORMAL_CASES = ['fan_hub_last', 'fan_of_twelve', 'strip_permuted', 'soup', 'sphere', 'torus', 'degenerate_and_duplicate']


@pytest.mark.parametrize('name', NORMAL_CASES)
def test_normal_sums_within_the_derived_bound(name):
  vertices, faces, _ = case(name)
  mesh = on_device(vertices, faces)
  got = tm.vertex_normal_sums(mesh)
  assert got.dtype == torch.float32 and tuple(got.shape) == vertices.shape
  want, scale = mo.normal_sums(vertices, faces), mo.normal_scale(vertices, faces)
  error = np.abs(got.cpu().numpy().astype(np.float64) - want).max(axis=1)
  bound = mo.NORMAL_C * EPS * scale
  live = scale > 0
  ratio = float((error[live] / bound[live]).max()) if live.any() else 0.0
  print(f"{name}: largest |s - s64| / (c 2^-24 S) = {ratio:.3f} with c = {mo.NORMAL_C}; largest degree {int(mo.degree(vertices.shape[0], faces).max())}")
  assert (error <= bound).all(), ratio
  assert torch.equal(bits(tm.vertex_normal_sums(mesh)), bits(got))


# the 5000 slivers of the large fan (apex angle 2 pi / 5000) are ill conditioned at every vertex by the measure below: the
# unit normal is checked on a fan of twelve instead
@pytest.mark.parametrize('name', NORMAL_CASES[1:])
def test_unit_normals_where_well_conditioned(name):
  vertices, faces, _ = case(name)
  mesh = on_device(vertices, faces)
  got = tm.vertex_normals(mesh)
  shaded = tm.with_vertex_normals(mesh)
  assert torch.equal(bits(shaded.normals), bits(got)) and shaded.vertices is mesh.vertices and mesh.normals is None
  got = got.cpu().numpy().astype(np.float64)
  assert np.isfinite(got).all()
  sums, scale = mo.normal_sums(vertices, faces), mo.normal_scale(vertices, faces)
  length = np.linalg.norm(sums, axis=1)
  referenced = mo.degree(vertices.shape[0], faces) > 0
  well = referenced & (scale > 0) & (length >= mo.WELL_CONDITIONED * scale)
  left_out = referenced & (scale > 0) & ~well
  fraction = float(left_out.sum()) / max(int(referenced.sum()), 1)
  error = np.abs(got[well] - sums[well] / length[well, None]).max() if well.any() else 0.0
  print(f"{name}: {fraction:.4f} of the vertices below the conditioning threshold; largest unit-normal error {error:.3e}, "
        f"bound {mo.UNIT_NORMAL_BOUND:.3e}")
  assert fraction <= 0.02
  assert error <= mo.UNIT_NORMAL_BOUND
  assert (got[~referenced] == 0).all() and (got[referenced & (scale == 0)] == 0).all()
  norms = np.linalg.norm(got[well], axis=1)
  assert (np.abs(norms - 1) <= 4 * EPS).all()


def test_sphere_normals_point_outward():
  _, vertices, faces = extracted('sphere')
  normals = tm.vertex_normals(extracted('sphere')[0]).cpu().numpy().astype(np.float64)
  radial = vertices.astype(np.float64) - mo.CENTRE
  radial /= np.linalg.norm(radial, axis=1, keepdims=True)
  cosine = (normals * radial).sum(axis=1)
  angle = float(np.degrees(np.arccos(np.clip(cosine.min(), -1, 1))))
  print(f"sphere: largest angle between a vertex normal and the radial direction {angle:.2f} degrees")
  assert (cosine > 0).all() and angle < 15.0


def test_zero_sums_and_unreferenced_vertices_give_exact_zeros():
  vertices = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [5, 5, 5], [2, 2, 2], [3, 2, 2], [2, 3, 2], [1, 1, 1]], dtype=np.float32)
  faces = np.array([(0, 1, 2), (0, 2, 1), (4, 5, 6), (4, 4, 6), (7, 7, 7)], dtype=np.int32)     # vertex 3 unreferenced
  mesh = on_device(vertices, faces)
  normals, sums = tm.vertex_normals(mesh).cpu().numpy(), tm.vertex_normal_sums(mesh).cpu().numpy()
  assert not np.isnan(normals).any() and not np.isnan(sums).any()
  assert (normals[[0, 1, 2, 3, 7]] == 0).all() and (sums[[0, 1, 2, 3, 7]] == 0).all()
  assert np.array_equal(normals[4:7], np.tile(np.array([0, 0, 1], dtype=np.float32), (3, 1)))
  only_vertices = on_device(vertices, np.zeros((0, 3), dtype=np.int32))
  assert bool((tm.vertex_normals(only_vertices) == 0).all())


def test_vertex_normals_capture_into_a_graph():
  """no host read: captured once, replayed after the positions were rewritten in place, equal bits to an eager call"""
  _, vertices, faces = extracted('torus')
  mesh = on_device(vertices, faces)
  moved = torch.from_numpy(vertices * np.array([1.0, 0.5, 2.0], dtype=np.float32) + 0.25).to(DEVICE)
  eager_first = tm.vertex_normals(mesh)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured = tm.vertex_normals(mesh)
  graph.replay()
  torch.cuda.synchronize()
  assert torch.equal(bits(captured), bits(eager_first))
  mesh.vertices.copy_(moved)
  graph.replay()
  torch.cuda.synchronize()
  eager_second = tm.vertex_normals(mesh)
  assert torch.equal(bits(captured), bits(eager_second)) and not torch.equal(bits(eager_first), bits(eager_second))


# ---- the whole path -----------------------------------------------------------------------------------------------------

def test_extract_clean_shade_save_and_read_back(tmp_path):
  mesh, _, _, want = floater_scene()
  shell_faces = int(want['face_count'].min())
  cleaned = tm.with_vertex_normals(tm.remove_small_components(mesh, min_faces=shell_faces + 1))
  assert cleaned.normals is not None and cleaned.colours is not None
  path = tmp_path / 'clean.ply'
  save_mesh_ply(cleaned, path)
  read = mo.read_mesh_ply(path)
  assert read['properties'] == ['x', 'y', 'z', 'nx', 'ny', 'nz', 'red', 'green', 'blue']
  assert read['vertex'].shape[0] == cleaned.vertices.shape[0] and read['faces'].shape == tuple(cleaned.faces.shape)
  xyz = np.stack([read['vertex'][n] for n in 'xyz'], axis=1)
  nxyz = np.stack([read['vertex'][n] for n in ('nx', 'ny', 'nz')], axis=1)
  rgb = np.stack([read['vertex'][n] for n in ('red', 'green', 'blue')], axis=1)
  assert np.array_equal(xyz.view(np.int32), bits(cleaned.vertices).cpu().numpy())
  assert np.array_equal(nxyz.view(np.int32), bits(cleaned.normals).cpu().numpy())
  assert np.array_equal(rgb, cleaned.colours.clamp(0, 1).mul(255).round().to(torch.uint8).cpu().numpy())
  assert np.array_equal(read['faces'], cleaned.faces.cpu().numpy())
  assert 0 < cleaned.faces.shape[0] < mesh.faces.shape[0]
  assert np.abs(np.linalg.norm(nxyz, axis=1) - 1).max() < 1e-6


def test_render_scene_tool_cleans_and_shades_its_mesh(tmp_path):
  """``tools/render_scene.py scene.ply --mesh … --keep-components 1 --min-component-faces N --mesh-normals``, a fresh
  child process: the written file holds one component with normals, the report the counts before cleaning"""
  import json
  import subprocess
  import sys
  from pathlib import Path
  from taichi_splatting_amd import Gaussians3D, save_ply
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
                         '--voxel-size', '0.08', '--bounds', '-1.2', '-1.2', '-1.2', '1.2', '1.2', '1.2', '--min-component-faces', '10',
                         '--keep-components', '1', '--mesh-normals'], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stderr[-2000:]
  report = json.loads(done.stdout.strip().splitlines()[-1])['mesh']
  read = mo.read_mesh_ply(out)
  assert read['properties'][:6] == ['x', 'y', 'z', 'nx', 'ny', 'nz'] and report['normals'] is True
  assert report['vertices'] == read['vertex'].shape[0] > 50 and report['triangles'] == read['faces'].shape[0] > 50
  assert report['triangles_before'] >= report['triangles'] and report['components'] >= 1 and report['clean_s'] >= 0.0
  assert mo.components(report['vertices'], read['faces'])['num_components'] == 1
