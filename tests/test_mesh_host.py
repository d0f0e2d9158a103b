"""The mesh oracle against an independent implementation, and the host side of the mesh calls (no GPU).

tests/mesh_oracle.py is what tests/test_gpu_mesh.py compares the kernels with, so its partition is checked here against
scipy.sparse.csgraph.connected_components on the vertex graph; label order, the -1 rule and selection are checked on
cases small enough to state by hand.  save_mesh_ply is a host function: its bytes without normals must be those of the
writer as it was before the ``normals`` field existed (kept below, verbatim), and its file with normals must parse back.
"""
import numpy as np
import pytest
import torch

from taichi_splatting_amd import TriangleMesh, save_mesh_ply
from taichi_splatting_amd import mesh as tm
from tests import mesh_oracle as mo


def scipy_partition(num_vertices, faces):
  from scipy.sparse import coo_matrix
  from scipy.sparse.csgraph import connected_components
  faces = np.asarray(faces, dtype=np.int64).reshape(-1, 3)
  rows = np.concatenate([faces[:, 0], faces[:, 1], faces[:, 2]])
  cols = np.concatenate([faces[:, 1], faces[:, 2], faces[:, 0]])
  graph = coo_matrix((np.ones(rows.shape[0]), (rows, cols)), shape=(num_vertices, num_vertices))
  _, label = connected_components(graph, directed=False)
  referenced = np.zeros((num_vertices,), dtype=bool)
  referenced[faces.reshape(-1)] = True
  return np.where(referenced, label, -1)


def random_soup(rng, num_vertices, num_faces):
  return rng.integers(0, num_vertices, size=(num_faces, 3)).astype(np.int32)


@pytest.mark.parametrize('num_vertices, num_faces, seed', [(1, 1, 0), (10, 3, 1), (50, 20, 2), (300, 80, 3), (300, 400, 4), (2000, 700, 5)])
def test_oracle_partition_equals_scipy_on_random_soups(num_vertices, num_faces, seed):
  faces = random_soup(np.random.default_rng(seed), num_vertices, num_faces)
  got = mo.components(num_vertices, faces)
  want = scipy_partition(num_vertices, faces)
  assert mo.same_partition(got['vertex_label'], want)
  live = want >= 0
  assert got['num_components'] == len(np.unique(want[live]))
  assert int(got['face_count'].sum()) == num_faces and int(got['vertex_count'].sum()) == int(live.sum())


@pytest.mark.parametrize('kind, handles', [('sphere', 0), ('torus', 1)])
def test_oracle_partition_equals_scipy_on_the_analytic_meshes(kind, handles):
  from tests import tsdf_oracle as to
  vertices, faces = mo.analytic_mesh(kind)
  got = mo.components(vertices.shape[0], faces)
  assert got['num_components'] == 1 and mo.same_partition(got['vertex_label'], scipy_partition(vertices.shape[0], faces))
  assert to.euler_characteristic(faces.astype(np.int64)) == 2 - 2 * handles
  both = np.concatenate([faces, faces[::-1] + vertices.shape[0]])     # two copies: two components, the first labelled 0
  got = mo.components(2 * vertices.shape[0] + 3, both)
  assert got['num_components'] == 2 and got['face_count'].tolist() == [faces.shape[0]] * 2
  assert (got['vertex_label'][:vertices.shape[0]] == 0).all() and (got['vertex_label'][-3:] == -1).all()
  assert mo.same_partition(got['vertex_label'], scipy_partition(2 * vertices.shape[0] + 3, both))


def test_label_order_and_the_minus_one_rule():
  faces = np.array([(7, 8, 9), (4, 2, 5), (9, 3, 7), (0, 0, 0)], dtype=np.int32)        # roots 3, 2 and 0; 1 and 6 unreferenced
  got = mo.components(10, faces)
  assert got['vertex_label'].tolist() == [0, -1, 1, 2, 1, 1, -1, 2, 2, 2]
  assert got['face_label'].tolist() == [2, 1, 2, 0]
  assert got['num_components'] == 3 and got['face_count'].tolist() == [1, 1, 2] and got['vertex_count'].tolist() == [1, 3, 4]
  for seed in range(3):                                               # any order of the faces: the same vertex labels
    again = mo.components(10, mo.shuffle_faces(faces, seed))
    assert np.array_equal(again['vertex_label'], got['vertex_label'])
  empty = mo.components(4, np.zeros((0, 3), dtype=np.int32))
  assert empty['num_components'] == 0 and empty['vertex_label'].tolist() == [-1] * 4 and empty['face_count'].shape == (0,)
  with pytest.raises(ValueError):
    mo.components(3, [(0, 1, 3)])
  with pytest.raises(ValueError):
    mo.components(3, [(0, -1, 2)])


def test_builders():
  vertices, faces = mo.strip(7)
  assert vertices.shape == (9, 3) and faces.shape == (7, 3) and mo.components(9, faces)['num_components'] == 1
  normals = mo.unit_normals(vertices, faces)
  assert (normals[:, 2] < -0.5).all()                                 # consistently oriented
  for hub_last in (True, False):
    vertices, faces = mo.fan(12, hub_last)
    assert mo.degree(13, faces).max() == 12 and mo.degree(13, faces)[12 if hub_last else 0] == 12
    assert (mo.unit_normals(vertices, faces)[:, 2] > 0).all()
  vertices, faces = mo.soup(40, 60, 5)
  got = mo.components(vertices.shape[0], faces)
  assert got['num_components'] == 41 and sorted(got['face_count'].tolist())[-2:] == [1, 60] and int((got['vertex_label'] < 0).sum()) == 5
  moved_v, moved_f = mo.permute_vertices(vertices, faces, np.random.default_rng(0).permutation(vertices.shape[0]))
  assert np.allclose(np.sort(mo.normal_scale(moved_v, moved_f)), np.sort(mo.normal_scale(vertices, faces)))


def test_selection_round_trips():
  vertices, faces = mo.soup(30, 50, 4)
  colours = np.random.default_rng(1).random(vertices.shape).astype(np.float32)
  everything = np.ones((faces.shape[0],), dtype=bool)
  v, f, c, n = mo.select(vertices, faces, everything, colours)
  assert n is None and v.shape[0] == vertices.shape[0] - 4 and np.array_equal(v[f], vertices[faces]) and np.array_equal(c[f], colours[faces])
  again = mo.select(v, f, everything, c)                              # nothing loose is left: the identity
  assert np.array_equal(again[0], v) and np.array_equal(again[1], f) and np.array_equal(again[2], c)
  mask = np.random.default_rng(2).random(faces.shape[0]) < 0.5
  v, f, c, _ = mo.select(vertices, faces, mask, colours)
  assert np.array_equal(v[f], vertices[faces[mask]])                  # same triangles, same order
  assert (np.diff(np.flatnonzero(np.isin(np.arange(vertices.shape[0]), faces[mask]))) > 0).all()
  assert mo.degree(v.shape[0], f).min() >= 1
  v, f, _, _ = mo.select(vertices, faces, ~everything)
  assert v.shape == (0, 3) and f.shape == (0, 3)
  got = mo.components(vertices.shape[0], faces)
  keep = mo.keep_mask(got['face_label'], got['face_count'], min_faces=2)
  assert int(keep.sum()) == 50
  keep = mo.keep_mask(got['face_label'], got['face_count'], keep_largest=2)
  assert int(keep.sum()) == 51 and keep[np.flatnonzero(got['face_label'] == np.flatnonzero(got['face_count'] == 1)[0])].all()


# ---- save_mesh_ply -------------------------------------------------------------------------------------------------------

def save_mesh_ply_before_normals(mesh, path):
  """the writer as it stood before TriangleMesh had normals"""
  vertices = mesh.vertices.detach().cpu()
  faces = mesh.faces.detach().cpu()
  count = vertices.shape[0]
  coloured = mesh.colours is not None
  fields = [('x', '<f4'), ('y', '<f4'), ('z', '<f4')]
  if coloured:
    colours = mesh.colours.detach().cpu()
    fields += [('red', 'u1'), ('green', 'u1'), ('blue', 'u1')]
  vertex_rows = np.zeros((count,), dtype=np.dtype(fields))
  xyz = vertices.to(torch.float32).numpy()
  for a, name in enumerate('xyz'):
    vertex_rows[name] = xyz[:, a]
  if coloured:
    rgb = torch.nan_to_num(colours.to(torch.float32), nan=0.0).clamp(0.0, 1.0).mul(255.0).round().to(torch.uint8).numpy()
    for a, name in enumerate(('red', 'green', 'blue')):
      vertex_rows[name] = rgb[:, a]
  face_rows = np.zeros((faces.shape[0],), dtype=np.dtype([('n', 'u1'), ('v', '<i4', (3,))]))
  face_rows['n'] = 3
  face_rows['v'] = faces.to(torch.int32).numpy()
  header = ["ply", "format binary_little_endian 1.0", f"element vertex {count}",
            "property float x", "property float y", "property float z"]
  if coloured:
    header += ["property uchar red", "property uchar green", "property uchar blue"]
  header += [f"element face {faces.shape[0]}", "property list uchar int vertex_indices", "end_header"]
  with open(path, 'wb') as f:
    f.write(("\n".join(header) + "\n").encode('ascii'))
    f.write(vertex_rows.tobytes())
    f.write(face_rows.tobytes())


def host_mesh(coloured, shaded, seed=0):
  vertices, faces = mo.soup(6, 9, 2, seed)
  rng = np.random.default_rng(seed)
  colours = torch.from_numpy(rng.uniform(-0.2, 1.2, size=vertices.shape).astype(np.float32)) if coloured else None
  normals = torch.from_numpy(mo.unit_normals(vertices, faces).astype(np.float32)) if shaded else None
  return TriangleMesh(vertices=torch.from_numpy(vertices), faces=torch.from_numpy(faces), colours=colours, normals=normals)


@pytest.mark.parametrize('coloured', [True, False])
def test_ply_without_normals_is_byte_for_byte_what_it_was(tmp_path, coloured):
  mesh = host_mesh(coloured, False)
  assert mesh.normals is None
  save_mesh_ply(mesh, tmp_path / 'new.ply')
  save_mesh_ply_before_normals(mesh, tmp_path / 'old.ply')
  assert (tmp_path / 'new.ply').read_bytes() == (tmp_path / 'old.ply').read_bytes()
  positional = TriangleMesh(mesh.vertices, mesh.faces, mesh.colours)   # the three-field construction still works
  assert positional.normals is None


@pytest.mark.parametrize('coloured', [True, False])
def test_ply_with_normals_parses_back(tmp_path, coloured):
  mesh = host_mesh(coloured, True)
  save_mesh_ply(mesh, tmp_path / 'shaded.ply')
  read = mo.read_mesh_ply(tmp_path / 'shaded.ply')
  assert read['properties'] == ['x', 'y', 'z', 'nx', 'ny', 'nz'] + (['red', 'green', 'blue'] if coloured else [])
  assert np.array_equal(np.stack([read['vertex'][n] for n in 'xyz'], axis=1), mesh.vertices.numpy())
  assert np.array_equal(np.stack([read['vertex'][n] for n in ('nx', 'ny', 'nz')], axis=1), mesh.normals.numpy())
  assert np.array_equal(read['faces'], mesh.faces.numpy())
  if coloured:
    rgb = np.stack([read['vertex'][n] for n in ('red', 'green', 'blue')], axis=1)
    assert np.array_equal(rgb, mesh.colours.clamp(0, 1).mul(255).round().to(torch.uint8).numpy())
  with pytest.raises(ValueError):
    save_mesh_ply(TriangleMesh(mesh.vertices, mesh.faces, mesh.colours, mesh.normals[:-1]), tmp_path / 'bad.ply')


# ---- argument errors, before any device work -----------------------------------------------------------------------------

def test_argument_errors_raise_before_any_device_work():
  mesh = host_mesh(True, True)
  calls = [tm.mesh_components, tm.vertex_normals, tm.vertex_normal_sums, tm.with_vertex_normals, tm.remove_small_components,
           lambda m: tm.select_faces(m, torch.ones((mesh.faces.shape[0],), dtype=torch.bool))]
  for call in calls:
    with pytest.raises(RuntimeError, match="no CPU fallback"):
      call(mesh)
    with pytest.raises(TypeError):
      call((mesh.vertices, mesh.faces))
    with pytest.raises(TypeError):
      call(TriangleMesh(mesh.vertices.double(), mesh.faces))
    with pytest.raises(TypeError):
      call(TriangleMesh(mesh.vertices, mesh.faces.long()))
    with pytest.raises(ValueError):
      call(TriangleMesh(mesh.vertices[:, :2], mesh.faces))
    with pytest.raises(ValueError):
      call(TriangleMesh(mesh.vertices, mesh.faces.reshape(-1)))
    with pytest.raises(ValueError):
      call(TriangleMesh(mesh.vertices, mesh.faces, colours=mesh.colours[:-1]))
    with pytest.raises(ValueError):
      call(TriangleMesh(mesh.vertices, mesh.faces, normals=mesh.normals[:, :2]))
  for bad in (0, -3, 1.5, '2', None, True):
    with pytest.raises(ValueError):
      tm.remove_small_components(mesh, min_faces=bad)
  for bad in (0, -1, 2.0, 'all', False):
    with pytest.raises(ValueError):
      tm.remove_small_components(mesh, keep_largest=bad)
  with pytest.raises(TypeError):
    tm.select_faces(TriangleMesh(mesh.vertices, mesh.faces), [True] * mesh.faces.shape[0])
  # beyond the limits: a ValueError from the shapes alone (meta tensors: nothing is allocated, nothing is launched)
  huge_faces = TriangleMesh(torch.empty((4, 3), device='meta'), torch.empty((2 ** 31 // 3 + 1, 3), dtype=torch.int32, device='meta'))
  huge_vertices = TriangleMesh(torch.empty((2 ** 31, 3), device='meta'), torch.empty((1, 3), dtype=torch.int32, device='meta'))
  for call in calls[:5]:
    for mesh_too_large in (huge_faces, huge_vertices):
      with pytest.raises(ValueError, match="2\\^31"):
        call(mesh_too_large)


def test_the_package_exports_the_mesh_calls():
  import taichi_splatting_amd as pkg
  for name in tm.__all__:
    if name[0].islower() or name == 'MeshComponents':
      assert getattr(pkg, name) is getattr(tm, name), name
  assert tm.MAX_VERTICES == tm.MAX_CORNERS == 2 ** 31 - 1
  fields = [f.name for f in __import__('dataclasses').fields(TriangleMesh)]
  assert fields == ['vertices', 'faces', 'colours', 'normals']
