"""TSDF fusion and mesh extraction without a GPU: the float64 oracle's own meshes (tests/tsdf_oracle.py) are closed,
consistently oriented surfaces of the right topology, ``save_mesh_ply`` writes what a PLY reader parses back, and every
argument error of ``TSDFVolume`` / ``save_mesh_ply`` / ``fuse_scene`` is raised before anything touches a device.
(The C-ABI of the three new entry points is covered by the generic tests/test_abi.py.)"""
import ctypes

import numpy as np
import pytest
import torch

from taichi_splatting_amd import TSDFVolume, TriangleMesh, fuse_scene, save_mesh_ply, _lib
from tests import tsdf_oracle as to

H = 0.25


def oracle_mesh(field, origin=(-2.5, -2.5, -2.5), dims=(21, 21, 21)):
  positions = to.grid_positions(origin, H, dims)
  values = field(positions)
  return to.marching_tetrahedra(values, np.ones_like(values), origin, H)


@pytest.fixture(scope='module')
def sphere():
  return oracle_mesh(lambda p: to.sphere_field(p, (0.03, -0.02, 0.01), 6.3 * H))


def closed_and_oriented(faces):
  _, counts = to.undirected_edges(faces)
  assert counts.size > 0 and (counts == 2).all()                 # every edge in exactly two triangles
  assert (to.directed_edge_multiplicities(faces) == 1).all()     # ... once in each direction


def test_sphere_is_a_closed_oriented_surface_of_genus_zero(sphere):
  vertices, faces, _ = sphere
  closed_and_oriented(faces)
  assert to.euler_characteristic(faces) == 2
  radius = 6.3 * H
  volume = to.signed_volume(vertices, faces)
  assert volume > 0
  # linear interpolation of a distance function along a segment of at most sqrt(3) h whose curvature is at most
  # 1 / (R - sqrt(3) h): the bound of tests/test_gpu_tsdf.py
  bound = 3 * H * H / (8 * (radius - np.sqrt(3) * H))
  error = np.abs(np.linalg.norm(vertices - np.array([0.03, -0.02, 0.01]), axis=1) - radius)
  assert error.max() <= bound
  assert 4 / 3 * np.pi * (radius - bound) ** 3 <= volume <= 4 / 3 * np.pi * (radius + bound) ** 3
  # vertices in (owner, edge type) order and faces in cell order: both are produced sorted
  assert faces.min() == 0 and faces.max() == vertices.shape[0] - 1


def test_torus_has_euler_characteristic_zero():
  vertices, faces, _ = oracle_mesh(lambda p: to.torus_field(p, (0.02, 0.01, -0.03), 1.5, 0.6), dims=(21, 21, 21))
  closed_and_oriented(faces)
  assert to.euler_characteristic(faces) == 0
  assert to.signed_volume(vertices, faces) > 0


def test_two_disjoint_spheres_have_euler_characteristic_four():
  field = lambda p: np.minimum(to.sphere_field(p, (-1.2, 0.01, 0.02), 0.9), to.sphere_field(p, (1.2, -0.03, 0.04), 0.8))
  vertices, faces, _ = oracle_mesh(field)
  closed_and_oriented(faces)
  assert to.euler_characteristic(faces) == 4
  assert to.signed_volume(vertices, faces) > 0


def test_all_256_sign_patterns_give_locally_consistent_triangles():
  """every cell pattern on its own: no edge in more than two triangles, no directed edge twice, and the 254 mixed
  patterns all emit"""
  tsdf, weight = to.all_sign_patterns()
  vertices, faces, _ = to.marching_tetrahedra(tsdf, weight, (0, 0, 0), 1.0)
  assert (to.undirected_edges(faces)[1] <= 2).all() and (to.directed_edge_multiplicities(faces) == 1).all()
  cells = set((np.floor(vertices[faces[:, 0], 0] / 3).astype(int) + 16 * np.floor(vertices[faces[:, 0], 1] / 3).astype(int)).tolist())
  assert cells == set(range(1, 255))


def test_tet_cases_cover_sixteen_patterns():
  counts = [len(to.tet_triangles([bool(m >> v & 1) for v in range(4)])) for m in range(16)]
  assert counts == [0, 1, 1, 2, 1, 2, 2, 1, 1, 2, 2, 1, 2, 1, 1, 0]
  assert len(to.TETRAHEDRA) == 6 and to.TETRAHEDRA[0] == [(0, 0, 0), (1, 0, 0), (1, 1, 0), (1, 1, 1)]
  assert to.TETRAHEDRA[5] == [(0, 0, 0), (0, 0, 1), (0, 1, 1), (1, 1, 1)]


def parse_ply(path):
  data = open(path, 'rb').read()
  end = data.index(b'end_header\n') + len(b'end_header\n')
  header = data[:end].decode('ascii').splitlines()
  assert header[0] == 'ply' and header[1] == 'format binary_little_endian 1.0'
  elements, current = [], None
  for line in header[2:-1]:
    words = line.split()
    if words[0] == 'element':
      current = (words[1], int(words[2]), [])
      elements.append(current)
    else:
      assert words[0] == 'property'
      current[2].append(words[1:])
  return elements, data[end:]


def test_save_mesh_ply_round_trip(tmp_path, sphere):
  vertices, faces, _ = sphere
  colours = torch.rand((vertices.shape[0], 3), generator=torch.Generator().manual_seed(1))
  colours[0] = torch.tensor([-1.0, 2.0, float('nan')])
  mesh = TriangleMesh(torch.from_numpy(vertices).float(), torch.from_numpy(faces).int(), colours)
  for coloured in (True, False):
    path = tmp_path / f'mesh_{coloured}.ply'
    save_mesh_ply(mesh if coloured else TriangleMesh(mesh.vertices, mesh.faces), path)
    elements, body = parse_ply(path)
    assert [e[0] for e in elements] == ['vertex', 'face'] and elements[0][1] == vertices.shape[0] and elements[1][1] == faces.shape[0]
    names = [p[-1] for p in elements[0][2]]
    assert names == (['x', 'y', 'z', 'red', 'green', 'blue'] if coloured else ['x', 'y', 'z'])
    assert elements[1][2] == [['list', 'uchar', 'int', 'vertex_indices']]
    vertex_type = np.dtype([('p', '<f4', (3,))] + ([('c', 'u1', (3,))] if coloured else []))
    face_type = np.dtype([('n', 'u1'), ('v', '<i4', (3,))])
    assert len(body) == vertex_type.itemsize * vertices.shape[0] + face_type.itemsize * faces.shape[0]
    v = np.frombuffer(body, dtype=vertex_type, count=vertices.shape[0])
    f = np.frombuffer(body, dtype=face_type, offset=vertex_type.itemsize * vertices.shape[0])
    assert np.array_equal(v['p'], vertices.astype(np.float32)) and (f['n'] == 3).all() and np.array_equal(f['v'], faces)
    if coloured:
      assert v['c'][0].tolist() == [0, 255, 0]
      assert np.array_equal(v['c'][1:], np.round(colours[1:].numpy() * 255).astype(np.uint8))
  empty = tmp_path / 'empty.ply'
  save_mesh_ply(TriangleMesh(torch.zeros((0, 3)), torch.zeros((0, 3), dtype=torch.int32)), empty)
  elements, body = parse_ply(empty)
  assert elements[0][1] == 0 and elements[1][1] == 0 and body == b''


def test_save_mesh_ply_argument_errors(tmp_path):
  ok = TriangleMesh(torch.zeros((3, 3)), torch.tensor([[0, 1, 2]], dtype=torch.int32))
  with pytest.raises(TypeError):
    save_mesh_ply((ok.vertices, ok.faces), tmp_path / 'a.ply')
  with pytest.raises(ValueError):
    save_mesh_ply(TriangleMesh(torch.zeros((3, 2)), ok.faces), tmp_path / 'a.ply')
  with pytest.raises(ValueError):
    save_mesh_ply(TriangleMesh(ok.vertices, torch.tensor([[0, 1, 3]], dtype=torch.int32)), tmp_path / 'a.ply')
  with pytest.raises(TypeError):
    save_mesh_ply(TriangleMesh(ok.vertices, ok.faces.float()), tmp_path / 'a.ply')
  with pytest.raises(ValueError):
    save_mesh_ply(TriangleMesh(ok.vertices, ok.faces, torch.zeros((2, 3))), tmp_path / 'a.ply')
  assert not (tmp_path / 'a.ply').exists()


@pytest.mark.parametrize('kwargs, error', [
  (dict(dims=(0, 4, 4)), ValueError), (dict(dims=(4, 4)), ValueError), (dict(dims=(4, -1, 4)), ValueError),
  (dict(dims=(513, 512, 512)), ValueError), (dict(dims=(1 << 14, 1 << 14, 1)), ValueError),
  (dict(dims=(4.5, 4, 4)), TypeError), (dict(dims=(True, 4, 4)), TypeError), (dict(dims=4), TypeError),
  (dict(origin=(0, 0)), ValueError), (dict(origin=(0, 0, float('nan'))), ValueError), (dict(origin=(0, 0, float('inf'))), ValueError),
  (dict(origin=('a', 0, 0)), TypeError), (dict(origin=None), TypeError),
  (dict(voxel_size=0.0), ValueError), (dict(voxel_size=-1.0), ValueError), (dict(voxel_size=float('nan')), ValueError),
  (dict(voxel_size=float('inf')), ValueError), (dict(voxel_size=1e39), ValueError), (dict(voxel_size='x'), TypeError),
  (dict(truncation=0.0), ValueError), (dict(truncation=-0.5), ValueError), (dict(truncation=float('inf')), ValueError),
  (dict(max_weight=0.0), ValueError), (dict(max_weight=-3.0), ValueError), (dict(max_weight=float('nan')), ValueError),
])
def test_volume_argument_errors_come_before_any_allocation(kwargs, error):
  args = dict(origin=(0.0, 0.0, 0.0), voxel_size=0.1, dims=(4, 4, 4))
  args.update(kwargs)
  with pytest.raises(error):
    TSDFVolume(**args)


def test_volume_is_gpu_only():
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    TSDFVolume((0, 0, 0), 0.1, (4, 4, 4), device='cpu')


def test_fuse_scene_argument_errors():
  with pytest.raises(TypeError):
    fuse_scene(None, [], None, object())


def test_entry_points_check_their_arguments(lib):
  """host-side checks of the three C calls, before any launch (no GPU needed)"""
  origin = (ctypes.c_double * 3)(0.0, 0.0, 0.0)
  inf = float('inf')
  good = dict(tsdf=16, weight=32, colour=None, nx=4, ny=4, nz=4, origin=origin, voxel=0.1, trunc=0.4, maxw=inf, depth=4,
              pw=None, image=None, cams=8, c=1, w=8, h=8)
  def integrate(**kw):
    a = dict(good)
    a.update(kw)
    return lib.ms_tsdf_integrate(a['tsdf'], a['weight'], a['colour'], a['nx'], a['ny'], a['nz'], a['origin'], a['voxel'],
                                 a['trunc'], a['maxw'], a['depth'], a['pw'], a['image'], a['cams'], a['c'], a['w'], a['h'], None)
  for bad in (dict(nx=0), dict(nx=1 << 14, ny=1 << 14), dict(nx=513, ny=512, nz=512), dict(voxel=0.0), dict(voxel=float('nan')),
              dict(trunc=-1.0), dict(maxw=0.0), dict(maxw=float('nan')), dict(c=0), dict(c=65536), dict(w=0), dict(h=-1),
              dict(tsdf=None), dict(depth=None), dict(cams=None), dict(tsdf=20), dict(weight=36), dict(depth=6),
              dict(colour=48), dict(image=4), dict(colour=40, image=4), dict(origin=None)):
    assert integrate(**bad) == -1, bad
  assert b'ms_tsdf_integrate' in lib.ms_last_error_string()
  assert lib.ms_tsdf_classify(4, 4, 0, 1, 1, 0.0, 4, 4, 4, None) == -1
  assert lib.ms_tsdf_classify(4, 4, 2, 2, 2, float('nan'), 4, 4, 4, None) == -1
  assert lib.ms_tsdf_classify(4, None, 2, 2, 2, 0.0, 4, 4, 4, None) == -1
  assert lib.ms_tsdf_classify(4, 4, 2, 2, 2, 0.0, 4, 6, 4, None) == -1
  assert lib.ms_tsdf_emit(4, 4, None, 2, 2, 2, origin, 0.1, 0.0, 4, 4, 4, None, 4, None, None) == -1
  assert lib.ms_tsdf_emit(4, 4, None, 2, 2, 2, origin, 0.1, 0.0, 4, 4, 4, 4, 4, 4, None) == -1       # colours of a plain volume
  assert lib.ms_tsdf_emit(4, 4, None, 2, 2, 2, origin, -0.1, 0.0, 4, 4, 4, 4, 4, None, None) == -1
  assert lib.ms_tsdf_emit(4, 4, None, 1 << 10, 1 << 10, 1 << 10, origin, 0.1, 0.0, 4, 4, 4, 4, 4, None, None) == -1
  assert _lib.TSDF_MAX_SAMPLES == 1 << 27 and _lib.TSDF_RUN == 4 and _lib.TSDF_CAMERA_CHUNK == 64
