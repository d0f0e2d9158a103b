"""The simplification oracle against an independent implementation, and the host side of ``simplify_mesh`` (no GPU).

tests/mesh_simplify_oracle.py is what tests/test_gpu_mesh_simplify.py compares the kernels with.  Here its clusters, faces
and positions are checked against a brute-force form that shares no code with it: clusters from a dictionary of cell
tuples, faces by a loop, and the position of a cluster as the ``numpy.linalg.lstsq`` solution of the stacked system
[m_i^T ; sqrt(lambda) I] y = [-d_i ; 0] — the least-squares statement of the PLACEMENT RULE — instead of the normal
equations.  The figures the feature was proposed with (output sizes, quadric share, closest optimum to a cell face,
largest condition number) are re-derived on the two meshes the GPU tests use.
"""
import numpy as np
import pytest
import torch

from taichi_splatting_amd import TriangleMesh, simplify_mesh
from taichi_splatting_amd import mesh as tm
from tests import mesh_simplify_oracle as so

SPHERE_ORIGIN = (-1.01, -1.02, -1.03)
CUBE_ORIGIN = (-0.02, -0.02, -0.02)


def brute_force(vertices, faces, cell_size, origin, regularisation=1e-3):
  """-> (cells in ascending key order -> unrounded quadric position or None, mean), kept faces as cell-tuple triples"""
  vertices = np.asarray(vertices, dtype=np.float32)
  origin32, size32 = np.asarray(origin, dtype=np.float32), np.float32(cell_size)
  cell_of = {}
  for v in sorted(set(int(i) for i in faces.reshape(-1))):
    q = np.floor((vertices[v] - origin32) / size32)
    cell_of[v] = (int(q[2]), int(q[1]), int(q[0]))                       # (z, y, x): tuple order = key order
  clusters = {}
  for v, cell in cell_of.items():
    clusters.setdefault(cell, []).append(v)
  order = sorted(clusters)
  rank = {cell: i for i, cell in enumerate(order)}
  kept, seen = [], set()
  for f in faces.tolist():
    t = [rank[cell_of[v]] for v in f]
    if len(set(t)) < 3:
      continue
    k = t.index(min(t))
    t = tuple(t[k:] + t[:k])
    if t not in seen:
      seen.add(t)
      kept.append(t)
  positions = {}
  p64 = vertices.astype(np.float64)
  for cell in order:
    members = clusters[cell]
    mean = p64[members].mean(axis=0)
    rows, rhs = [], []
    for f in faces.tolist():
      for v in f:
        if cell_of[v] == cell:
          a, b, c = p64[f[0]], p64[f[1]], p64[f[2]]
          m = np.cross(b - a, c - a)
          rows.append(m)
          rhs.append(m @ (a - mean))                                  # = -d
    trace = sum(float(m @ m) for m in rows)
    quadric = None
    if trace > 0:
      weight = np.sqrt(regularisation * trace / 3.0)
      system = np.vstack(rows + [weight * np.eye(3)])
      y = np.linalg.lstsq(system, np.asarray(rhs + [0.0, 0.0, 0.0]), rcond=None)[0]
      quadric = mean + y
    positions[cell] = (quadric, mean)
  return order, positions, kept


def check_against_brute_force(vertices, faces, cell_size, origin):
  got = so.simplify(vertices, faces, cell_size, origin)
  order, positions, kept = brute_force(vertices, faces, cell_size, origin)
  used = sorted(set(i for t in kept for i in t))
  assert got['vertices'].shape[0] == len(used) and got['faces'].shape[0] == len(kept)
  remap = {c: i for i, c in enumerate(used)}
  assert got['faces'].tolist() == [[remap[i] for i in t] for t in kept]
  assert [tuple(int(x) for x in c[::-1]) for c in got['cell']] == [order[c] for c in used]
  for i, c in enumerate(used):
    quadric, mean = positions[order[c]]
    assert np.allclose(got['mean'][i], mean, rtol=0, atol=1e-6)
    if got['choice'][i] == so.QUADRIC:
      # two float64 solutions of one well-conditioned system (<= 3001) on positions of order 1
      assert np.abs(got['vertices'][i] - quadric).max() <= 2.0 ** -22, (i, got['vertices'][i], quadric)
  return got


@pytest.fixture(scope='module')
def sphere():
  vertices, faces = so.icosphere(4)
  assert vertices.shape == (2562, 3) and faces.shape == (5120, 3)
  assert np.allclose(np.linalg.norm(vertices.astype(np.float64), axis=1), 1.0, atol=1e-6)
  return vertices, faces


@pytest.fixture(scope='module')
def cube():
  vertices, faces = so.cube_surface(12)
  assert vertices.shape == (866, 3) and faces.shape == (1728, 3)
  return vertices, faces


def outward(vertices, faces, centre):
  p = vertices.astype(np.float64)
  normal = np.cross(p[faces[:, 1]] - p[faces[:, 0]], p[faces[:, 2]] - p[faces[:, 0]])
  return bool((np.einsum('ij,ij->i', normal, p[faces].mean(axis=1) - centre) > 0).all())


def test_the_builders_make_closed_outward_surfaces(sphere, cube):
  for (vertices, faces), centre in ((sphere, 0.0), (cube, 0.5)):
    assert outward(vertices, faces, centre)
    edges = np.sort(np.concatenate([faces[:, [0, 1]], faces[:, [1, 2]], faces[:, [2, 0]]]), axis=1)
    _, counts = np.unique(edges, axis=0, return_counts=True)
    assert (counts == 2).all()                                         # closed and manifold
    assert vertices.shape[0] - edges.shape[0] // 2 + faces.shape[0] == 2


@pytest.mark.parametrize('cell_size, num_vertices, num_faces, quadric, condition', [(0.25, 276, 550, 274, 877.0),
                                                                                   (0.20, 401, 810, 399, 899.0)])
def test_the_sphere_against_brute_force(sphere, cell_size, num_vertices, num_faces, quadric, condition):
  got = check_against_brute_force(*sphere, cell_size, SPHERE_ORIGIN)
  assert got['vertices'].shape[0] == num_vertices and got['faces'].shape[0] == num_faces
  share = float((got['choice'] == so.QUADRIC).mean())
  closest = float(np.abs(got['margin']).min())
  print(f"sphere, cell {cell_size}: quadric share {share:.4f}, closest optimum to a cell face {closest:.2e} of a cell, "
        f"largest condition number {got['condition'].max():.0f}, largest error bound / cell ulp "
        f"{(got['error_bound'][:, None] / got['cell_ulp']).max():.3f}")
  assert int((got['choice'] == so.QUADRIC).sum()) == quadric and int((got['choice'] == so.MEAN).sum()) == num_vertices - quadric
  assert closest > 10 * so.FLIP_MARGIN                                 # no cluster of these two cases can flip
  assert got['condition'].max() <= 1.0 + 3.0 / 1e-3 + 1e-6 and abs(got['condition'].max() / condition - 1.0) < 0.01
  assert (got['error_bound'][:, None] < 0.25 * got['cell_ulp']).all()
  # every vertex is in its own cell; the mean of points ON the sphere lies inside it, the quadric position need not
  assert np.array_equal(so.cells(got['vertices'], SPHERE_ORIGIN, cell_size).astype(np.int64), got['cell'])
  radius = np.linalg.norm(got['vertices'].astype(np.float64), axis=1)
  mean_radius = np.linalg.norm(so.simplify(*sphere, cell_size, SPHERE_ORIGIN, placement='mean')['vertices'].astype(np.float64), axis=1)
  assert np.abs(radius - 1).max() < 0.01 and mean_radius.max() <= 1 + 1e-7 and mean_radius.min() > 0.99


def test_the_cube_against_brute_force(cube):
  got = check_against_brute_force(*cube, 0.26, CUBE_ORIGIN)
  assert got['vertices'].shape[0] == 56 and got['faces'].shape[0] == 108
  assert (got['choice'] == so.QUADRIC).all()
  assert abs(got['condition'].max() - 3001.0) < 1e-3                   # 1 + 3 / regularisation: a flat cluster
  assert (got['error_bound'][:, None] < 0.25 * got['cell_ulp']).all()
  corner = np.linalg.norm(got['vertices'].astype(np.float64), axis=1).argmin()
  mean = so.simplify(*cube, 0.26, CUBE_ORIGIN, placement='mean')
  assert np.array_equal(mean['faces'], got['faces']) and (mean['choice'] == so.MEAN).all()
  quadric_distance = float(np.abs(got['vertices'][corner]).max())      # per axis; the corner is (0, 0, 0)
  mean_distance = float(np.abs(mean['vertices'][corner]).max())
  print(f"cube corner: quadric {quadric_distance:.2e} from the corner per axis, mean {mean_distance:.3f}")
  assert quadric_distance < 1e-4 and 0.05 < mean_distance < 0.08 and mean_distance > 500 * quadric_distance


def test_the_oracle_is_idempotent_and_stable(sphere):
  vertices, faces = sphere
  colours = np.random.default_rng(0).random(vertices.shape).astype(np.float32)
  once = so.simplify(vertices, faces, 0.25, SPHERE_ORIGIN, colours=colours)
  assert once['colours'].shape == once['vertices'].shape and once['colours'].min() > 0 and once['colours'].max() < 1
  twice = so.simplify(once['vertices'], once['faces'], 0.25, SPHERE_ORIGIN)
  assert np.array_equal(twice['faces'], once['faces']) and twice['vertices'].shape == once['vertices'].shape
  assert (once['vertex_map'][faces] >= 0).all()
  padded = np.concatenate([np.full((2, 3), np.nan, dtype=np.float32), vertices])       # unreferenced, not even finite
  shifted = so.simplify(padded, faces + 2, 0.25, SPHERE_ORIGIN)
  assert np.array_equal(shifted['faces'], once['faces']) and np.array_equal(shifted['vertices'], once['vertices'])
  assert shifted['vertex_map'][:2].tolist() == [-1, -1]
  assert np.array_equal(so.default_origin(padded), vertices.min(axis=0))
  zeros = np.array([(0.0, -0.0, 1.0), (-0.0, 0.0, 2.0), (3.0, 0.0, -0.0), (-1.0, 5.0, 0.0)], dtype=np.float32)
  assert so.default_origin(zeros).view(np.int32).tolist() == [np.float32(-1).view(np.int32), -2 ** 31, -2 ** 31]      # -0 below +0
  assert so.default_origin(np.abs(zeros)).view(np.int32).tolist() == [0, 0, 0]


def test_the_rules_on_cases_small_enough_to_state_by_hand():
  # cells of side 1 from the origin: vertices 0, 1 in cell (0,0,0), 2 in (1,0,0), 3 in (0,1,0), 4 in (0,0,1); 5 is loose
  vertices = np.array([(0.25, 0.25, 0.25), (0.5, 0.5, 0.5), (1.5, 0.5, 0.5), (0.5, 1.0, 0.5), (0.5, 0.5, 1.5), (9, 9, 9)], dtype=np.float32)
  faces = np.array([(2, 3, 0), (1, 2, 3), (3, 2, 1), (0, 1, 2), (4, 3, 2), (3, 1, 2)], dtype=np.int32)
  got = so.simplify(vertices, faces, 1.0, (0, 0, 0))
  # keys: (0,0,0) < (1,0,0) < (0,1,0) < (0,0,1) -> clusters 0 .. 3; vertex 3 sits ON a cell face and goes to the upper cell
  assert got['cell'].tolist() == [[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]]
  assert got['vertex_map'].tolist() == [0, 0, 1, 2, 3, -1]
  # (2,3,0) -> (1,2,0) -> rotated (0,1,2); (1,2,3) -> (0,1,2): a duplicate, the lower index survives; (3,2,1) -> (2,1,0) ->
  # (0,2,1): the opposite orientation stays; (0,1,2) collapses; (4,3,2) -> (3,2,1) -> (1,3,2); (3,1,2) -> (2,0,1) -> (0,1,2) again
  assert got['faces'].tolist() == [[0, 1, 2], [0, 2, 1], [1, 3, 2]]
  for bad in ([(0, 1, 6)], [(0, -1, 2)]):
    with pytest.raises(ValueError, match="outside"):
      so.simplify(vertices, bad, 1.0, (0, 0, 0))
  with pytest.raises(ValueError, match="not finite"):
    so.simplify(np.array([(0, 0, 0), (1, 1, np.nan), (2, 2, 2)], dtype=np.float32), [(0, 1, 2)], 1.0)
  with pytest.raises(ValueError, match="cell outside"):
    so.simplify(np.array([(0, 0, 0), (1, 1, 1), (2.0 ** 21, 0, 0)], dtype=np.float32), [(0, 1, 2)], 1.0, (0, 0, 0))
  last = so.simplify(np.array([(0, 0, 0), (1, 1, 1), (2.0 ** 21 - 1, 0, 0)], dtype=np.float32), [(0, 1, 2)], 1.0, (0, 0, 0))
  assert last['cell'][:, 0].max() == so.MAX_CELL
  with pytest.raises(ValueError, match="cell outside"):
    so.simplify(vertices, faces, 1.0, (1, 0, 0))                       # a negative cell index
  inside = so.simplify(vertices[:5] * 0.1, [(0, 1, 2), (1, 2, 3), (2, 3, 4), (0, 4, 2)], 1.0, (0, 0, 0))     # one cell
  assert inside['vertices'].shape == (0, 3) and inside['faces'].shape == (0, 3) and (inside['vertex_map'] == -1).all()
  empty = so.simplify(np.zeros((0, 3), dtype=np.float32), np.zeros((0, 3), dtype=np.int32), 1.0)
  assert empty['vertices'].shape == (0, 3) and empty['vertex_map'].shape == (0,)


# ---- argument errors, before any device work -----------------------------------------------------------------------------

def test_argument_errors_raise_before_any_device_work():
  vertices, faces = so.cube_surface(2)
  mesh = TriangleMesh(vertices=torch.from_numpy(vertices), faces=torch.from_numpy(faces))     # on the CPU: never launched
  for bad in (0, 0.0, -1.0, float('nan'), float('inf'), 1e-60, 1e60, '0.1', None, True, torch.tensor(0.1)):
    with pytest.raises(ValueError, match="cell_size"):
      tm.simplify_mesh(mesh, bad)
  for bad in (0, 0.0, -1e-3, float('nan'), float('inf'), '1e-3', None, False):
    with pytest.raises(ValueError, match="regularisation"):
      tm.simplify_mesh(mesh, 0.1, regularisation=bad)
  for bad in ('Quadric', 'median', 0, None):
    with pytest.raises(ValueError, match="placement"):
      tm.simplify_mesh(mesh, 0.1, placement=bad)
  for bad in ((0, 0), (0, 0, 0, 0), 0.0, torch.zeros(2), torch.zeros(1, 3), (0, float('nan'), 0)):
    with pytest.raises(ValueError, match="origin"):
      tm.simplify_mesh(mesh, 0.1, origin=bad)
  with pytest.raises(ValueError, match="no CPU fallback"):             # every argument fine but the device
    tm.simplify_mesh(mesh, 0.1)
  with pytest.raises(ValueError, match="no CPU fallback"):
    tm.simplify_mesh(mesh, 0.1, origin=torch.zeros(3), placement='mean', regularisation=1.0, return_map=True)
  with pytest.raises(TypeError):
    tm.simplify_mesh((mesh.vertices, mesh.faces), 0.1)
  huge = TriangleMesh(torch.empty((4, 3), device='meta'), torch.empty((2 ** 31 // 3 + 1, 3), dtype=torch.int32, device='meta'))
  with pytest.raises(ValueError, match="2\\^31"):
    tm.simplify_mesh(huge, 0.1)


def test_render_scene_refuses_the_cell_size_without_a_mesh(tmp_path):
  import subprocess
  import sys
  from pathlib import Path
  tool = str(Path(__file__).resolve().parent.parent / 'tools' / 'render_scene.py')
  done = subprocess.run([sys.executable, tool, str(tmp_path / 'absent.ply'), '--mesh-cell-size', '0.1'], capture_output=True,
                        text=True, timeout=120)
  assert done.returncode != 0 and '--mesh-cell-size' in done.stderr and 'need --mesh' in done.stderr


def test_the_package_exports_simplify_mesh_and_the_header_states_its_rules():
  import taichi_splatting_amd as pkg
  from pathlib import Path
  assert pkg.simplify_mesh is tm.simplify_mesh is simplify_mesh and 'simplify_mesh' in pkg.__all__ and 'simplify_mesh' in tm.__all__
  header = (Path(__file__).resolve().parent.parent / 'include' / 'mi355_splat.h').read_text()
  for rule in ('CELL RULE', 'ORDER RULE', 'FACE RULE', 'PLACEMENT RULE'):
    assert rule in header
  from taichi_splatting_amd import _lib
  assert _lib.MESH_SIMPLIFY_MAX_CELL == so.MAX_CELL == tm.MAX_CELL
  assert (_lib.MESH_SIMPLIFY_QUADRIC, _lib.MESH_SIMPLIFY_MEAN, _lib.MESH_SIMPLIFY_MEMBER) == (so.QUADRIC, so.MEAN, so.MEMBER)
  new = [name for name in _lib.SIGNATURES if name.startswith('ms_mesh_simplify_')]
  assert len(new) == 10 and not any(_lib.POINTER(_lib.c_size_t) in _lib.SIGNATURES[name][1] for name in new)      # no scratch block
