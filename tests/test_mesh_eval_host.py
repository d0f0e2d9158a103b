"""What of the mesh evaluation needs no GPU: the sampler's numpy oracle against hand answers (tests/mesh_sample_oracle.py),
the arithmetic of SurfaceMetrics, load_points_ply, and the argument checks of the Python calls and of the three C entry
points (which come before any launch)."""
import ctypes
import math

import numpy as np
import pytest
import torch

from taichi_splatting_amd import (SurfaceMetrics, TriangleMesh, evaluate_mesh, load_points_ply, metrics_from_distances,
                                  sample_mesh_points, surface_distances, surface_metrics)
from taichi_splatting_amd.misc import knn_query
from taichi_splatting_amd.misc.knn import query_scratch_bytes
from tests import mesh_sample_oracle as so


def test_the_generator_against_known_answers():
  """evaluated with exact integer arithmetic (Python ints masked to 32 bits), independently of numpy"""
  assert int(so.mix(0)) == 0
  assert int(so.mix(1)) == 0x688990c0
  assert int(so.mix(0xdeadbeef)) == 0xe628c683
  assert int(so.word(0, 0, 0)) == 0xae6f80f1
  assert int(so.word(7, 12345, 2)) == 0x8fe0e284
  assert int(so.word(0xffffffff, 2 ** 31 - 1, 1)) == 0xa28c294b            # both additions wrap
  assert float(so.unit(0, 0, 0)) == 0xae6f80 / 2.0 ** 24
  # arrays, and the seed is taken modulo 2^32
  i = np.array([0, 12345, 2 ** 31 - 1], dtype=np.uint64)
  assert so.word(7, i, 2)[1] == 0x8fe0e284 and so.word(7 + 2 ** 32, i, 2)[1] == 0x8fe0e284
  u = so.unit(3, np.arange(100000, dtype=np.uint64), 1)
  assert u.min() >= 0.0 and u.max() < 1.0 and (u.astype(np.float32).astype(np.float64) == u).all()
  assert abs(u.mean() - 0.5) < 0.01


def test_triangle_areas_against_hand_answers():
  vertices = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [6, 0, 0], [1, 1, 1]], dtype=np.float32)
  faces = np.array([[0, 1, 2],          # right triangle with legs 3 and 4: area 6
                    [0, 1, 3],          # three points on a line: area 0
                    [4, 4, 4],          # one point three times: area 0
                    [2, 1, 0]])         # the first face reversed: the same area
  assert so.face_areas(vertices, faces).tolist() == [6.0, 0.0, 0.0, 6.0]
  unit = np.array([[0, 0, 0], [1, 0, 0], [0, 1, 0], [0, 0, 1]], dtype=np.float32)
  assert so.face_areas(unit, [[1, 2, 3]])[0] == pytest.approx(math.sqrt(3.0) / 2.0, rel=1e-15)      # equilateral, side sqrt(2)
  assert so.face_unit_normals(unit, [[1, 2, 3], [0, 0, 1]]).tolist()[1] == [0.0, 0.0, 0.0]
  assert so.face_unit_normals(unit, [[1, 2, 3]])[0] == pytest.approx([3 ** -0.5] * 3, rel=1e-15)


def test_the_sampling_oracle():
  """strata, the search over the cdf, the weights: properties that follow from the rules alone"""
  vertices = np.array([[0, 0, 0], [3, 0, 0], [0, 4, 0], [6, 0, 0], [0, 0, 2]], dtype=np.float32)
  faces = np.array([[0, 1, 3], [0, 1, 2], [4, 4, 4], [0, 2, 4], [0, 1, 3]])         # areas 0, 6, 0, 4, 0
  cdf = np.cumsum(so.face_areas(vertices, faces))
  assert cdf.tolist() == [0.0, 6.0, 6.0, 10.0, 10.0]
  n = 1000
  t = so.strata(cdf, n, seed=3)
  i = np.arange(n)
  assert (t >= i * (10.0 / n)).all() and (t <= (i + 1) * (10.0 / n)).all() and (t < 10.0).all()
  points, face, w = so.sample(vertices, faces, cdf, n, seed=3)
  assert set(face.tolist()) == {1, 3}                                      # a face of zero area is never drawn
  assert abs((face == 1).sum() - 600) < 2 and abs((face == 3).sum() - 400) < 2
  assert (w >= 0).all() and np.abs(w.sum(axis=1) - 1.0).max() <= 2.0 ** -23
  assert (np.abs(points[face == 1][:, 2]) == 0).all() and (points[face == 3][:, 0] == 0).all()      # in the faces' planes
  assert (points[face == 1][:, 0] / 3 + points[face == 1][:, 1] / 4 <= 1 + 1e-6).all()
  again = so.sample(vertices, faces, cdf, n, seed=3)
  assert np.array_equal(again[0], points) and not np.array_equal(so.sample(vertices, faces, cdf, n, seed=4)[0], points)
  # the last stratum is capped below the total even when u0 would round it up to the total
  assert so.strata(np.array([1.0]), 1, 0)[0] < 1.0
  f32 = so.combine_f32(vertices, faces, face, w.astype(np.float32))
  assert f32.dtype == np.float32 and np.abs(f32 - points).max() <= 4 * 2.0 ** -24 * 6.0


def test_surface_metrics_arithmetic():
  d_ab = torch.tensor([0.0, 1.0, 2.0, 5.0], dtype=torch.float32)
  d_ba = torch.tensor([0.5, 0.5, 3.0], dtype=torch.float32)
  m = metrics_from_distances(d_ab, d_ba, threshold=1.0)
  assert isinstance(m, SurfaceMetrics) and all(isinstance(v, float) for v in vars(m).values())
  assert m.accuracy == 2.0 and m.completeness == 4.0 / 3.0 and m.chamfer == (2.0 + 4.0 / 3.0) / 2.0
  assert m.precision == 0.5 and m.recall == 2.0 / 3.0                       # d <= threshold: the 1.0 counts
  assert m.fscore == pytest.approx(2 * 0.5 * (2 / 3) / (0.5 + 2 / 3), rel=1e-15)
  assert m.dropped_a == 0.0 and m.dropped_b == 0.0
  capped = metrics_from_distances(d_ab, d_ba, threshold=1.0, max_distance=2.0)
  assert capped.accuracy == 1.0 and capped.completeness == 0.5 and capped.chamfer == 0.75
  assert capped.dropped_a == 0.25 and capped.dropped_b == 1.0 / 3.0
  assert (capped.precision, capped.recall, capped.fscore) == (m.precision, m.recall, m.fscore)      # the cap does not touch them
  none = metrics_from_distances(d_ab + 1.0, d_ba + 1.0, threshold=0.25)
  assert none.precision == 0.0 and none.recall == 0.0 and none.fscore == 0.0      # P + R = 0: no division
  everything = metrics_from_distances(d_ab, d_ba, threshold=5.0)
  assert everything.precision == 1.0 and everything.recall == 1.0 and everything.fscore == 1.0
  gone = metrics_from_distances(d_ab + 1.0, d_ba, threshold=1.0, max_distance=0.75)
  assert math.isnan(gone.accuracy) and gone.dropped_a == 1.0 and gone.completeness == 0.5
  # float64 sums: a million float32 distances of 0.1 average to float32(0.1) within a few 2^-53
  many = torch.full((1_000_000,), 0.1, dtype=torch.float32)
  assert metrics_from_distances(many, many, 1.0).chamfer == pytest.approx(float(np.float32(0.1)), rel=1e-13)
  for bad in (dict(threshold=-1.0), dict(threshold=math.nan), dict(threshold='1'), dict(threshold=1.0, max_distance=-2.0)):
    with pytest.raises(ValueError):
      metrics_from_distances(d_ab, d_ba, **bad)
  with pytest.raises(ValueError, match="non-empty"):
    metrics_from_distances(d_ab[:0], d_ba, 1.0)
  with pytest.raises(ValueError, match="non-empty"):
    metrics_from_distances(d_ab, d_ba.reshape(3, 1), 1.0)


POINTS = np.array([[0.5, -1.25, 3.0], [1e-3, 2.5e4, -7.0], [0.0, 0.0, 0.0]], dtype=np.float64)
RGB = np.array([[255, 0, 51], [0, 102, 255], [1, 2, 3]], dtype=np.uint8)


def test_load_points_ply_ascii(tmp_path):
  path = tmp_path / 'cloud.ply'
  body = "".join(f"{p[0]!r} {p[1]!r} {p[2]!r} {c[0]} {c[1]} {c[2]} 0.5\n" for p, c in zip(POINTS.tolist(), RGB.tolist()))
  path.write_text("ply\nformat ascii 1.0\ncomment a scan\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                  "property uchar red\nproperty uchar green\nproperty uchar blue\nproperty float confidence\n"
                  "element face 1\nproperty list uchar int vertex_indices\nend_header\n" + body + "3 0 1 2\n")
  points, colours = load_points_ply(path)
  assert points.dtype == torch.float32 and points.device.type == 'cpu' and colours.dtype == torch.float32
  assert np.array_equal(points.numpy(), POINTS.astype(np.float32))
  assert np.array_equal(colours.numpy(), RGB.astype(np.float32) / np.float32(255.0))
  assert float(colours.max()) == 1.0 and float(colours.min()) == 0.0


def test_load_points_ply_binary(tmp_path):
  # properties out of order, a double coordinate, an extra column between them
  row = np.dtype([('green', 'u1'), ('z', '<f4'), ('x', '<f8'), ('intensity', '<u2'), ('red', 'u1'), ('y', '<f4'), ('blue', 'u1')])
  data = np.zeros((3,), dtype=row)
  data['x'], data['y'], data['z'] = POINTS[:, 0], POINTS[:, 1], POINTS[:, 2]
  data['red'], data['green'], data['blue'] = RGB[:, 0], RGB[:, 1], RGB[:, 2]
  data['intensity'] = 40000
  header = ("ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty uchar green\nproperty float z\nproperty double x\n"
            "property ushort intensity\nproperty uchar red\nproperty float y\nproperty uchar blue\nend_header\n")
  path = tmp_path / 'cloud.ply'
  path.write_bytes(header.encode('ascii') + data.tobytes())
  points, colours = load_points_ply(path, chunk_rows=2)                   # two slabs
  assert np.array_equal(points.numpy(), POINTS.astype(np.float32))
  assert np.array_equal(colours.numpy(), RGB.astype(np.float32) / np.float32(255.0))

  # without colours (all float32: the memory-mapped path), and a float `red` is not a colour
  plain = tmp_path / 'plain.ply'
  plain.write_bytes(b"ply\nformat binary_little_endian 1.0\nelement vertex 3\nproperty float x\nproperty float y\nproperty float z\n"
                    b"property float red\nend_header\n" + np.concatenate([POINTS, np.ones((3, 1))], axis=1).astype('<f4').tobytes())
  points, colours = load_points_ply(plain)
  assert colours is None and np.array_equal(points.numpy(), POINTS.astype(np.float32))

  for name, text, match in (
      ('big.ply', "ply\nformat binary_big_endian 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n", "big_endian"),
      ('noz.ply', "ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nend_header\n", "missing required property z"),
      ('int.ply', "ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty int y\nproperty float z\nend_header\n", "integer type"),
      ('short.ply', "ply\nformat binary_little_endian 1.0\nelement vertex 5\nproperty float x\nproperty float y\nproperty float z\nend_header\n", "shorter"),
  ):
    bad = tmp_path / name
    bad.write_text(text)
    with pytest.raises(ValueError, match=match):
      load_points_ply(bad)
  empty = tmp_path / 'empty.ply'
  empty.write_text("ply\nformat ascii 1.0\nelement vertex 0\nproperty float x\nproperty float y\nproperty float z\nend_header\n")
  points, colours = load_points_ply(empty)
  assert points.shape == (0, 3) and colours is None


def triangle():
  return TriangleMesh(vertices=torch.tensor([[0.0, 0, 0], [1, 0, 0], [0, 1, 0]]), faces=torch.tensor([[0, 1, 2]], dtype=torch.int32))


def test_arguments_that_need_no_gpu():
  mesh = triangle()
  for kw in (dict(), dict(n=10, density=2.0), dict(n=0), dict(n=-3), dict(n=2.5), dict(n=True), dict(n=2 ** 31), dict(density=0.0),
             dict(density=-1.0), dict(density=math.inf), dict(density='3'), dict(n=10, seed=1.5)):
    with pytest.raises(ValueError):
      sample_mesh_points(mesh, **kw)
  with pytest.raises(TypeError):
    sample_mesh_points((mesh.vertices, mesh.faces), n=10)
  with pytest.raises(RuntimeError, match="no CPU fallback"):                # a valid request, on the CPU
    sample_mesh_points(mesh, n=10)
  cloud = torch.zeros((4, 3))
  for call in (surface_distances, lambda a, b: surface_metrics(a, b, 0.1), lambda a, b: evaluate_mesh(mesh, b, 0.1, n=5)):
    with pytest.raises(ValueError, match=r"\(N, 3\)|empty"):
      call(cloud, torch.zeros((4, 2)))
    with pytest.raises(ValueError, match=r"\(N, 3\)|empty"):
      call(cloud, torch.zeros((0, 3)))
  with pytest.raises(ValueError, match="threshold"):
    surface_metrics(cloud, cloud, -0.5)
  with pytest.raises(ValueError, match="threshold"):
    evaluate_mesh(mesh, cloud, None, n=5)
  with pytest.raises(ValueError, match="k must be"):
    knn_query(cloud, cloud, 9)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    knn_query(cloud, cloud)


def test_the_c_entry_points_check_their_arguments(lib):
  size = ctypes.c_size_t(12345)
  query = lambda m, n, k, tmp=None, size_ref=ctypes.byref(size): lib.ms_knn_query(None, None, m, None, None, None, n, k, None,
                                                                                  None, None, tmp, size_ref, None)
  up = lambda nbytes: -(-nbytes // 256) * 256          # rows of 16 bytes, then two arrays of one 16-byte box per 256 points
  assert query(1000, 10, 1) == 0 and size.value == up(1000 * 16) + 2 * up(4 * 16)
  assert query(0, 10, 8) == 0 and size.value == 0
  assert query(257, 0, 8) == 0 and size.value == up(257 * 16) + 2 * up(2 * 16)
  assert query_scratch_bytes(257, 5) == size.value
  for m, n, k, word in ((-1, 1, 1, b'm < 0'), (1, -1, 1, b'n < 0'), (2 ** 31, 1, 1, b'2^31'), (1, 2 ** 31, 1, b'2^31'),
                        (1, 1, 0, b'k must'), (1, 1, 9, b'k must')):
    assert query(m, n, k) == -1 and word in lib.ms_last_error_string(), (m, n, k)
  # the sizes pinned as literals, as tests/test_scratch_sizes_host.py pins every other entry point's (its table is closed to
  # new rows): the layout is that of ms_knn_points over the M points, whatever N and k
  counts = (0, 1, 15, 16, 17, 255, 256, 257, 4096, 4097, 100000)
  pinned = [0, 768, 768, 768, 1024, 4608, 4608, 4864, 66048, 66816, 1612800]
  for n, k in ((0, 1), (1, 3), (1000000, 8)):
    got = []
    for m in counts:
      assert query(m, n, k) == 0
      got.append(size.value)
    assert got == pinned, (n, k, got)
  # the protocol: a null tmp_bytes is MS_ERR_BAD_ARG, a short block MS_ERR_TMP_TOO_SMALL with the one message text, and a
  # run never writes the size back
  block = (ctypes.c_char * 4096)()
  for m, need in zip(counts, pinned):
    assert query(m, 10, 1, None, None) == -1 and b'tmp_bytes' in lib.ms_last_error_string()
    assert query(m, 10, 1, ctypes.addressof(block), None) == -1
    for short in ({0, need - 1} if need else ()):
      small = ctypes.c_size_t(short)
      assert query(m, 10, 1, ctypes.addressof(block), ctypes.byref(small)) == -3, (m, short)
      assert b'ms_knn_query: tmp_bytes too small' in lib.ms_last_error_string() and small.value == short
  big = ctypes.c_size_t(4096)
  assert query(10, 0, 1, ctypes.addressof(block), ctypes.byref(big)) == 0   # no queries: returns before the pointers
  assert query(10, 10, 1, ctypes.addressof(block), ctypes.byref(big)) == -1 and b'null' in lib.ms_last_error_string()

  assert lib.ms_mesh_face_areas(None, None, 0, 0, None, None, None) == -1 and b'status' in lib.ms_last_error_string()
  assert lib.ms_mesh_face_areas(None, None, -1, 0, None, 4, None) == -1
  assert lib.ms_mesh_face_areas(4, None, 3, 1, 8, 4, None) == -1 and b'faces' in lib.ms_last_error_string()
  assert lib.ms_mesh_face_areas(4, 4, 3, 1, 4, 4, None) == -1 and b'aligned' in lib.ms_last_error_string()
  sample = lambda v, t, n, points=4, colours=None, out_colours=None: lib.ms_mesh_sample_points(
    4, 4, colours, None, v, t, 8, n, 0, points, None, None, out_colours, None, None)
  assert sample(3, 1, 0) == 0                                               # nothing to do
  assert sample(3, 1, -1) == -1 and sample(3, 1, 2 ** 31) == -1
  assert sample(0, 1, 5) == -1 and sample(3, 0, 5) == -1 and b'no surface' in lib.ms_last_error_string()
  assert sample(3, 1, 5, points=None) == -1
  assert sample(3, 1, 5, out_colours=4) == -1 and b'out_colours' in lib.ms_last_error_string()
  assert sample(3, 1, 5, points=6) == -1 and b'aligned' in lib.ms_last_error_string()
