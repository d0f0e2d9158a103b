"""TSDF fusion and marching tetrahedra on the GPU (taichi_splatting_amd/fusion.py, csrc/tsdf.hip) against the float64
oracle of tests/tsdf_oracle.py.

Integration cases, by the path of the kernel they run (a lane owns 4 consecutive samples, a wave 256, a workgroup 1024):
  (1, 1, 1)      one sample: one lane on the scalar (partial run) path
  (3, 2, 5)      30 samples: runs that wrap rows and slices, a partial last run
  (64, 1, 1)     16 full runs in one row: the 16-byte path alone
  (65, 3, 2)     390 samples: two waves, rows that are no multiple of the run, a partial last run
  (33, 17, 9)    5049 samples: five workgroups, the last one ragged, a wave box that spans slices
  (16, 16, 4)    1024 samples: exactly one full workgroup
  (1025, 1, 1)   one full workgroup and a second one that holds a single sample
  (257, 2, 2)    1028 samples: a second workgroup of exactly one full run
with 5 x 7 and 64 x 48 images and C = 1, 2 and 65 frames (one more than the 64 cameras a wave culls per ballot).

The bound is the one tests/tsdf_oracle.py derives from the roundings (its docstring counts them): t carries
(2 eps |s| + 12 eps M_z) / truncation + 2 eps, with |s| <= |d| + |z| and M_z the magnitude of the terms of z; the running
mean is a convex combination and adds (4 + q / 2) eps at the q-th update.  Ill-posed samples (a decision within its own
rounding error of flipping) are left out; the oracle alone asserts they are under 1 % of every case.  Measured, as the
largest error over its bound, over all cases: the float32 torch composition on the CPU 0.062 (tsdf) and 0.222 (colour), the
kernel the same two figures — it takes the composition's operations in the composition's order.

Triangulation: K eps (|p| + voxel_size) with K = 8 — p_o and p_b carry 2 eps |p| each, their difference another eps h, l
two roundings, the product and the final sum one each; every test volume has a non-negative origin, so |o| + h i = |p|.
"""
import math

import numpy as np
import pytest
import torch

from taichi_splatting_amd import TSDFVolume, fuse_scene, pack_cameras
from tests import tsdf_oracle as to

pytestmark = pytest.mark.gpu
DEVICE = 'cuda:0'
EPS = to.EPS

DIMS = [(1, 1, 1), (3, 2, 5), (64, 1, 1), (65, 3, 2), (33, 17, 9), (16, 16, 4), (1025, 1, 1), (257, 2, 2)]
CASES = [(dims, (64, 48), 2, True, 1.5) for dims in DIMS] + [
  ((33, 17, 9), (5, 7), 1, True, None), ((33, 17, 9), (64, 48), 1, False, None), ((33, 17, 9), (5, 7), 65, True, 3.0),
  ((33, 17, 9), (5, 7), 65, False, 20.0), ((65, 3, 2), (5, 7), 65, False, None), ((3, 2, 5), (5, 7), 65, True, 3.0),
  ((1025, 1, 1), (64, 48), 1, False, None), ((16, 16, 4), (5, 7), 2, False, 1.0),
]


def volume_of(case, max_weight=None, colour=True):
  return TSDFVolume(case['origin'], case['voxel_size'], case['dims'], truncation=case['truncation'], colour=colour,
                    max_weight=max_weight, device=DEVICE)


def on_device(case):
  move = lambda t: None if t is None else t.to(DEVICE)
  return move(case['depth']), move(case['cameras']), move(case['image']), move(case['pixel_weight'])


def fresh(dims):
  nx, ny, nz = dims
  return torch.ones(nz, ny, nx), torch.zeros(nz, ny, nx), torch.zeros(nz, ny, nx, 3)


@pytest.mark.parametrize('dims, size, count, weighted, max_weight', CASES)
def test_integration_against_the_oracle(dims, size, count, weighted, max_weight):
  case = to.integration_case(dims, size, count, weighted=weighted)
  args = (case['origin'], case['voxel_size'], case['truncation'], max_weight, case['depth'], case['cameras'], case['image'],
          case['pixel_weight'])
  want_t, want_w, want_c, info = to.integrate(*fresh(dims), *args, analyse=True)
  ill = info['ill']
  assert float(ill.float().mean()) < 0.01, f"{float(ill.float().mean()):.4f} of the samples are ill-posed"
  good = ~ill
  n = good.numel()

  volume = volume_of(case, max_weight)
  depth, cameras, image, pixel_weight = on_device(case)
  assert volume.integrate(depth, cameras, colour=image, pixel_weight=pixel_weight) is volume
  composed = to.integrate(*fresh(dims), *args, dtype=torch.float32)
  results = {'kernel': (volume.tsdf.cpu(), volume.weight.cpu(), volume.colour.cpu()), 'float32 composition': composed}

  updated = info['updates'] > 0
  weight_bound = (info['updates'] + 1).double() * EPS * want_w.reshape(n)
  fractions = {}
  for name, (t, w, c) in results.items():
    err_t = (t.reshape(n).double() - want_t.reshape(n)).abs()
    err_c = (c.reshape(n, 3).double() - want_c.reshape(n, 3)).abs().amax(1)
    err_w = (w.reshape(n).double() - want_w.reshape(n)).abs()
    live = good & updated
    fractions[name] = (float((err_t[live] / info['bound'][live]).max()) if live.any() else 0.0,
                       float((err_c[live] / info['colour_bound'][live]).max()) if live.any() else 0.0)
    print(f"{dims} {size} C={count} {name}: largest tsdf error / bound {fractions[name][0]:.3f}, colour {fractions[name][1]:.3f}, "
          f"ill-posed {int(ill.sum())} of {n}, updated {int(updated.sum())}")
    assert bool((err_t[good] <= info['bound'][good]).all()), (name, float((err_t[good] - info['bound'][good]).max()))
    assert bool((err_c[good] <= info['colour_bound'][good]).all()), name
    if weighted:
      assert bool((err_w[good] <= weight_bound[good]).all()), name
    else:
      assert torch.equal(w.reshape(n)[good].double(), want_w.reshape(n)[good]), name            # unit weights: bit for bit
    untouched = good & ~updated
    assert bool((t.reshape(n)[untouched] == 1).all()) and bool((w.reshape(n)[untouched] == 0).all())
    assert bool((c.reshape(n, 3)[untouched] == 0).all())
  if max_weight is not None and count > 2:
    assert int((want_w == max_weight).sum()) > 0                      # the clamp is reached


def bits(t):
  return t.contiguous().view(torch.int32)


def test_skipped_samples_keep_their_bits():
  """a volume that lies half outside every frustum, one camera that sees none of it, and fields filled with arbitrary bit
  patterns (NaNs included): a sample the oracle does not update holds the same bits afterwards"""
  dims = (40, 24, 12)
  case = to.integration_case(dims, (64, 48), 3, weighted=True)
  cams = case['cameras'].clone()
  cams[:, 12:14] *= 2.5                                               # narrow frusta: much of the volume is outside
  away = to.look_at((6.0, 5.0, 4.0), (12.0, 10.0, 8.0))                # looks away from the volume
  cams[2] = to.pack_camera(away, 50.0, 52.0, 32.3, 23.8, 0.3, 10.0, 64, 48)
  generator = torch.Generator().manual_seed(3)
  nx, ny, nz = dims
  raw = torch.randint(-2 ** 31, 2 ** 31 - 1, (nz, ny, nx, 5), generator=generator, dtype=torch.int64).to(torch.int32)
  field = raw.view(torch.float32)
  tsdf0, colour0 = field[..., 0].contiguous(), field[..., 2:5].contiguous()
  weight0 = torch.rand((nz, ny, nx), generator=generator) * 4
  sane_t = torch.where(torch.isfinite(tsdf0) & (tsdf0.abs() < 1), tsdf0, torch.zeros_like(tsdf0))
  sane_c = torch.where(torch.isfinite(colour0) & (colour0.abs() < 1), colour0, torch.zeros_like(colour0))
  _, _, _, info = to.integrate(sane_t, weight0, sane_c, case['origin'], case['voxel_size'], case['truncation'], None,
                               case['depth'], cams, case['image'], case['pixel_weight'], analyse=True)
  skipped = (~info['ill'] & (info['updates'] == 0)).reshape(nz, ny, nx)
  assert 0.5 < float(skipped.float().mean()) < 0.99 and float(info['ill'].float().mean()) < 0.01
  volume = volume_of(case)
  volume.tsdf.copy_(tsdf0)
  volume.weight.copy_(weight0)
  volume.colour.copy_(colour0)
  depth, _, image, pixel_weight = on_device(case)
  volume.integrate(depth, cams.to(DEVICE), colour=image, pixel_weight=pixel_weight)
  assert torch.equal(bits(volume.tsdf).cpu()[skipped], bits(tsdf0)[skipped])
  assert torch.equal(bits(volume.weight).cpu()[skipped], bits(weight0)[skipped])
  assert torch.equal(bits(volume.colour).cpu()[skipped], bits(colour0)[skipped])
  changed = (bits(volume.weight).cpu() != bits(weight0))
  assert int(changed.sum()) > 0 and not bool((changed & skipped).any())
  # the camera that sees nothing, alone: the whole volume keeps its bits
  before = [bits(t).clone() for t in (volume.tsdf, volume.weight, volume.colour)]
  volume.integrate(depth[2], cams[2:3].to(DEVICE), colour=image[2], pixel_weight=pixel_weight[2])
  assert all(torch.equal(a, bits(t)) for a, t in zip(before, (volume.tsdf, volume.weight, volume.colour)))


def test_one_call_equals_single_frame_calls_and_runs_repeat():
  """C = 65 frames (two camera chunks) in one call, in 65 calls, in calls of 7, and once more: the same bits; reset
  restores the fresh state"""
  case = to.integration_case((33, 17, 9), (5, 7), 65, weighted=True)
  depth, cameras, image, pixel_weight = on_device(case)
  volumes = [volume_of(case, 6.0) for _ in range(4)]
  volumes[0].integrate(depth, cameras, colour=image, pixel_weight=pixel_weight)
  for c in range(65):
    volumes[1].integrate(depth[c], cameras[c:c + 1], colour=image[c], pixel_weight=pixel_weight[c])
  for c in range(0, 65, 7):
    volumes[2].integrate(depth[c:c + 7], cameras[c:c + 7], colour=image[c:c + 7], pixel_weight=pixel_weight[c:c + 7])
  volumes[3].integrate(depth, cameras, colour=image, pixel_weight=pixel_weight)
  assert float((volumes[0].weight > 0).float().mean()) > 0.5
  for other in volumes[1:]:
    for name in ('tsdf', 'weight', 'colour'):
      assert torch.equal(bits(getattr(volumes[0], name)), bits(getattr(other, name))), name
  assert volumes[0].reset() is volumes[0]
  assert bool((volumes[0].tsdf == 1).all()) and bool((volumes[0].weight == 0).all()) and bool((volumes[0].colour == 0).all())


def test_integrate_captures_into_a_graph():
  """packed cameras: no allocation, no synchronisation, no host read — two replays equal two eager calls bit for bit"""
  case = to.integration_case((33, 17, 9), (64, 48), 2, weighted=True)
  depth, cameras, image, pixel_weight = on_device(case)
  eager, captured = volume_of(case), volume_of(case)
  for _ in range(2):
    eager.integrate(depth, cameras, colour=image, pixel_weight=pixel_weight)
  torch.cuda.synchronize()
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    captured.integrate(depth, cameras, colour=image, pixel_weight=pixel_weight)
  captured.reset()                                                    # whatever the capture itself did or did not run
  graph.replay()
  graph.replay()
  torch.cuda.synchronize()
  for name in ('tsdf', 'weight', 'colour'):
    assert torch.equal(bits(getattr(eager, name)), bits(getattr(captured, name))), name
  assert float(eager.weight.max()) >= 2.0


def test_integrate_takes_camera_params_and_rejects_bad_arguments():
  from taichi_splatting_amd import CameraParams
  case = to.integration_case((9, 8, 7), (5, 7), 2, weighted=False)
  depth, packed, image, _ = on_device(case)
  cams = [CameraParams(projection=row[12:16].clone(), T_camera_world=torch.cat([row[:12].reshape(3, 4),
                       torch.tensor([[0.0, 0.0, 0.0, 1.0]], device=DEVICE)]), near_plane=float(row[16]), far_plane=float(row[17]),
                       image_size=(5, 7)) for row in packed]
  a, b = volume_of(case), volume_of(case)
  a.integrate(depth, packed, colour=image)
  b.integrate(depth, cams, colour=image)
  assert torch.equal(bits(a.tsdf), bits(b.tsdf)) and torch.equal(bits(a.colour), bits(b.colour))
  assert torch.equal(bits(pack_cameras(cams)), bits(packed))
  plain = volume_of(case, colour=False)
  plain.integrate(depth[0], cams[0])
  assert plain.colour is None and float(plain.weight.sum()) > 0
  with pytest.raises(ValueError):
    a.integrate(depth, packed)                                        # a coloured volume without colour images
  with pytest.raises(ValueError):
    plain.integrate(depth, packed, colour=image)
  with pytest.raises(ValueError):
    a.integrate(depth, packed[:1], colour=image)                      # 2 images, 1 camera
  with pytest.raises(ValueError):
    a.integrate(depth, packed, colour=image[:, :, :, :2])
  with pytest.raises(ValueError):
    a.integrate(depth, packed, colour=image, pixel_weight=depth[0])
  with pytest.raises(ValueError):
    a.integrate(depth, [cams[0], CameraParams(projection=cams[1].projection, T_camera_world=cams[1].T_camera_world,
                                              near_plane=0.1, far_plane=9.0, image_size=(6, 7))], colour=image)
  with pytest.raises(TypeError):
    a.integrate(depth.double(), packed, colour=image)
  with pytest.raises(TypeError):
    a.integrate(depth, 'cameras', colour=image)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    a.integrate(depth.cpu(), packed, colour=image)
  a.tsdf = a.tsdf[:, :, ::2]
  with pytest.raises(ValueError):
    a.integrate(depth, packed, colour=image)
  with pytest.raises(ValueError):
    a.extract_mesh()


# ---- triangulation -----------------------------------------------------------------------------------------------------

def extract(tsdf, weight, origin, voxel_size, min_weight=0.0, colour=None):
  nz, ny, nx = tsdf.shape
  volume = TSDFVolume(origin, voxel_size, (nx, ny, nz), colour=colour is not None, device=DEVICE)
  volume.tsdf.copy_(torch.as_tensor(tsdf))
  volume.weight.copy_(torch.as_tensor(weight))
  if colour is not None:
    volume.colour.copy_(torch.as_tensor(colour))
  return volume, volume.extract_mesh(min_weight)


def assert_matches_oracle(tsdf, weight, origin, voxel_size, min_weight=0.0, colour=None):
  volume, mesh = extract(tsdf, weight, origin, voxel_size, min_weight, colour)
  vertices, faces, colours = to.marching_tetrahedra(tsdf, weight, origin, voxel_size, min_weight, colour)
  assert mesh.vertices.dtype == torch.float32 and mesh.faces.dtype == torch.int32
  assert tuple(mesh.vertices.shape) == vertices.shape and tuple(mesh.faces.shape) == faces.shape
  got = mesh.vertices.cpu().double().numpy()
  bound = 8 * EPS * (np.abs(vertices) + to.f32(voxel_size))
  assert (np.abs(got - vertices) <= bound).all(), float((np.abs(got - vertices) / bound).max())
  assert np.array_equal(to.canonical_faces(mesh.faces.cpu().numpy()), to.canonical_faces(faces))
  if colour is not None:
    assert (np.abs(mesh.colours.cpu().double().numpy() - colours) <= 8 * EPS * max(1.0, float(np.abs(colour).max()))).all()
  else:
    assert mesh.colours is None
  again = volume.extract_mesh(min_weight)
  assert torch.equal(bits(again.vertices), bits(mesh.vertices)) and torch.equal(again.faces, mesh.faces)
  return mesh


def test_all_256_sign_patterns_in_one_launch():
  tsdf, weight = to.all_sign_patterns()
  mesh = assert_matches_oracle(tsdf, weight, (0.5, 0.25, 0.0), 0.125)
  assert mesh.faces.shape[0] > 254


@pytest.mark.parametrize('dims', [(1, 1, 1), (2, 1, 1), (2, 2, 2), (3, 2, 2), (7, 5, 3), (67, 5, 4), (9, 33, 2)])
def test_triangulation_against_the_oracle(dims):
  """random fields with a fifth of the samples unobserved and a weight threshold that rejects some more; (2, 1, 1) and
  (1, 1, 1) have no cell: an empty face list (and for one sample an empty mesh) without a division by zero; (67, 5, 4) and
  (9, 33, 2) span several workgroups with rows that are no multiple of anything"""
  nx, ny, nz = dims
  generator = torch.Generator().manual_seed(nx * 100 + ny * 10 + nz)
  tsdf = (torch.rand((nz, ny, nx), generator=generator) * 2 - 1).numpy()
  tsdf.reshape(-1)[::5] = 0.0                                         # exact zeros count as outside; lambda = 0 or 1
  weight = (torch.rand((nz, ny, nx), generator=generator) * 3).numpy()
  weight[torch.rand((nz, ny, nx), generator=generator).numpy() < 0.2] = 0.0
  colour = torch.rand((nz, ny, nx, 3), generator=generator).numpy()
  mesh = assert_matches_oracle(tsdf, weight, (0.3, 1.7, 0.0), 0.21, min_weight=0.4, colour=colour)
  if nx == 1 or ny == 1 or nz == 1:
    assert mesh.faces.shape[0] == 0
  if dims == (2, 1, 1):
    _, empty = extract(np.ones((1, 1, 2), dtype=np.float32), np.ones((1, 1, 2), dtype=np.float32), (0, 0, 0), 1.0)
    assert empty.vertices.shape == (0, 3) and empty.faces.shape == (0, 3)
  assert_matches_oracle(tsdf, weight, (0.3, 1.7, 0.0), 0.21)          # min_weight 0: weight > 0 alone


# ---- geometry ----------------------------------------------------------------------------------------------------------

H = 0.25
ORIGIN = (0.5, 1.0, 0.25)
GRID = (21, 21, 21)
CENTRE = np.array([0.5 + 2.5 + 0.03, 1.0 + 2.5 - 0.02, 0.25 + 2.5 + 0.01])


def analytic_mesh(field, weight=None, dims=GRID):
  positions = to.grid_positions(ORIGIN, H, dims)
  values = field(positions).astype(np.float32)
  weight = np.ones_like(values) if weight is None else weight(positions).astype(np.float32)
  _, mesh = extract(values, weight, ORIGIN, H)
  return mesh.vertices.cpu().double().numpy(), mesh.faces.cpu().numpy().astype(np.int64), positions, weight


def test_plane_vertices_lie_on_the_plane():
  normal = np.array([0.36, -0.48, 0.8])
  offset = float(normal @ CENTRE) + 0.037
  vertices, faces, _, _ = analytic_mesh(lambda p: p @ normal - offset)
  assert faces.shape[0] > 100
  # linear interpolation of a linear field is exact: what is left is the position error (8 eps (|p| + h) per component,
  # sqrt(3) of it along the normal) and the float32 rounding of the stored field (eps |t|, |t| <= sqrt(3) h at an edge end)
  bound = (8 * math.sqrt(3) + 2) * EPS * (np.abs(vertices).max() + H)
  assert np.abs(vertices @ normal - offset).max() <= bound
  assert (to.undirected_edges(faces)[1] <= 2).all() and (to.directed_edge_multiplicities(faces) == 1).all()


def test_sphere_is_closed_oriented_and_accurate():
  radius = 6.3 * H
  vertices, faces, _, _ = analytic_mesh(lambda p: to.sphere_field(p, CENTRE, radius))
  assert to.euler_characteristic(faces) == 2
  assert (to.undirected_edges(faces)[1] == 2).all() and (to.directed_edge_multiplicities(faces) == 1).all()
  bound = 3 * H * H / (8 * (radius - math.sqrt(3) * H))
  error = np.abs(np.linalg.norm(vertices - CENTRE, axis=1) - radius)
  print(f"sphere: largest radial error {error.max() / H:.4f} h, bound {bound / H:.4f} h")
  assert error.max() <= bound
  volume = to.signed_volume(vertices, faces)
  assert 4 / 3 * math.pi * (radius - bound) ** 3 <= volume <= 4 / 3 * math.pi * (radius + bound) ** 3


def test_torus_has_euler_characteristic_zero():
  vertices, faces, _, _ = analytic_mesh(lambda p: to.torus_field(p, CENTRE, 1.5, 0.6))
  assert to.euler_characteristic(faces) == 0
  assert (to.undirected_edges(faces)[1] == 2).all() and (to.directed_edge_multiplicities(faces) == 1).all()
  assert to.signed_volume(vertices, faces) > 0


def test_half_valid_field_gives_an_open_surface_bounded_by_invalid_cells():
  radius = 6.3 * H
  vertices, faces, positions, weight = analytic_mesh(lambda p: to.sphere_field(p, CENTRE, radius),
                                                     weight=lambda p: (p[..., 0] < CENTRE[0] + 0.3 * H).astype(np.float64))
  edges, counts = to.undirected_edges(faces)
  assert counts.max() == 2 and (counts == 1).any()                    # open, and no edge in more than two triangles
  assert (to.directed_edge_multiplicities(faces) == 1).all()
  valid = weight > 0
  nz, ny, nx = valid.shape
  cell_valid = np.ones((nz - 1, ny - 1, nx - 1), dtype=bool)
  for dz in (0, 1):
    for dy in (0, 1):
      for dx in (0, 1):
        cell_valid &= valid[dz:nz - 1 + dz, dy:ny - 1 + dy, dx:nx - 1 + dx]
  for a, b in edges[counts == 1]:
    middle = (0.5 * (vertices[a] + vertices[b]) - np.array(ORIGIN)) / H
    touching = [tuple(np.clip(np.floor(middle + 1e-6 * np.array(s)).astype(int), 0, [nx - 2, ny - 2, nz - 2]))
                for s in [(sx, sy, sz) for sx in (-1, 1) for sy in (-1, 1) for sz in (-1, 1)]]
    assert any(not cell_valid[k, j, i] for i, j, k in touching), (a, b, middle)


# ---- the scene-level call ----------------------------------------------------------------------------------------------

def test_fuse_scene_equals_the_hand_loop():
  from taichi_splatting_amd import CameraParams, Gaussians3D, RasterConfig, render_gaussians, render_geometry
  generator = torch.Generator().manual_seed(5)
  n = 600
  normal = torch.nn.functional.normalize(torch.randn((n, 3), generator=generator), dim=1)
  position = 0.8 * normal
  axis = torch.linalg.cross(torch.tensor([0.0, 0.0, 1.0]).expand(n, 3), normal)
  rotation = torch.nn.functional.normalize(torch.cat([axis, 1.0 + normal[:, 2:3]], dim=1), dim=1)       # z axis -> normal (xyzw)
  log_scaling = torch.tensor([0.12, 0.12, 0.004]).log().expand(n, 3).contiguous()
  scene = Gaussians3D(position=position, log_scaling=log_scaling, rotation=rotation, alpha_logit=torch.full((n, 1), 6.0),
                      feature=torch.rand((n, 3), generator=generator), batch_size=(n,)).to(DEVICE)
  cameras = []
  for eye in ((3, 0, 0), (-3, 0, 0), (0, 3, 0.1), (0, -3, 0.1), (0.1, 0, 3), (0.1, 0, -3)):
    T = torch.from_numpy(to.look_at(eye, (0, 0, 0))).to(torch.float32).to(DEVICE)
    cameras.append(CameraParams(projection=torch.tensor([70.0, 70.0, 32.0, 32.0], device=DEVICE), T_camera_world=T,
                                near_plane=0.1, far_plane=20.0, image_size=(64, 64)))
  config = RasterConfig()
  make = lambda: TSDFVolume((-1.2, -1.2, -1.2), 2.4 / 31, (32, 32, 32), device=DEVICE)
  fused = fuse_scene(scene, cameras, config, make(), batch=4)
  by_hand = make()
  with torch.no_grad():
    for camera in cameras:
      rendering = render_gaussians(scene, camera, config, use_sh=False)
      depth = render_geometry(rendering, scene, normals=False).depth
      by_hand.integrate(depth, camera, colour=rendering.image)
  for name in ('tsdf', 'weight', 'colour'):
    assert torch.equal(bits(getattr(fused, name)), bits(getattr(by_hand, name))), name
  mesh = fused.extract_mesh(min_weight=1.0)
  assert mesh.vertices.shape[0] > 100 and mesh.faces.shape[0] > 100 and mesh.colours.shape == mesh.vertices.shape
  radial = (mesh.vertices.norm(dim=1) - 0.8).abs()
  print(f"fuse_scene: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} faces, median radial error "
        f"{float(radial.median()) / (2.4 / 31):.3f} voxels")
