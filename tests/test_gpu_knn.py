"""ms_knn_points / misc.knn / Gaussians3D.from_point_cloud on the GPU against the float64 brute-force oracle
(tests/knn_oracle.py: the oracle, the point sets and the criterion, all argued there).

Sizes sit around the structure of the search: one lane per query in waves of 64, blocks of BLOCK sorted points (BLOCK
imported, not written here).  The seven point sets at N = 20 000 (79 blocks) each aim at one way to lose a neighbour.
The pruning conditions read the kernel's own counters, not a clock: a CPU model of the design (blocks of 256, seed from
the own block, wave-uniform scan) evaluates 0.19 - 0.24 of brute force at 20 000 uniform points and grows 1.33 x per
query from 20 000 to 80 000 where brute force grows 4 x; the conditions (<= 0.5, < 2 x) leave that room.
Measured figures: profiles/knn.txt.
"""
import math

import pytest
import torch

from taichi_splatting_amd import Gaussians3D, RasterConfig, render_gaussians
from taichi_splatting_amd.data_types import SH_C0
from taichi_splatting_amd.misc import knn, mean_knn_dist2
from taichi_splatting_amd.misc.knn import BLOCK, knn_into, morton_order, scratch_bytes
from taichi_splatting_amd.testing import random_camera
from tests import knn_oracle as ko

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N_SET = 20_000
SIZES = (1, 2, 3, 4, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7)
KS = (1, 3, 8)

_cache = {}


def point_set(name, n=N_SET):
  """(points on the GPU, oracle dist2 for k = 8 on the GPU): made once per module, never written to"""
  key = (name, n)
  if key not in _cache:
    p = ko.make(name, n, BLOCK).to(DEV)
    _cache[key] = (p, ko.brute_force(p, 8)[0])
  return _cache[key]


def stats_of(points, k=3):
  """[blocks scanned x queries, distance evaluations] of one search in Morton order"""
  n = points.shape[0]
  stats = torch.zeros((2,), dtype=torch.int64, device=points.device)
  dist2 = torch.empty((n, k), dtype=torch.float32, device=points.device)
  knn_into(points, morton_order(points), k, dist2, None, torch.empty((scratch_bytes(n),), dtype=torch.uint8, device=points.device), stats)
  return [int(v) for v in stats.tolist()], dist2


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('n', SIZES)
def test_sizes_around_the_wave_and_the_block(n, k):
  p = ko.make('uniform_cube', n, BLOCK, seed=n).to(DEV)
  dist2, index = knn(p, k)
  worst = ko.check(p, k, dist2, index, ko.brute_force(p, 8)[0], f"N = {n}, k = {k}")
  print(f"N = {n} k = {k}: largest relative error {worst:.2f} x 2^-24")
  again, none = knn(p, k, return_indices=False)
  assert none is None and torch.equal(again.view(torch.int32), dist2.view(torch.int32))


def test_no_points():
  dist2, index = knn(torch.empty((0, 3), device=DEV), 3)
  assert dist2.shape == (0, 3) and dist2.dtype == torch.float32 and index.shape == (0, 3) and index.dtype == torch.int32


@pytest.mark.parametrize('k', (3, 8))
@pytest.mark.parametrize('name', sorted(ko.DISTRIBUTIONS))
def test_point_sets(name, k):
  p, want = point_set(name)
  dist2, index = knn(p, k)
  worst = ko.check(p, k, dist2, index, want, f"{name}, k = {k}")
  print(f"{name} k = {k}: largest relative error {worst:.2f} x 2^-24")


@pytest.mark.parametrize('name', ('uniform_cube', 'duplicates', 'lattice', 'clusters_and_loner'))
def test_distances_do_not_depend_on_the_order(name):
  p, want = point_set(name)
  n = p.shape[0]
  orders = {
    'morton': morton_order(p),
    'identity': torch.arange(n, dtype=torch.int32, device=DEV),
    'random': torch.randperm(n, generator=torch.Generator().manual_seed(5)).to(DEV),      # int64: converted by knn
  }
  results = {key: knn(p, 3, order=order) for key, order in orders.items()}
  results['morton again'] = knn(p, 3, order=orders['morton'])
  results['own order'] = knn(p, 3)
  first = results['morton'][0].view(torch.int32)
  for key, (dist2, index) in results.items():
    assert torch.equal(dist2.view(torch.int32), first), f"{name}: dist2 under order '{key}' differs bitwise"
    ko.check(p, 3, dist2, index, want, f"{name}, order {key}")
  assert torch.equal(results['morton again'][1], results['morton'][1])          # the same run twice: indices too


def test_nonfinite_points_and_bad_orders_are_refused():
  p = point_set('uniform_cube')[0].clone()
  p[17, 1] = math.nan
  with pytest.raises(ValueError, match="finite"):
    knn(p, 3)
  p[17, 1] = math.inf
  with pytest.raises(ValueError, match="finite"):
    mean_knn_dist2(p, 3)
  p[17, 1] = 0.5
  with pytest.raises(ValueError, match="order"):
    knn(p, 3, order=torch.arange(5, dtype=torch.int32, device=DEV))
  with pytest.raises(ValueError, match="order"):
    knn(p, 3, order=torch.arange(p.shape[0], dtype=torch.float32, device=DEV))


def test_pruning_by_the_counters():
  """conditions on the kernel's own counters (module docstring): no clock"""
  p20, want = point_set('uniform_cube')
  (scanned20, evals20), dist2 = stats_of(p20)
  ko.check(p20, 3, dist2, None, want, "uniform cube with counters")
  n20 = p20.shape[0]
  brute20 = n20 * (n20 - 1)
  print(f"uniform cube N = {n20}: {evals20} evaluations = {evals20 / brute20:.3f} of brute force, "
        f"{evals20 / n20:.0f} per query, {scanned20 / n20:.1f} blocks per query")
  assert evals20 >= 3 * n20 and scanned20 >= n20                 # the counters count: at least the own block
  assert evals20 <= 0.5 * brute20
  p80 = ko.make('uniform_cube', 4 * n20, BLOCK, seed=1).to(DEV)
  (scanned80, evals80), _ = stats_of(p80)
  n80 = p80.shape[0]
  print(f"uniform cube N = {n80}: {evals80} evaluations = {evals80 / (n80 * (n80 - 1)):.3f} of brute force, "
        f"{evals80 / n80:.0f} per query, {scanned80 / n80:.1f} blocks per query; per-query growth {evals80 / n80 / (evals20 / n20):.2f} x")
  assert evals80 / n80 < 2.0 * evals20 / n20
  # an order without locality prunes nothing, and is still exact: the counters then read brute force
  stats = torch.zeros((2,), dtype=torch.int64, device=DEV)
  small = p20[:5000].contiguous()
  out = torch.empty((5000, 3), dtype=torch.float32, device=DEV)
  knn_into(small, torch.arange(5000, dtype=torch.int32, device=DEV), 3, out, None,
           torch.empty((scratch_bytes(5000),), dtype=torch.uint8, device=DEV), stats)
  assert int(stats[1]) <= 5000 * 4999
  print(f"uniform cube N = 5000 in input (random) order: {int(stats[1]) / (5000 * 4999):.3f} of brute force")


def test_on_another_stream():
  p, want = point_set('uniform_cube')
  expect = knn(p, 3)
  stream = torch.cuda.Stream(device=DEV)
  stream.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(stream):
    dist2, index = knn(p, 3)
  stream.synchronize()
  assert torch.equal(dist2.view(torch.int32), expect[0].view(torch.int32)) and torch.equal(index, expect[1])


def test_the_c_call_replays_from_a_graph():
  first, second = point_set('uniform_cube')[0], point_set('duplicates')[0]
  n, k = first.shape[0], 3
  static = first.clone()
  order = morton_order(first)                 # kept for the second set too: any permutation gives the same distances
  dist2 = torch.zeros((n, k), dtype=torch.float32, device=DEV)
  index = torch.zeros((n, k), dtype=torch.int32, device=DEV)
  scratch = torch.empty((scratch_bytes(n),), dtype=torch.uint8, device=DEV)
  side = torch.cuda.Stream(device=DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    knn_into(static, order, k, dist2, index, scratch)           # warm-up outside the capture
  torch.cuda.current_stream(DEV).wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    knn_into(static, order, k, dist2, index, scratch)
  for points in (first, second, first):
    static.copy_(points)
    dist2.zero_()
    index.zero_()
    graph.replay()
    torch.cuda.synchronize()
    expect = knn(points, k)
    assert torch.equal(dist2.view(torch.int32), expect[0].view(torch.int32))
    ko.check(points, k, dist2, index, point_set('uniform_cube' if points is first else 'duplicates')[1], "graph replay")


def test_mean_knn_dist2():
  p, want = point_set('clusters_and_loner')
  got = mean_knn_dist2(p, 3)
  expect = want[:, :3].mean(dim=1)
  assert got.shape == (p.shape[0],) and got.dtype == torch.float32
  assert float(((got.double() - expect).abs() / expect).max()) <= 8 * 2.0 ** -24     # 4 of the entries + two additions and a division, one more to spare
  pair = torch.tensor([[0.0, 0.0, 0.0], [3.0, 4.0, 0.0]], device=DEV)
  assert mean_knn_dist2(pair, 3).tolist() == [25.0, 25.0]                           # the mean of the one finite entry


def test_from_point_cloud():
  n = 5000
  gen = torch.Generator().manual_seed(11)
  torch.manual_seed(3)
  cam = random_camera(image_size=(160, 96))
  # points in front of the camera: in its frame, x, y within the view at depths 2 .. 6, then to the world
  depth = 2.0 + 4.0 * torch.rand((n, 1), generator=gen)
  local = torch.cat([(torch.rand((n, 2), generator=gen) - 0.5) * depth * 0.8, depth, torch.ones((n, 1))], dim=1)
  world = (torch.linalg.inv(cam.T_camera_world.double()) @ local.double().T).T[:, :3].float().contiguous()
  colours = torch.rand((n, 3), generator=gen)
  points, colours = world.to(DEV), colours.to(DEV)

  want = ko.brute_force(points, 3)[0].mean(dim=1)
  log_scale = torch.log(torch.sqrt(torch.clamp_min(want, 1e-7)))
  for degree in (None, 3):
    g = Gaussians3D.from_point_cloud(points, colours, sh_degree=degree)
    assert g.batch_size == (n,) and torch.equal(g.position, points)
    assert g.log_scaling.shape == (n, 3) and float((g.log_scaling.double() - log_scale[:, None]).abs().max()) <= 1e-6
    assert torch.equal(g.rotation, torch.tensor([0.0, 0.0, 0.0, 1.0], device=DEV).expand(n, 4))
    assert g.alpha_logit.shape == (n, 1) and float((torch.sigmoid(g.alpha_logit) - 0.1).abs().max()) <= 1e-6
    if degree is None:
      assert g.feature.shape == (n, 3) and torch.equal(g.feature, colours)
    else:
      assert g.feature.shape == (n, 3, 16) and float(g.feature[:, :, 1:].abs().max()) == 0.0
      assert float((g.feature[:, :, 0].double() - (colours.double() - 0.5) / SH_C0).abs().max()) <= 1e-6
  grey = Gaussians3D.from_point_cloud(points, k=2, initial_alpha=0.5, min_dist2=1e3)
  assert torch.equal(grey.feature, torch.full((n, 3), 0.5, device=DEV)) and float(grey.alpha_logit.abs().max()) <= 1e-6
  assert float((grey.log_scaling - 0.5 * math.log(1e3)).abs().max()) <= 1e-6       # the floor on the squared distance

  g = Gaussians3D.from_point_cloud(points, colours, sh_degree=3).requires_grad_(True)
  r = render_gaussians(g, cam.to(device=DEV), RasterConfig(), use_sh=True)
  assert r.image.shape == (96, 160, 3) and bool(torch.isfinite(r.image).all())
  assert float(r.image_weight.sum()) > 0
  r.image.sum().backward()
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature'):
    grad = getattr(g, name).grad
    assert grad is not None and bool(torch.isfinite(grad).all()), name
  assert float(g.feature.grad.abs().sum()) > 0 and float(g.position.grad.abs().sum()) > 0
