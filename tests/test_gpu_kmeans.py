"""ms_kmeans_assign / ms_kmeans_update, misc.kmeans.kmeans and scene_codec.compress_scene on the GPU against the float64
oracle (tests/kmeans_oracle.py, where the bound b is derived).

Exact cases use integer-valued float32 in [-8, 8]: every product, sum and norm is exact in float32, so index (lowest on
ties) and dist2 must equal the oracle's bit for bit.  The data are random, hence asymmetric: a row/column swap in the
accumulator map cannot pass.  Duplicated codes are planted at K - 1, across the 32-code tile boundary, in the same lane
of two tiles and in neighbouring lanes of one, each with a point sitting exactly on it.  Float cases hold every point
to b.  The update is held to one float32 ulp of the float64 mean (its float64 sums leave only the final rounding)."""
import numpy as np
import pytest
import torch

from taichi_splatting_amd import Gaussians3D, RasterConfig, render_gaussians, compress_scene, load_compressed
from taichi_splatting_amd.misc import kmeans as km
from taichi_splatting_amd.testing import random_camera, random_3d_gaussians
from tests import kmeans_oracle as ko

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
U = ko.U


def dev(a, dtype=None):
  return torch.as_tensor(np.ascontiguousarray(a), dtype=dtype).to(DEV)


def integer_case(n, k, d, seed):
  """(x, codebook) of integers in [-8, 8] with planted duplicate codes and points on them (where the indices exist)"""
  rng = np.random.default_rng(seed)
  x = rng.integers(-8, 9, size=(n, d)).astype(np.float32)
  c = rng.integers(-8, 9, size=(k, d)).astype(np.float32)
  # (later copy, earlier original): K - 1 <- 3, 33 <- 30 (tile boundary), 40 <- 8 (same lane, next tile), 5 <- 4 (same tile)
  for row, (late, early) in enumerate(((k - 1, 3), (33, 30), (40, 8), (5, 4))):
    if early < late < k:
      c[late] = c[early]
      if row < n:
        x[row] = c[early]
  return x, c


def check_exact(x, c):
  index, dist2 = km.kmeans_assign(dev(x), dev(c))
  torch.cuda.synchronize()
  want_index, want_dist2 = ko.assign(x, c)
  assert index.dtype == torch.int32 and dist2.dtype == torch.float32
  got = index.cpu().numpy()
  assert np.array_equal(got, want_index), (np.flatnonzero(got != want_index)[:8], got[got != want_index][:8],
                                            want_index[got != want_index][:8])
  assert np.array_equal(dist2.cpu().numpy().astype(np.float64), want_dist2)


@pytest.mark.parametrize('d', [1, 2, 9, 24, 45, 63, 64])
def test_assign_exact_on_integers(d):
  check_exact(*integer_case(1000, 70, d, seed=d))


@pytest.mark.parametrize('k', [1, 31, 32, 33])
def test_assign_exact_at_tile_edges(k):
  for n in (1, 31, 32, 33, 127, 128, 129):
    check_exact(*integer_case(n, k, 9, seed=100 * k + n))


def test_assign_exact_over_several_staging_passes():
  x, c = integer_case(300, 4100, 45, seed=7)
  c[4099] = c[130]                          # a duplicate 31 chunks apart, with a point on it
  x[5] = c[130]
  check_exact(x, c)


def test_assign_exact_at_the_largest_codebook():
  x, c = integer_case(64, 65536, 9, seed=8)
  c[65535] = c[65000]
  x[6] = c[65000]
  x[7] = c[65535 - 64]
  check_exact(x, c)


def test_assign_of_no_points_is_empty():
  index, dist2 = km.kmeans_assign(torch.empty((0, 9), device=DEV), torch.randn(5, 9, device=DEV))
  assert index.shape == (0,) and index.dtype == torch.int32 and dist2.shape == (0,)
  new, counts = km.kmeans_update(torch.empty((0, 9), device=DEV), torch.empty((0,), dtype=torch.int32, device=DEV),
                                 torch.ones(5, 9, device=DEV))
  assert bool((new == 1).all()) and counts.tolist() == [0] * 5


@pytest.mark.parametrize('scale', [1e-3, 1.0, 1e3])
@pytest.mark.parametrize('d', [9, 45, 64])
def test_assign_floats_within_the_bound(scale, d):
  """Every point: the chosen code is within b of the best one, and dist2 within b + (D + 1) u ||x||^2 of the truth."""
  rng = np.random.default_rng(d)
  n, k = 1000, 70
  x = (scale * rng.standard_normal((n, d))).astype(np.float32)
  c = (scale * rng.standard_normal((k, d))).astype(np.float32)
  c[:35] = x[:35] + np.float32(1e-4 * scale) * rng.standard_normal((35, d)).astype(np.float32)   # near misses
  c[36] = c[35]
  index, dist2 = km.kmeans_assign(dev(x), dev(c))
  torch.cuda.synchronize()
  index, dist2 = index.cpu().numpy(), dist2.cpu().numpy().astype(np.float64)
  assert index.min() >= 0 and index.max() < k
  best, best_d = ko.assign(x, c)
  true_d = ko.dist2_to(x, c, index)
  b_got, b_best = ko.score_bound(x, c, index), ko.score_bound(x, c, best)
  slack = best_d + b_got + b_best - true_d
  print(f"scale {scale} D {d}: {int((index != best).sum())} of {n} differ from the oracle; worst excess over the best "
        f"{float(((true_d - best_d) / (b_got + b_best)).max()):.3f} of the allowance")
  assert (slack >= 0).all(), (int((slack < 0).sum()), float(slack.min()))
  x_norm = (x.astype(np.float64) ** 2).sum(axis=1)
  dist_err, dist_tol = np.abs(dist2 - true_d), b_got + (d + 1) * U * x_norm
  print(f"  dist2: worst {float((dist_err / dist_tol).max()):.3f} of the allowance")
  assert (dist_err <= dist_tol).all(), (int((dist_err > dist_tol).sum()), float((dist_err / dist_tol).max()))
  assert (dist2 >= 0).all()


# ---- update --------------------------------------------------------------------------------------------------------

def check_update(x, index, old, weights=None):
  args = (dev(x), dev(index, torch.int32), dev(old))
  w = None if weights is None else dev(weights)
  new, counts = km.kmeans_update(*args, weights=w)
  again, _ = km.kmeans_update(*args, weights=w)
  torch.cuda.synchronize()
  assert torch.equal(new, again), "two runs differ"
  assert torch.equal(args[2], dev(old)), "the input codebook was modified"
  want, want_counts, wsum = ko.update(x, index, old, weights)
  new = new.cpu().numpy()
  assert np.array_equal(counts.cpu().numpy(), want_counts)
  kept = (want_counts == 0) | (wsum == 0)
  assert np.array_equal(new[kept].view(np.uint32), old[kept].view(np.uint32)), "an empty or weightless code moved"
  ulp = np.spacing(np.abs(want))
  assert (np.abs(new.astype(np.float64) - want.astype(np.float64)) <= ulp).all(), \
    float((np.abs(new.astype(np.float64) - want) / ulp).max())
  return new


@pytest.mark.parametrize('weighted', [False, True])
def test_update_matches_the_float64_mean(weighted):
  rng = np.random.default_rng(3)
  n, k, d = 1000, 70, 45
  x = rng.standard_normal((n, d)).astype(np.float32)
  old = rng.standard_normal((k, d)).astype(np.float32)
  index = rng.integers(0, k, size=n)
  index[(index == 7) | (index == 69) | (index == 0)] = 1         # codes 0, 7 and the last stay empty
  weights = None
  if weighted:
    weights = rng.random(n).astype(np.float32)
    weights[index == 9] = 0.0                                    # a code whose members weigh nothing
    weights[::17] = 0.0
  check_update(x, index, old, weights)


def test_update_of_one_cluster_holding_every_point():
  rng = np.random.default_rng(4)
  x = (5.0 + rng.standard_normal((5000, 24))).astype(np.float32)
  old = rng.standard_normal((4, 24)).astype(np.float32)
  check_update(x, np.full(5000, 2), old)
  check_update(x, np.full(5000, 2), old, rng.random(5000).astype(np.float32))


def test_update_combines_many_chunks():
  rng = np.random.default_rng(5)
  n = 100_000
  x = (1.0 + rng.standard_normal((n, 9))).astype(np.float32)
  old = np.zeros((3, 9), dtype=np.float32)
  index = rng.integers(0, 3, size=n)
  check_update(x, index, old)
  check_update(x, index, old, rng.random(n).astype(np.float32))


def test_update_returns_weight_sums_when_asked():
  rng = np.random.default_rng(6)
  x, index = rng.standard_normal((500, 9)).astype(np.float32), rng.integers(0, 5, size=500)
  w = rng.random(500).astype(np.float32)
  codebook, counts = dev(np.zeros((5, 9), dtype=np.float32)), torch.empty(5, dtype=torch.int32, device=DEV)
  sums = torch.empty(5, dtype=torch.float64, device=DEV)
  scratch = torch.empty(km.update_scratch_bytes(500, 9, 5), dtype=torch.uint8, device=DEV)
  km.kmeans_update_into(dev(x), dev(index, torch.int32), codebook, counts, scratch, dev(w), sums)
  want = np.bincount(index, weights=w.astype(np.float64), minlength=5)
  assert np.allclose(sums.cpu().numpy(), want, rtol=1e-14, atol=0)


# ---- Lloyd ---------------------------------------------------------------------------------------------------------

def clustered(n, d, centres, seed):
  rng = np.random.default_rng(seed)
  mu = 3.0 * rng.standard_normal((centres, d))
  return (mu[rng.integers(0, centres, size=n)] + rng.standard_normal((n, d))).astype(np.float32)


def test_lloyd_objective_never_rises_beyond_the_assignment_tolerance():
  """kmeans is bitwise reproducible under a seed, so iterations = 0..5 are the states of one run after each assign."""
  x = clustered(3000, 24, 12, seed=11)
  xd = dev(x)
  previous = None
  for iterations in range(6):
    r = km.kmeans(xd, 20, iterations=iterations, seed=5)
    codebook, index = r.codebook.cpu().numpy(), r.index.cpu().numpy()
    best, _ = ko.assign(x, codebook)
    tolerance = float((ko.score_bound(x, codebook, index) + ko.score_bound(x, codebook, best)).sum())
    value = ko.objective(x, codebook, index)
    print(f"iterations {iterations}: objective {value:.6f}, tolerance {tolerance:.3e}")
    if previous is not None:
      assert value <= previous + tolerance, (iterations, value, previous, tolerance)
    previous = value
    # index is the assignment of the returned codebook, dist2 and counts belong to it
    again, dist2 = km.kmeans_assign(xd, r.codebook)
    assert torch.equal(again, r.index) and torch.equal(dist2, r.dist2)
    assert np.array_equal(r.counts.cpu().numpy(), np.bincount(index, minlength=20))
  first = km.kmeans(xd, 20, iterations=0, seed=5)
  assert ko.objective(x, r.codebook.cpu().numpy(), r.index.cpu().numpy()) < \
    ko.objective(x, first.codebook.cpu().numpy(), first.index.cpu().numpy())


def test_lloyd_is_reproducible_under_a_seed_and_starts_from_rows_of_x():
  x = dev(clustered(2000, 9, 8, seed=12))
  w = torch.rand(2000, device=DEV)
  a, b = km.kmeans(x, 16, iterations=5, weights=w, seed=3), km.kmeans(x, 16, iterations=5, weights=w, seed=3)
  for got, want in zip(a, b):
    assert torch.equal(got, want)
  assert not torch.equal(a.codebook, km.kmeans(x, 16, iterations=5, weights=w, seed=4).codebook)
  start = km.kmeans(x, 16, iterations=0, seed=3)
  g = torch.Generator(device=DEV)
  g.manual_seed(3)
  rows = torch.randperm(2000, generator=g, device=DEV)[:16]
  assert torch.equal(start.codebook, x[rows]) and rows.unique().numel() == 16
  torch.manual_seed(9)
  c = km.kmeans(x, 16, iterations=2)
  torch.manual_seed(9)
  assert torch.equal(c.codebook, km.kmeans(x, 16, iterations=2).codebook)


def test_one_lloyd_iteration_on_integers_is_the_oracle_s():
  """Integer data: the first assignment is exact, so after one iteration the codebook is the oracle's to the one ulp of
  the update's final rounding."""
  xi, _ = integer_case(2000, 16, 9, seed=14)
  x = dev(xi)
  start = km.kmeans(x, 16, iterations=0, seed=3).codebook.cpu().numpy()
  want, _, _ = ko.lloyd(xi, start, 1)
  got = km.kmeans(x, 16, iterations=1, seed=3).codebook.cpu().numpy()
  assert (np.abs(got.astype(np.float64) - want.astype(np.float64)) <= np.spacing(np.abs(want))).all()


def test_assign_and_update_capture_into_one_graph():
  x = dev(clustered(1500, 45, 6, seed=13))
  n, d, k = 1500, 45, 33
  start = x[:k].clone()
  index = torch.empty(n, dtype=torch.int32, device=DEV)
  dist2 = torch.empty(n, dtype=torch.float32, device=DEV)
  counts = torch.empty(k, dtype=torch.int32, device=DEV)
  codebook = start.clone()
  sa = torch.empty(km.assign_scratch_bytes(n, d, k), dtype=torch.uint8, device=DEV)
  su = torch.empty(km.update_scratch_bytes(n, d, k), dtype=torch.uint8, device=DEV)

  def step():
    km.kmeans_assign_into(x, codebook, index, dist2, sa)
    km.kmeans_update_into(x, index, codebook, counts, su)

  step()
  torch.cuda.synchronize()
  eager = [t.clone() for t in (codebook, index, dist2, counts)]

  graph = torch.cuda.CUDAGraph()
  codebook.copy_(start)
  torch.cuda.synchronize()
  with torch.cuda.graph(graph):
    step()
  for _ in range(2):
    codebook.copy_(start)
    index.fill_(-1)
    graph.replay()
    torch.cuda.synchronize()
    for got, want in zip((codebook, index, dist2, counts), eager):
      assert torch.equal(got, want)


# ---- scenes --------------------------------------------------------------------------------------------------------

def random_scene(n, degree, seed):
  torch.manual_seed(seed)
  cam = random_camera(image_size=(160, 96))
  g = random_3d_gaussians(n, cam, scale_factor=1.0, alpha_range=(0.1, 0.9))
  return g.replace(feature=(torch.rand(n, 3, (degree + 1) ** 2) - 0.5) * 0.5).to(DEV), cam.to(device=DEV)


@pytest.mark.parametrize('degree,codes', [(3, 64), (1, 16)])
def test_compress_scene(degree, codes, tmp_path):
  n = 2000
  g, cam = random_scene(n, degree, seed=degree)
  c = compress_scene(g, sh_codes=codes, iterations=5, seed=1)
  m = (degree + 1) ** 2 - 1
  assert c.sh_degree == degree and c.sh_codebook.shape == (codes, 3, m) and c.sh_index.dtype == torch.int32
  assert int(c.sh_index.min()) >= 0 and int(c.sh_index.max()) < codes
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit'):
    assert torch.equal(getattr(c, name), getattr(g, name)), name
  assert torch.equal(c.dc, g.feature[:, :, 0])
  decoded = c.decode()
  assert decoded.feature.shape == g.feature.shape and decoded.feature.is_cuda
  assert torch.equal(decoded.feature[:, :, 0], g.feature[:, :, 0])
  assert torch.equal(decoded.feature[:, :, 1:], c.sh_codebook[c.sh_index.long()])
  assert c.nbytes == n * 58 + codes * 3 * m * 4 and c.nbytes < sum(t.numel() * 4 for t in g.shape_tensors() + (g.feature,))
  assert torch.equal(g.compressed(sh_codes=codes, iterations=5, seed=1).sh_index, c.sh_index)

  rows = g.feature[:, :, 1:].reshape(n, 3 * m).cpu().numpy()
  first = compress_scene(g, sh_codes=codes, iterations=0, seed=1)
  objective = lambda s: ko.objective(rows, s.sh_codebook.reshape(codes, 3 * m).cpu().numpy(), s.sh_index.cpu().numpy())
  assert objective(c) <= objective(first)

  r = render_gaussians(decoded, cam, RasterConfig(), use_sh=True)
  torch.cuda.synchronize()
  assert r.image.shape[:2] == (96, 160) and bool(torch.isfinite(r.image).all())

  c.save(tmp_path / 'scene.npz')
  back = load_compressed(tmp_path / 'scene.npz', device=DEV).decode()
  for name in ('position', 'log_scaling', 'rotation', 'alpha_logit', 'feature'):
    assert getattr(back, name).is_cuda and torch.equal(getattr(back, name), getattr(decoded, name)), name


def test_render_scene_tool_renders_the_quantised_scene(tmp_path):
  """``tools/render_scene.py scene.ply --sh-codes K``, a fresh child process: the two sizes and the PSNR of the renders"""
  import json
  import subprocess
  import sys
  from pathlib import Path
  from taichi_splatting_amd import save_ply
  n = 300
  g, _ = random_scene(n, 2, seed=6)
  save_ply(g.to('cpu'), tmp_path / 'scene.ply')
  tool = str(Path(__file__).resolve().parent.parent / 'tools' / 'render_scene.py')
  done = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--sh-codes', '8', '--views', '2', '--size', '64', '48',
                         '--out', str(tmp_path / 'out')], capture_output=True, text=True, timeout=120)
  assert done.returncode == 0, done.stderr[-2000:]
  q = json.loads(done.stdout.strip().splitlines()[-1])['quantised']
  assert q['sh_codes'] == 8 and q['original_bytes'] == n * (11 + 27) * 4 and q['quantised_bytes'] == n * 58 + 8 * 24 * 4
  assert len(q['psnr_db_per_view']) == 2 and q['psnr_db'] is not None and q['psnr_db'] > 0.0 and q['compress_s'] > 0
  assert (tmp_path / 'out' / 'quantised_001.npy').exists() and 'quantised: 8 codes' in done.stderr
  refused = subprocess.run([sys.executable, tool, str(tmp_path / 'scene.ply'), '--sh-codes', '301', '--views', '1', '--size', '64', '48'],
                           capture_output=True, text=True, timeout=120)
  assert refused.returncode != 0 and '--sh-codes' in refused.stderr


def test_compress_scene_with_weights_moves_the_codes_towards_heavy_rows():
  g, _ = random_scene(500, 2, seed=4)
  w = torch.zeros(500, device=DEV)
  w[:100] = 1.0
  c = compress_scene(g, sh_codes=1, iterations=1, weights=w, seed=0)
  want = g.feature[:100, :, 1:].double().mean(dim=0)
  assert torch.allclose(c.sh_codebook[0].double(), want, rtol=0, atol=1e-6)
