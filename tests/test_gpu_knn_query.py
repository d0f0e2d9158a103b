"""ms_knn_query / misc.knn_query on the GPU against the float64 brute force of tests/nearest_oracle.py (the oracle and
the criterion are argued there; the point sets are those of tests/knn_oracle.py).

Sizes sit around the structure of the search on BOTH sides: one lane per query in waves of 64, blocks of BLOCK sorted
points (imported, not written here), fewer points than k, and an empty set on either side.  The named sets at
20 000 x 20 000 (79 blocks) each aim at one way to lose a neighbour; `clusters_and_loner` points against `uniform_cube`
queries have disjoint boxes, so every neighbour lies in a block far from any seed.  Pruning is read from the kernel's own
counters, not from a clock: a numpy model of the design (256-point blocks, 64-query waves, seed from the hinted block)
evaluates 0.98 - 1.04 of what the self search evaluates on the same points, and under 0.25 of M N.
"""
import math

import pytest
import torch

from taichi_splatting_amd.misc import knn, knn_query
from taichi_splatting_amd.misc.knn import (BLOCK, MAX_K, knn_into, knn_query_into, morton_order, query_scratch_bytes, scratch_bytes,
                                           _common_bounds, _sorted_codes)
from tests import knn_oracle as ko
from tests import nearest_oracle as no

pytestmark = pytest.mark.gpu

DEV = 'cuda:0'
N_SET = 20_000
SIZES = (0, 1, 2, 63, 64, 65, BLOCK - 1, BLOCK, BLOCK + 1, 3 * BLOCK + 7)
GRID = sorted({(m, 65) for m in SIZES} | {(BLOCK + 1, n) for n in SIZES})        # (M, N)
KS = (1, 3, 8)

_cache = {}


def pair(points_name, queries_name=None, n=N_SET):
  """(points, queries, oracle dist2 for k = 8), all on the GPU: made once per module, never written to.  The queries are
  an independent draw (another seed) of `queries_name`, by default the points' own distribution."""
  queries_name = queries_name or points_name
  key = (points_name, queries_name, n)
  if key not in _cache:
    p = ko.make(points_name, n, BLOCK).to(DEV)
    q = ko.make(queries_name, n, BLOCK, seed=1000).to(DEV)
    _cache[key] = (p, q, no.cross(q, p, 8)[0])
  return _cache[key]


def bits(t):
  return t.view(torch.int32)


def plan(points, queries):
  """(point_order, query_order, hint) as knn_query makes them"""
  lower, upper = _common_bounds(queries, points)
  point_codes, point_order = _sorted_codes(points, lower, upper)
  query_codes, query_order = _sorted_codes(queries, lower, upper)
  return point_order, query_order, torch.searchsorted(point_codes, query_codes).to(torch.int32)


def run_into(points, point_order, queries, query_order, hint, k, stats=None):
  m, n = points.shape[0], queries.shape[0]
  dist2 = torch.empty((n, k), dtype=torch.float32, device=DEV)
  index = torch.empty((n, k), dtype=torch.int32, device=DEV)
  scratch = torch.empty((max(query_scratch_bytes(m, n), 1),), dtype=torch.uint8, device=DEV)
  knn_query_into(points, point_order, queries, query_order, hint, k, dist2, index, scratch, stats)
  return dist2, index


@pytest.mark.parametrize('k', KS)
@pytest.mark.parametrize('m,n', GRID)
def test_sizes_around_the_wave_and_the_block(m, n, k):
  p = ko.make('uniform_cube', m, BLOCK, seed=m).to(DEV)
  q = ko.make('uniform_cube', n, BLOCK, seed=5000 + n).to(DEV)
  dist2, index = knn_query(q, p, k)
  assert dist2.shape == (n, k) and dist2.dtype == torch.float32 and index.shape == (n, k) and index.dtype == torch.int32
  worst = no.check_cross(q, p, k, dist2, index, no.cross(q, p, 8)[0], f"M = {m}, N = {n}, k = {k}")
  print(f"M = {m} N = {n} k = {k}: largest relative error {worst:.2f} x 2^-24")
  again, none = knn_query(q, p, k, return_indices=False)
  assert none is None and torch.equal(bits(again), bits(dist2))


@pytest.mark.parametrize('k', (1, 8))
@pytest.mark.parametrize('name', sorted(ko.DISTRIBUTIONS))
def test_point_sets(name, k):
  p, q, want = pair(name)
  dist2, index = knn_query(q, p, k)
  worst = no.check_cross(q, p, k, dist2, index, want, f"{name}, k = {k}")
  print(f"{name} k = {k}: largest relative error {worst:.2f} x 2^-24")


@pytest.mark.parametrize('k', (1, 8))
def test_disjoint_boxes(k):
  """every neighbour lies in a far block: two tight clusters and a loner against a unit cube"""
  p, q, want = pair('clusters_and_loner', 'uniform_cube')
  dist2, index = knn_query(q, p, k)
  no.check_cross(q, p, k, dist2, index, want, f"clusters_and_loner x uniform_cube, k = {k}")
  back, back_index = knn_query(p, q, k)
  no.check_cross(p, q, k, back, back_index, no.cross(p, q, k)[0], f"uniform_cube x clusters_and_loner, k = {k}")


def test_duplicates_against_themselves():
  p = pair('duplicates')[0]
  dist2, index = knn_query(p, p, 8)
  no.check_cross(p, p, 8, dist2, index, no.cross(p, p, 8)[0], "duplicates x duplicates")
  assert float(dist2[:, 0].max()) == 0.0                                   # every point finds itself (or a copy)


@pytest.mark.parametrize('name', ('uniform_cube', 'duplicates', 'lattice', 'clusters_and_loner'))
def test_distances_do_not_depend_on_orders_or_hint(name):
  p, q, want = pair(name)
  m, n, k = p.shape[0], q.shape[0], 3
  point_order, query_order, hint = plan(p, q)
  gen = torch.Generator().manual_seed(5)
  identity = lambda count: torch.arange(count, dtype=torch.int32, device=DEV)
  shuffled = lambda count: torch.randperm(count, generator=gen).to(torch.int32).to(DEV)
  point_orders = {'morton': point_order, 'identity': identity(m), 'random': shuffled(m)}
  query_orders = {'morton': query_order, 'identity': identity(n), 'random': shuffled(n)}
  hints = {
    'searchsorted': hint, 'none': None, 'zero': torch.zeros((n,), dtype=torch.int32, device=DEV),
    'random': torch.randint(0, m, (n,), generator=gen).to(torch.int32).to(DEV),
    'negative': torch.full((n,), -7, dtype=torch.int32, device=DEV),
    'beyond': torch.full((n,), m + 12345, dtype=torch.int32, device=DEV),
    'extremes': torch.where(torch.arange(n, device=DEV) % 2 == 0, -2 ** 31, 2 ** 31 - 1).to(torch.int32),
  }
  first, first_index = run_into(p, point_order, q, query_order, hint, k)
  no.check_cross(q, p, k, first, first_index, want, f"{name}, as knn_query plans it")
  assert torch.equal(bits(knn_query(q, p, k)[0]), bits(first))
  for pk, po in point_orders.items():
    for qk, qo in query_orders.items():
      dist2, index = run_into(p, po, q, qo, hint if (pk, qk) == ('morton', 'morton') else None, k)
      assert torch.equal(bits(dist2), bits(first)), f"{name}: dist2 under point order '{pk}', query order '{qk}' differs bitwise"
      no.check_cross(q, p, k, dist2, index, want, f"{name}, orders {pk} / {qk}")
  for hk, h in hints.items():
    dist2, index = run_into(p, point_order, q, query_order, h, k)
    assert torch.equal(bits(dist2), bits(first)), f"{name}: dist2 under hint '{hk}' differs bitwise"
    no.check_cross(q, p, k, dist2, index, want, f"{name}, hint {hk}")
  again, again_index = run_into(p, point_order, q, query_order, hint, k)
  assert torch.equal(bits(again), bits(first)) and torch.equal(again_index, first_index)      # the same run twice: indices too


@pytest.mark.parametrize('name', ('uniform_cube', 'lattice', 'duplicates'))
def test_against_the_self_search(name):
  """knn_query(p, p, 4) = a column of zeros, then knn(p, 3) bit for bit"""
  p = pair(name)[0]
  cross4 = knn_query(p, p, 4)[0]
  own3 = knn(p, 3)[0]
  assert float(cross4[:, 0].abs().max()) == 0.0
  assert torch.equal(bits(cross4[:, 1:].contiguous()), bits(own3))


def test_pruning_by_the_counters():
  """conditions on the kernels' own counters (module docstring): no clock"""
  p, q, want = pair('uniform_cube')
  m, n = p.shape[0], q.shape[0]
  point_order, query_order, hint = plan(p, q)
  stats = torch.zeros((2,), dtype=torch.int64, device=DEV)
  dist2, index = run_into(p, point_order, q, query_order, hint, 1, stats)
  no.check_cross(q, p, 1, dist2, index, want, "uniform cubes with counters")
  scanned, evals = (int(v) for v in stats.tolist())

  own = torch.zeros((2,), dtype=torch.int64, device=DEV)
  knn_into(p, morton_order(p), 1, torch.empty((m, 1), dtype=torch.float32, device=DEV), None,
           torch.empty((scratch_bytes(m),), dtype=torch.uint8, device=DEV), own)
  own_evals = int(own[1])
  print(f"uniform cubes {m} x {n}, k = 1: {evals} evaluations = {evals / (m * n):.3f} of M N, {evals / n:.0f} per query, "
        f"{scanned / n:.1f} blocks per query; the self search of the points: {own_evals / m:.0f} per query; "
        f"ratio {evals / n / (own_evals / m):.3f}")
  assert evals >= n and scanned >= n                                     # the counters count: at least the seed block
  assert evals / n <= 1.5 * own_evals / m
  assert evals <= 0.5 * m * n

  stats.zero_()
  random_hint = torch.randint(0, m, (n,), generator=torch.Generator().manual_seed(9)).to(torch.int32).to(DEV)
  dist2, index = run_into(p, point_order, q, query_order, random_hint, 1, stats)
  no.check_cross(q, p, 1, dist2, index, want, "uniform cubes, random hint")
  print(f"random hint: {int(stats[1]) / n:.0f} evaluations per query")
  assert n <= int(stats[1]) <= m * n


def test_arguments_are_checked():
  p, q, _ = pair('uniform_cube')
  for k in (0, 9, 1.0, True):
    with pytest.raises(ValueError, match="k must be"):
      knn_query(q, p, k)
  for bad in (torch.zeros((5, 2), device=DEV), torch.zeros((5,), device=DEV), torch.zeros((2, 5, 3), device=DEV), [[0.0, 0.0, 0.0]]):
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
      knn_query(bad, p)
    with pytest.raises(ValueError, match=r"\(N, 3\)"):
      knn_query(q, bad)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    knn_query(q.cpu(), p)
  with pytest.raises(RuntimeError, match="no CPU fallback"):
    knn_query(q, p.cpu())
  for value in (math.nan, math.inf, -math.inf):
    for side in (0, 1):
      sets = [q[:300].clone(), p[:300].clone()]
      sets[side][17, 1] = value
      with pytest.raises(ValueError, match="finite"):
        knn_query(sets[0], sets[1])
  assert MAX_K == 8


def test_on_another_stream():
  p, q, _ = pair('uniform_cube')
  expect = knn_query(q, p, 3)
  stream = torch.cuda.Stream(device=DEV)
  stream.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(stream):
    dist2, index = knn_query(q, p, 3)
  stream.synchronize()
  assert torch.equal(bits(dist2), bits(expect[0])) and torch.equal(index, expect[1])


def test_the_c_call_replays_from_a_graph():
  """points and queries rewritten in place; the orders and the hint of the first pair stay (they decide speed only)"""
  first, second = pair('uniform_cube'), pair('duplicates')
  m, n, k = first[0].shape[0], first[1].shape[0], 3
  points, queries = first[0].clone(), first[1].clone()
  point_order, query_order, hint = plan(points, queries)
  dist2 = torch.zeros((n, k), dtype=torch.float32, device=DEV)
  index = torch.zeros((n, k), dtype=torch.int32, device=DEV)
  scratch = torch.empty((query_scratch_bytes(m, n),), dtype=torch.uint8, device=DEV)
  side = torch.cuda.Stream(device=DEV)
  side.wait_stream(torch.cuda.current_stream(DEV))
  with torch.cuda.stream(side):
    knn_query_into(points, point_order, queries, query_order, hint, k, dist2, index, scratch)      # warm-up outside the capture
  torch.cuda.current_stream(DEV).wait_stream(side)
  graph = torch.cuda.CUDAGraph()
  with torch.cuda.graph(graph):
    knn_query_into(points, point_order, queries, query_order, hint, k, dist2, index, scratch)
  for p, q, want in (first, second, first):
    points.copy_(p)
    queries.copy_(q)
    dist2.zero_()
    index.zero_()
    graph.replay()
    torch.cuda.synchronize()
    assert torch.equal(bits(dist2), bits(knn_query(q, p, k)[0]))
    no.check_cross(q, p, k, dist2, index, want, "graph replay")
