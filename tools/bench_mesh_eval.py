#!/usr/bin/env python
"""Mesh evaluation (csrc/knn_query.hip, csrc/mesh_sample.hip) against its yardsticks — same process, same box, same data.

  knn_query, N queries x N points (default 6 M x 6 M), k = 1, on
    (a) two independent uniform cubes, and
    (b) samples of a unit sphere against samples of a sphere of radius 1.02 (what a mesh evaluation looks like);
    beside the whole call (bounds + two Morton sorts + hint + search): ms_knn_query alone (knn_query_into: gather +
    search), the self search knn_into(p, 1) on the same points, and the kernels' own counters for both.
  chunked torch.cdist + min at --cdist x --cdist (default 200 000), the composition a user would write without the operator.
  sample_mesh_points: N samples of the sphere of tools/bench_mesh.py (--volume 512: 4.8 M triangles) against the torch
    composition (rand, searchsorted over the same cdf, three gathers, a weighted sum).

Events on the stream, warm-up, the variants alternating inside every round, median / min / max over the rounds.  Nothing
here is asserted as a ratio; what is slower is printed as slower.

    python tools/bench_mesh_eval.py [--points 6000000] [--cdist 200000] [--volume 512] [--rounds 10] [--warmup 3]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import TSDFVolume, face_area_cdf, sample_mesh_points                       # noqa: E402
from taichi_splatting_amd.misc.knn import (BLOCK, knn_into, knn_query, knn_query_into, morton_order, query_scratch_bytes,   # noqa: E402
                                           scratch_bytes, _common_bounds, _sorted_codes)


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def interleaved(variants, rounds, warmup):
  times = {k: [] for k in variants}
  for r in range(warmup + rounds):
    for name, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[name].append(ms)
  for name, xs in times.items():
    print(f"  {name:44s} median {statistics.median(xs):9.3f} ms  min {min(xs):9.3f}  max {max(xs):9.3f}")
  return {k: statistics.median(v) for k, v in times.items()}


def on_sphere(n, radius, gen, device):
  p = torch.randn((n, 3), generator=gen, device=device)
  return (p / p.norm(dim=1, keepdim=True) * radius).contiguous()


def cdist_min(queries, points, chunk):
  out = torch.empty((queries.shape[0],), dtype=torch.float32, device=queries.device)
  for begin in range(0, queries.shape[0], chunk):
    out[begin:begin + chunk] = torch.cdist(queries[begin:begin + chunk], points).amin(dim=1)
  return out


def bench_query(name, points, queries, rounds, warmup):
  device = points.device
  m, n = points.shape[0], queries.shape[0]
  print(f"== {name}: {n} queries x {m} points, k = 1, {-(-m // BLOCK)} blocks of {BLOCK}")
  lower, upper = _common_bounds(queries, points)
  point_codes, point_order = _sorted_codes(points, lower, upper)
  query_codes, query_order = _sorted_codes(queries, lower, upper)
  hint = torch.searchsorted(point_codes, query_codes).to(torch.int32)
  dist2 = torch.empty((n, 1), dtype=torch.float32, device=device)
  own = torch.empty((m, 1), dtype=torch.float32, device=device)
  scratch = torch.empty((max(query_scratch_bytes(m, n), 1),), dtype=torch.uint8, device=device)
  own_scratch = torch.empty((scratch_bytes(m),), dtype=torch.uint8, device=device)
  own_order = morton_order(points)

  stats, own_stats, no_hint = (torch.zeros((2,), dtype=torch.int64, device=device) for _ in range(3))
  knn_query_into(points, point_order, queries, query_order, hint, 1, dist2, None, scratch, stats)
  knn_query_into(points, point_order, queries, query_order, None, 1, dist2, None, scratch, no_hint)
  knn_into(points, own_order, 1, own, None, own_scratch, own_stats)
  (scanned, evals), (_, evals_no_hint), (own_scanned, own_evals) = stats.tolist(), no_hint.tolist(), own_stats.tolist()
  print(f"counters, query:       {scanned / n:.1f} blocks scanned and {evals / n:.0f} distances evaluated per query = "
        f"{evals / (m * n):.2e} of M N ({evals_no_hint / n:.0f} per query with the i M / N hint)")
  print(f"counters, self search: {own_scanned / m:.1f} blocks scanned and {own_evals / m:.0f} distances evaluated per query; "
        f"query / self = {evals / n / (own_evals / m):.3f}")
  print(f"mean distance to the nearest point: {float(dist2.sqrt().double().mean()):.4e}")
  median = interleaved({
    'knn_query (bounds, 2 sorts, hint, search)': lambda: knn_query(queries, points, 1, return_indices=False),
    'ms_knn_query alone (gather + search)': lambda: knn_query_into(points, point_order, queries, query_order, hint, 1, dist2,
                                                                    None, scratch),
    'ms_knn_query, i M / N hint': lambda: knn_query_into(points, point_order, queries, query_order, None, 1, dist2, None, scratch),
    'ms_knn_points alone, the points (self, k = 1)': lambda: knn_into(points, own_order, 1, own, None, own_scratch),
  }, rounds, warmup)
  ratio = median['ms_knn_query alone (gather + search)'] / median['ms_knn_points alone, the points (self, k = 1)']
  print(f"query / self search: {ratio:.2f} x in time, {evals / n / (own_evals / m):.2f} x in evaluations per query; "
        f"{evals / median['ms_knn_query alone (gather + search)'] / 1e6:.0f} G distance evaluations per second")


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--points', type=int, default=6_000_000)
  p.add_argument('--cdist', type=int, default=200_000)
  p.add_argument('--volume', type=int, default=512)
  p.add_argument('--rounds', type=int, default=10)
  p.add_argument('--warmup', type=int, default=3)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_mesh_eval: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  gen = torch.Generator(device=device).manual_seed(0)
  n = args.points

  bench_query("two uniform cubes", torch.rand((n, 3), generator=gen, device=device),
              torch.rand((n, 3), generator=gen, device=device), args.rounds, args.warmup)
  bench_query("sphere of radius 1 against sphere of radius 1.02", on_sphere(n, 1.0, gen, device), on_sphere(n, 1.02, gen, device),
              args.rounds, args.warmup)

  c = args.cdist
  points, queries = torch.rand((c, 3), generator=gen, device=device), torch.rand((c, 3), generator=gen, device=device)
  chunk = max(1, (1 << 28) // c)                                        # 1 GiB of float32 distances per chunk
  reference = cdist_min(queries, points, chunk)
  ours = knn_query(queries, points, 1, return_indices=False)[0][:, 0].sqrt()
  print(f"== torch.cdist + min, {c} x {c} uniform cubes in chunks of {chunk} queries; largest difference from knn_query "
        f"{float((reference - ours).abs().max()):.3e}")
  interleaved({'torch.cdist + amin, chunked': lambda: cdist_min(queries, points, chunk),
               'knn_query (one call)': lambda: knn_query(queries, points, 1, return_indices=False)}, args.rounds, args.warmup)

  v = args.volume
  volume = TSDFVolume((-1.0, -1.0, -1.0), 2.0 / (v - 1), (v, v, v), colour=False, device=device)
  volume.tsdf.copy_(((volume.positions().norm(dim=-1) - 0.8) / volume.truncation).clamp(-1, 1))
  volume.weight.fill_(1.0)
  mesh = volume.extract_mesh()
  del volume
  cdf = face_area_cdf(mesh)
  area = float(cdf[-1])
  print(f"== sampling {n} points of the {v}^3 sphere: {mesh.vertices.shape[0]} vertices, {mesh.faces.shape[0]} triangles, "
        f"area {area:.6f} (4 pi 0.8^2 = {4 * 3.141592653589793 * 0.64:.6f})")
  samples = sample_mesh_points(mesh, n)
  print(f"   distance of the samples from the centre: mean {float(samples.points.norm(dim=1).double().mean()):.6f}")

  def torch_samples():
    u = torch.rand((n, 3), device=device)
    face = torch.searchsorted(cdf, u[:, 0].double() * area).clamp_(max=cdf.shape[0] - 1)
    corners = mesh.faces[face].long()
    r = u[:, 1].sqrt()
    wa, wb, wc = 1 - r, r * (1 - u[:, 2]), r * u[:, 2]
    return (wa[:, None] * mesh.vertices[corners[:, 0]] + wb[:, None] * mesh.vertices[corners[:, 1]]
            + wc[:, None] * mesh.vertices[corners[:, 2]])

  interleaved({'sample_mesh_points (areas, cumsum, read, draw)': lambda: sample_mesh_points(mesh, n),
               'face_area_cdf alone (areas + cumsum)': lambda: face_area_cdf(mesh),
               'torch: rand, searchsorted, 3 gathers': torch_samples}, args.rounds, args.warmup)


if __name__ == '__main__':
  main()
