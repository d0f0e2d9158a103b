#!/usr/bin/env python
"""k nearest neighbours of a point cloud (csrc/knn.hip, k = 3): where the time of Gaussians3D.from_point_cloud goes.

Two sets of N points (default 6 M): a uniform cube, and a clustered set (2000 gaussian blobs, sigma log-uniform over
1e-3 .. 5e-2 of the cube, the shape of a structure-from-motion cloud).  Per set, events on the stream, warm-up rounds
first, the variants alternating inside every round, median / min / max over the rounds:

  morton + sort     ms_morton_codes64 + ms_radix_sort_pairs (64-bit codes, bits 0..63) + the index ramp: the `order`
  knn               ms_knn_points with that order: gather + block boxes + search, one call (the split between its two
                    kernels is a kernel trace's to give: rocprofv3 --kernel-trace --stats -- python tools/bench_knn.py)
  sort yardstick    ms_radix_sort_pairs alone on the same N codes: a known, tuned, bandwidth-bound pass over N items

and the search's own counters: blocks scanned and distances evaluated per query, and the share of brute force.

    python tools/bench_knn.py [--n 6000000] [--k 3] [--rounds 10] [--warmup 3]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd.cuda_lib import radix_sort_pairs                             # noqa: E402
from taichi_splatting_amd.misc.knn import BLOCK, _bounds, _codes_in_box, _order_in_box, knn_into, scratch_bytes   # noqa: E402


def event_ms(fn):
  start, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
  start.record()
  fn()
  end.record()
  end.synchronize()
  return start.elapsed_time(end)


def summary(xs):
  return f"median {statistics.median(xs):8.3f} ms  min {min(xs):8.3f}  max {max(xs):8.3f}"


def uniform(n, device, gen):
  return torch.rand((n, 3), device=device, generator=gen)


def clustered(n, device, gen, blobs=2000):
  centre = torch.rand((blobs, 3), device=device, generator=gen)
  sigma = torch.exp(torch.empty((blobs, 1), device=device).uniform_(-6.9, -3.0, generator=gen))      # 1e-3 .. 5e-2
  which = torch.randint(0, blobs, (n,), device=device, generator=gen)
  return (centre[which] + sigma[which] * torch.randn((n, 3), device=device, generator=gen)).contiguous()


def run(name, points, k, rounds, warmup):
  n, device = points.shape[0], points.device
  print(f"== {name}: N = {n}, k = {k}, {(n + BLOCK - 1) // BLOCK} blocks of {BLOCK}")
  lower, upper = _bounds(points)
  order = _order_in_box(points, lower, upper)
  dist2 = torch.empty((n, k), dtype=torch.float32, device=device)
  index = torch.empty((n, k), dtype=torch.int32, device=device)
  scratch = torch.empty((scratch_bytes(n),), dtype=torch.uint8, device=device)

  stats = torch.zeros((2,), dtype=torch.int64, device=device)
  knn_into(points, order, k, dist2, index, scratch, stats)
  scanned, evaluated = (int(v) for v in stats.tolist())
  print(f"counters: {scanned / n:.1f} blocks scanned and {evaluated / n:.0f} distances evaluated per query = "
        f"{evaluated / (n * (n - 1.0)):.2e} of brute force")
  print(f"mean squared distance to the {k} nearest: median {float(dist2.mean(dim=1).median()):.3e}")

  codes = _codes_in_box(points, lower, upper)
  ramp = torch.arange(n, dtype=torch.int32, device=device)

  variants = {
    'morton + sort': lambda: _order_in_box(points, lower, upper),
    'knn (one call)': lambda: knn_into(points, order, k, dist2, index, scratch),
    'sort yardstick': lambda: radix_sort_pairs(codes, ramp, 0, 63),
  }
  times = {key: [] for key in variants}
  for r in range(warmup + rounds):
    for key, fn in variants.items():
      ms = event_ms(fn)
      if r >= warmup:
        times[key].append(ms)
  for key, xs in times.items():
    print(f"{key:16s} {summary(xs)}")
  med = {key: statistics.median(xs) for key, xs in times.items()}
  print(f"knn / sort yardstick: {med['knn (one call)'] / med['sort yardstick']:.1f} x; "
        f"{evaluated / med['knn (one call)'] / 1e6:.0f} G distance evaluations per second; "
        f"points to scales (morton + sort + knn): {med['morton + sort'] + med['knn (one call)']:.1f} ms")


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--n', type=int, default=6_000_000)
  p.add_argument('--k', type=int, default=3)
  p.add_argument('--rounds', type=int, default=10)
  p.add_argument('--warmup', type=int, default=3)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_knn: no GPU visible (there is no CPU fallback to time)")
  device = torch.device('cuda:0')
  print(f"{torch.cuda.get_device_name(device)}; torch {torch.__version__}")
  gen = torch.Generator(device=device).manual_seed(0)
  run('uniform cube', uniform(args.n, device, gen), args.k, args.rounds, args.warmup)
  run('clustered', clustered(args.n, device, gen), args.k, args.rounds, args.warmup)


if __name__ == '__main__':
  main()
