#!/usr/bin/env python
"""What the active SH degree costs or saves: frame forward + backward of ONE degree-3 scene at sh_degree = None, 0, 1, 2, 3.

The scene is the flagship benchmark's (bench.py config D: --n random gaussians, --size^2 pixels, RGB degree 3, tile 16,
loss = image.sum()).  All five variants run in one process on the same tensors, interleaved over --rounds rounds of
--steps steps each (the order rotates per round), timed with device events around the whole round; the table gives the
median and the minimum over the rounds in ms per step.  Nothing is asserted: the numbers go to profiles/sh_active.txt and
decide what DESIGN.md may claim about the feature.

    python tools/bench_sh_active.py [--n 6000000] [--size 2048] [--steps 10] [--rounds 5]
"""
import argparse
import statistics
import sys
from pathlib import Path

import torch

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from taichi_splatting_amd import RasterConfig, render_gaussians                          # noqa: E402
from taichi_splatting_amd.testing import random_camera, random_3d_gaussians               # noqa: E402


def main():
  p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
  p.add_argument('--n', type=int, default=6_000_000)
  p.add_argument('--size', type=int, default=2048)
  p.add_argument('--steps', type=int, default=10)
  p.add_argument('--rounds', type=int, default=5)
  p.add_argument('--seed', type=int, default=0)
  args = p.parse_args()
  if not torch.cuda.is_available():
    sys.exit("bench_sh_active: no GPU visible")
  device = torch.device('cuda:0')
  torch.manual_seed(args.seed)
  cam = random_camera(image_size=(args.size, args.size))
  g = random_3d_gaussians(args.n, cam, scale_factor=1.0, alpha_range=(0.1, 0.9), margin=0.0)
  g = g.replace(feature=(torch.rand(args.n, 3, 16) - 0.5) * 0.5).to(device).requires_grad_(True)
  cam = cam.to(device=device)
  cfg = RasterConfig(tile_size=16)
  leaves = [g.position, g.log_scaling, g.rotation, g.alpha_logit, g.feature]

  def step(degree):
    for t in leaves:
      t.grad = None
    render_gaussians(g, cam, cfg, use_sh=True, sh_degree=degree).image.sum().backward()

  variants = [None, 0, 1, 2, 3]
  for degree in variants:                     # capacities, mapper choice, allocator, code objects
    for _ in range(3):
      step(degree)
  torch.cuda.synchronize()
  times = {degree: [] for degree in variants}
  for r in range(args.rounds):
    for degree in variants[r % len(variants):] + variants[:r % len(variants)]:
      begin, end = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
      begin.record()
      for _ in range(args.steps):
        step(degree)
      end.record()
      end.synchronize()
      times[degree].append(begin.elapsed_time(end) / args.steps)
  print(f"{torch.cuda.get_device_name(0)}; torch {torch.__version__}; N = {args.n}, {args.size}^2, stored SH degree 3, "
        f"tile 16, fwd+bwd, {args.rounds} rounds x {args.steps} steps, ms per step")
  for degree in variants:
    ms = times[degree]
    print(f"sh_degree={str(degree):>4}   median {statistics.median(ms):7.3f}   min {min(ms):7.3f}   rounds "
          + " ".join(f"{t:.3f}" for t in ms), flush=True)


if __name__ == '__main__':
  main()
